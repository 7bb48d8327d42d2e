"""CPU: the language definitions off the GPU — the pick rule of tests/lang_reference.py in numpy, the context function, LangCase on
the oracle (its conditions: enough clips keep the margin, enough distinct languages among them), that the new calls
exist and refuse a NULL handle (their numbering against the config needs an engine: tests/test_gpu_language.py), and the option
checks of whisper_cli that happen before a model is opened."""
import ctypes as C
import os

import numpy as np
import pytest

import lang_reference as lr
import prompt_reference as pr


def test_pick_rule():
    x = np.array([0.5, 3.0, -1.0, 3.0, 2.0], dtype=np.float32)
    idx, lp = lr.pick(x, 4)
    assert idx == 1  # ties go to the lower index
    assert lp[1] == lp[3] and lp.dtype == np.float32
    want = x.astype(np.float64) - np.log(np.exp(x.astype(np.float64)).sum())
    assert np.abs(lp - want).max() < 1e-6 and abs(float(np.exp(lp.astype(np.float64)).sum()) - 1.0) < 1e-6
    # NaN is left out: never the winner, not in the normaliser, -inf in the output
    y = x.copy()
    y[1] = np.nan
    idx, lp = lr.pick(y, 4)
    assert idx == 3 and lp[1] == -np.inf
    keep = np.array([0, 2, 3, 4])
    want = y[keep].astype(np.float64) - np.log(np.exp(y[keep].astype(np.float64)).sum())
    assert np.abs(lp[keep] - want).max() < 1e-6
    # -inf entries stay in: they add nothing
    y = x.copy()
    y[0] = -np.inf
    idx, lp = lr.pick(y, 4)
    assert idx == 1 and lp[0] == -np.inf and np.isfinite(lp[1:]).all()
    # nothing finite: the handle's language, all -inf
    for row in (np.full(5, np.nan), np.full(5, -np.inf), np.array([np.nan, -np.inf, np.nan, -np.inf, np.nan]),
                np.array([np.inf, np.nan, np.nan, np.nan, np.nan]), np.array([np.inf, -np.inf, np.nan, np.inf, np.nan]), np.full(5, np.inf)):
        idx, lp = lr.pick(row.astype(np.float32), 2)
        assert idx == 2 and (lp == -np.inf).all()
    # +inf beside a finite entry: something is finite, so the first +inf wins and the infinities share the whole mass
    idx, lp = lr.pick(np.array([1.0, np.inf, np.nan, np.inf, -3.0], dtype=np.float32), 0)
    assert idx == 1 and lp.tolist() == [-np.inf, 0.0, -np.inf, 0.0, -np.inf]
    # large logits: the maximum is subtracted first
    big = np.array([80.0, 79.0, -80.0], dtype=np.float32)
    idx, lp = lr.pick(big, 0)
    assert idx == 0 and np.isfinite(lp).all() and abs(float(lp[0]) + np.log1p(np.exp(-1.0))) < 1e-6


def test_context_function():
    import modelgen

    cfg = modelgen.make_config("micro", modelgen.DIMS["micro"])
    toks, codes = lr.lang_tokens(cfg), lr.lang_codes(cfg)
    assert len(toks) == len(codes) and len(toks) in (99, 100)
    zh = codes.index("zh")
    sot, tr, tl = int(cfg["sot"]), int(cfg["transcribe"]), int(cfg["translate"])
    assert lr.context(cfg, [], 3, 0) == [sot, toks[3], tr]
    assert lr.context(cfg, [], zh, 1) == [sot, toks[zh], tl]
    prompt = list(range(300))
    ctx = lr.context(cfg, prompt, 5, 0)
    assert ctx == [int(cfg["sot_prev"])] + prompt[-lr.KEEP:] + [sot, toks[5], tr] and len(ctx) - 1 == lr.KEEP + 3
    # the handle's language and transcribe: the prompted context of tests/prompt_reference.py
    assert lr.context(cfg, [7, 8], zh, 0) == pr.context(cfg, [7, 8], [sot, toks[zh], tr])
    # who needs a context
    assert not lr.needs_context(0, -1, 0, zh) and not lr.needs_context(0, zh, 0, zh)
    assert lr.needs_context(1, -1, 0, zh) and lr.needs_context(0, -2, 0, zh) and lr.needs_context(0, -1, 1, zh) and lr.needs_context(0, 3, 0, zh)


@pytest.fixture(scope="module", params=lr.MODELS, ids=["micro_bf16", "miniturbo_fp16"])
def case(request, oracle_mod):
    return lr.LangCase(*request.param)


def test_lang_case_conditions(case):
    kept = case.kept()
    ex = [case.expect(i) for i in range(lr.N_CLIPS)]
    winners = {ex[i]["index"] for i in kept}
    print("%s: %d distinct winners over all clips, smallest margin %.3g, %d kept, %d distinct among them, largest logit %.3g"
          % (case.model_type, len({e["index"] for e in ex}), min(e["margin"] for e in ex), len(kept), len(winners),
             max(float(e["lang_logit"].max()) for e in ex)))
    assert len(kept) >= 12 and len(winners) >= 3
    tok, K = case.tokens, lr.K
    emb = case.weights["decoder.token_embedding.weight"]
    others = np.setdiff1d(np.arange(emb.shape[0]), tok)
    assert not emb[others][:, :K].any() and not emb[tok][:, K:].any()  # the K coordinates reach the languages' logits and nothing else
    for e in ex:  # the oracle's values obey the pick rule
        idx, lp = lr.pick(e["lang_logit"], case.handle_index)
        assert idx == e["index"] and np.array_equal(lp, e["lang_logprob"])


def test_language_index_and_code_against_the_config(built_lib, tmp_path):
    """Host only, and no more than this: no engine is made (that needs a GPU), so the new calls are checked to exist, to be bound in
    Python and to refuse a NULL handle. The numbering against the config is checked where an engine exists, in
    tests/test_gpu_language.py::test_language_index_and_code_against_the_config."""
    L = built_lib.load_library()
    assert L.AX_WHISPER_LanguageIndex(None, b"en") == -1
    assert L.AX_WHISPER_LanguageCode(None, 0) is None
    for name in ("AX_WHISPER_LanguageIndex", "AX_WHISPER_LanguageCode", "AX_WHISPER_DetectLanguage", "AX_WHISPER_RunPCMBatchTimestampLang",
                 "AX_WHISPER_DetectLanguageStage", "AX_WHISPER_LanguageLogProbRows", "AX_WHISPER_PrefillContexts", "AX_WHISPER_DecodeForcedTimestampLang",
                 "AX_WHISPER_RunPCMLongWindowsLang", "AX_WHISPER_RunPCMLongLang", "AX_WHISPER_RunFileLongLang", "AX_WHISPER_TranscriptLang"):
        assert name in built_lib.SYMBOLS and hasattr(L, name)
    n = C.c_int()
    assert L.AX_WHISPER_DetectLanguage(None, None, None, 1, C.byref(n), None) == -1
    assert L.AX_WHISPER_DetectLanguageStage(None, 1, C.byref(n), None, None) == -1
    assert L.AX_WHISPER_LanguageLogProbRows(None, None, 1, None, None, None) == -1
    assert L.AX_WHISPER_PrefillContexts(None, 1, None, 0, None, None, None, None, None, None, None) == -1
    out = C.c_void_p()
    assert L.AX_WHISPER_RunPCMLongLang(None, None, 1, 0.0, 0.0, 0.0, None, 0, 0, None, 0, 0, -2, 0, None, C.byref(out)) == -1
    assert L.AX_WHISPER_RunFileLongLang(None, b"x.wav", 0.0, 0.0, 0.0, None, 0, 0, None, 0, 0, -2, 0, None, C.byref(out)) == -1
    assert L.AX_WHISPER_TranscriptLang(None, None, 0, 0, C.byref(out)) == -1
    for m in ("detect_language", "run_timestamp_lang_batch", "prefill_contexts", "decode_forced_timestamp_lang", "language_logprob_rows",
              "language_index", "language_code", "transcript_lang"):
        assert callable(getattr(built_lib.Whisper, m))
    import inspect

    for m in ("run_long_windows", "run_long_scored", "run_long_text"):
        sig = inspect.signature(getattr(built_lib.Whisper, m)).parameters
        assert sig["languages"].default is None and sig["tasks"].default is None


def test_cli_refuses_language_options_without_a_mode(built_lib):
    """whisper_cli: --detect_language and --task need --timestamps or --long, do not go with --beam_size, and --task takes two
    values; all of it is decided before a model is opened, so this runs without a GPU."""
    import subprocess

    cli = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_cli")
    for args, word in ((["--detect_language"], "need --timestamps or --long"), (["--task", "translate"], "need --timestamps or --long"),
                       (["--timestamps", "--task", "summarise"], "bad value: --task"),
                       (["--timestamps", "--beam_size", "2", "--detect_language"], "do not go with --beam_size")):
        r = subprocess.run([cli, "--wav", "none.wav"] + args, capture_output=True, text=True, timeout=30)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr[-300:])
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=30)
    assert "--detect_language" in r.stderr and "--task" in r.stderr
