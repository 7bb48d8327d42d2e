"""CPU: the confidence contract off the GPU — tests/score_reference.py against a direct float64 log_softmax of the filtered row,
AX_WHISPER_LongWindowIsSilent on a table, the seek loop under the silent-window rule, the new kernels' resources in both builds
and the new exports."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import longform_reference as lfr
import score_reference as sr
import ts_reference as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["AX_WHISPER_RunPCMBatchTimestampScores", "AX_WHISPER_DecodeForcedTimestampScores", "AX_WHISPER_ScoreTimestampRules",
               "AX_WHISPER_NoSpeechLogProb", "AX_WHISPER_LongWindowIsSilent", "AX_WHISPER_RunPCMLongWindowsScored",
               "AX_WHISPER_RunPCMLongOpts", "AX_WHISPER_RunFileLongOpts"]
E = 50257


def _T(nv):
    return 50364 if nv == 51865 else 50365


def _log_softmax64(x, mask):
    """torch's float64 log_softmax over the entries of `mask` (an implementation that shares nothing with the reference's)"""
    import torch

    f = torch.tensor(np.where(mask, np.asarray(x, dtype=np.float64), -np.inf), dtype=torch.float64)
    return torch.log_softmax(f, dim=0).numpy()


@pytest.mark.parametrize("nv", [51865, 51866])
def test_reference_matches_a_direct_log_softmax(nv):
    T = _T(nv)
    seen_inf = seen_rule5 = 0
    for name, x, seq, want in tsr.crafted_cases(nv):
        c, lp, info = sr.token_logprob(x, seq, T, E)
        assert c == want, (name, c, want)
        A = sr.final_allowed(x, seq, T, E)
        finite = A & np.isfinite(np.asarray(x, dtype=np.float64))
        if not finite.any():  # nothing finite left: the decision is eot, its log-probability -inf
            assert c == E and lp == -np.inf, (name, c, lp)
            seen_inf += 1
            continue
        ls = _log_softmax64(x, A)
        assert abs(float(lp) - float(ls[c])) <= 1e-6 + 1e-7 * abs(float(ls[c])), (name, float(lp), float(ls[c]))
        assert lp <= 0.0
        seen_rule5 += info["rule5"]
        if info["rule5"]:  # the text ids are outside the normaliser
            assert not A[:T].any()
    assert seen_inf == 2 and seen_rule5 >= 1


def test_reference_edge_cases():
    nv, T = 51865, _T(51865)
    base = lambda v=-10.0: np.full(nv, v, dtype=np.float32)
    # chosen logit +inf: 0
    x = base(); x[7] = np.inf
    c, lp, _ = sr.token_logprob(x, [T, 5], T, E)
    assert c == 7 and lp == 0.0
    # NaN entries are neither chosen nor in the normaliser
    x = base(-np.inf); x[4] = np.nan; x[6] = 1.0; x[9] = 1.0 - math.log(3.0)
    c, lp, _ = sr.token_logprob(x, [T, 5], T, E)
    assert c == 6 and abs(float(lp) - math.log(0.75)) < 1e-6
    # logits near +-80: the maximum is subtracted first, nothing overflows (exp(80) * 50000 would in float32: 2.8e39)
    rng = np.random.default_rng(5)
    x = rng.uniform(-80.0, 80.0, nv).astype(np.float32)
    x[:2000] = 80.0
    x[T:] = np.minimum(x[T:], 0.0)  # (the timestamps' mass stays below the best text id: rule 5 does not fire)
    c, lp, info = sr.token_logprob(x, [T, 5], T, E)
    assert c == 0 and not info["rule5"]
    A = sr.final_allowed(x, [T, 5], T, E)
    ls = _log_softmax64(x, A)
    assert np.isfinite(lp) and abs(float(lp) - float(ls[c])) < 1e-5 and float(lp) < -7.0  # 2000 ids share the maximum: below -log(2000)
    # no-speech: the whole row, NaN left out; -inf / +inf rows
    ns = T - 2
    full = np.ones(nv, dtype=bool)
    nsp = sr.no_speech_logprob(x, ns)
    assert abs(float(nsp) - float(_log_softmax64(x, full)[ns])) < 1e-5
    y = x.copy(); y[100] = np.nan
    full[100] = False
    assert abs(float(sr.no_speech_logprob(y, ns)) - float(_log_softmax64(y, full)[ns])) < 1e-5
    assert sr.no_speech_logprob(base(-np.inf), ns) == -np.inf
    y = base(); y[ns] = np.inf
    assert sr.no_speech_logprob(y, ns) == 0.0
    y = base(); y[3] = np.inf
    assert sr.no_speech_logprob(y, ns) == -np.inf
    # a uniform row: -log(n)
    assert abs(float(sr.no_speech_logprob(base(3.0), ns)) + math.log(nv)) < 1e-6


def test_reference_average():
    lp = np.array([-1.0, -2.0, -3.0, -0.5], dtype=np.float32)
    assert sr.avg_logprob(lp, 3, True) == np.float32(-6.5 / 4)   # the eot decision counts
    assert sr.avg_logprob(lp, 3, False) == np.float32(-6.0 / 4)  # an id dropped at the budget does not
    assert sr.avg_logprob(np.array([-0.25], dtype=np.float32), 0, True) == np.float32(-0.25)
    assert sr.avg_logprob(np.array([-0.25], dtype=np.float32), 0, False) == np.float32(0.0)


SILENT_TABLE = [
    # no_speech_logprob, avg_logprob, no_speech_threshold, logprob_threshold, silent
    (math.log(0.9), -2.0, 0.6, -1.0, True),
    (math.log(0.9), -0.5, 0.6, -1.0, False),       # confident text overrides no-speech
    (math.log(0.3), -2.0, 0.6, -1.0, False),
    (float(np.log(np.float32(0.5))), -2.0, float(np.exp(np.log(np.float32(0.5)))), -1.0, False),  # equality on no-speech: strict >
    (math.log(0.9), -1.0, 0.6, -1.0, True),        # equality on the average: "not >" holds
    (math.log(0.9), 0.0, 0.6, math.inf, True),     # +inf: no-speech alone decides
    (math.log(0.3), -50.0, 0.6, math.inf, False),
    (-324.39, -8.0, 0.6, -1.0, False),             # exp underflows to 0 in float32
    (-324.39, -8.0, 0.0, -1.0, False),             # 0 > 0 is false
    (0.0, -math.inf, 0.999, -1.0, True),
    (math.log(0.9), -2.0, math.nan, -1.0, False),  # NaN no-speech threshold: the rule is off
    (math.log(0.9), -2.0, math.nan, math.inf, False),
    (math.nan, -2.0, 0.6, -1.0, False),            # a NaN no-speech value is never above a threshold
    (math.log(0.9), math.nan, 0.6, -1.0, True),    # a NaN average is not above its threshold
    (math.log(0.9), -2.0, -1.0, -math.inf, False),
]


def test_long_window_is_silent_table(built_lib):
    for nsp, avg, nst, lpt, want in SILENT_TABLE:
        assert sr.is_silent(nsp, avg, nst, lpt) == want, (nsp, avg, nst, lpt)
        assert built_lib.long_window_is_silent(nsp, avg, nst, lpt) == want, (nsp, avg, nst, lpt)
    rng = np.random.default_rng(3)
    for _ in range(2000):
        nsp, avg = -float(rng.exponential(1.0)), -float(rng.exponential(1.5))
        nst, lpt = float(rng.choice([0.2, 0.6, 0.9])), float(rng.choice([-1.0, -0.3, math.inf]))
        assert built_lib.long_window_is_silent(nsp, avg, nst, lpt) == sr.is_silent(nsp, avg, nst, lpt)


def test_loop_under_the_silent_window_rule():
    T = _T(51865)
    n_samples = lfr.LENGTHS[5]  # 100 s
    # every window: a closed pair ending at 20.00 s, then an open tail -> advance 2000 frames unless the window is short
    ids_of = lambda seek, wf: [T, 5, 6, T + 200, T + 200, 7, T + 1000, T + 1000, 8]
    silent_seeks = {2000, 6000}
    score = lambda seek, wf: (math.log(0.95), -3.0) if seek in silent_seeks else (math.log(0.01), -0.4)
    plain = lfr.loop(n_samples, ids_of, T, E)
    got = sr.loop_scored(n_samples, ids_of, score, T, E, 0.6, -1.0)
    assert [w[0] for w in plain] == [0, 2000, 4000, 6000, 8000]
    # a silent window moves on by its whole length, so the windows after it sit elsewhere than in the plain loop
    assert [(w[0], w[2], w[5]) for w in got] == [(0, 2000, False), (2000, 3000, True), (5000, 2000, False), (7000, 2000, False), (9000, 1000, False)]
    for seek, wf, adv, ids, segs, skipped in got:
        if skipped:
            assert segs == [] and adv == wf
        else:
            want_segs, want_adv, _ = lfr.split_window(ids, T, E, wf)
            assert segs == want_segs and adv == want_adv and len(segs) >= 1
    # thresholds off: the plain loop, window for window
    off = sr.loop_scored(n_samples, ids_of, score, T, E, math.nan, math.inf)
    assert [(w[0], w[1], w[2], w[3]) for w in off] == plain and not any(w[5] for w in off)
    # everything silent: full advances, no segments
    every = sr.loop_scored(n_samples, ids_of, lambda s, w: (0.0, -9.0), T, E, 0.6, -1.0)
    assert [w[0] for w in every] == [0, 3000, 6000, 9000] and all(w[5] and not w[4] and w[2] == w[1] for w in every)


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_scored_kernels_compile_without_scratch_or_spills(f16, tmp_path):
    out = tmp_path / "ts.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out),
                        os.path.join(ROOT, "whisper.axera_amd", "csrc", "decode_timestamps.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    for k in ("timestamp_rules_kernel", "timestamp_rules_scored_kernel", "row_logprob_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M) == ["0"] * len(names)
    assert all(int(x) == 0 for x in re.findall(r"^\s+\.(?:vgpr|sgpr)_spill_count:\s+(\d+)", text, re.M))
    vg = dict(zip(names, (int(x) for x in re.findall(r"^\s+\.vgpr_count:\s+(\d+)", text, re.M))))
    assert all(v <= 64 for v in vg.values()), vg  # 256-thread workgroups, eight of them per CU wanted: far below any occupancy step


def test_new_symbols_are_exported_and_bound(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    assert set(NEW_SYMBOLS) <= set(built_lib.SYMBOLS)
    for m in ("run_timestamp_scores_batch", "decode_forced_timestamp_scores", "score_timestamp_rules", "no_speech_logprob", "run_long_scored"):
        assert callable(getattr(built_lib.Whisper, m))


def test_scored_calls_reject_null_arguments(built_lib):
    import ctypes as C

    L = built_lib.load_library()
    n = C.c_int()
    assert L.AX_WHISPER_RunPCMBatchTimestampScores(None, None, None, 1, 0, None, None, None, None, None, None, None) == -1
    assert L.AX_WHISPER_DecodeForcedTimestampScores(None, 1, None, 0, None, None, None, None, None) == -1
    assert L.AX_WHISPER_ScoreTimestampRules(None, None, None, None, 1, None, None) == -1
    assert L.AX_WHISPER_NoSpeechLogProb(None, None, 1, None) == -1
    assert L.AX_WHISPER_RunPCMLongWindowsScored(None, None, None, 1, 0, 0, 0.6, -1.0, 0, None, None, None, C.byref(n)) == -1
    out = C.c_void_p()
    assert L.AX_WHISPER_RunPCMLongOpts(None, None, 0, 0.6, -1.0, C.byref(out)) == -1
    assert L.AX_WHISPER_RunFileLongOpts(None, b"x.wav", 0.6, -1.0, C.byref(out)) == -1
