"""GPU: word-level timestamps end to end (DESIGN.md "Word-level timestamps") on micro bf16 and miniturbo fp16, demo.wav and a 1 s clip
of it (50 encoder frames: far from a block edge, so the key-count mask matters), against tests/word_reference.py.

The models carry modelgen.realistic_weights: with seeded N(0, 0.02) weights every cross-attention row is flat to 1e-6 of 1 / F, the
z-scores of such a matrix are rounding noise of the 16-bit activations, and no alignment path over it is stable (word_reference.py,
"the cases of the GPU word tests").

The float64 reference is fed the ENGINE's cross K / V (AX_WHISPER_GetCrossKV), so what is measured is the teacher-forced decoder pass
and the alignment kernels, not the encoder."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import word_reference as wr
from conftest import GOLDEN, ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

TABLE_PATH = os.path.join(GOLDEN, "multilingual.tiktoken")
CLIPS = ("demo", "1s")


@pytest.fixture(scope="module", params=wr.MODELS, ids=[m[0] for m in wr.MODELS])
def model(request, tmp_path_factory, built_lib, oracle_mod):
    model_type, seed, dtype = request.param
    case = ModelCase(tmp_path_factory.mktemp("words_" + model_type), model_type, seed, dtype=dtype, kind="realistic")
    eng = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=5)
    demo = load_demo_pcm()
    m = types.SimpleNamespace(case=case, cfg=case.cfg, eng=eng, lib=built_lib, table=wr.load_table(TABLE_PATH),
                              clips={"demo": demo, "1s": demo[16000:32000].copy()}, lang_tok=case.oracle_fp32.sot_seq("zh")[1], cache={},
                              meps=wr.MATRIX_EPS[model_type], lpeps=wr.LOGPROB_EPS[model_type])
    yield m
    eng.close()


def frames_of(pcm):
    return min(len(pcm) // 160, 3000)


def encoded(m, name):
    """the clip in slot 0 and the engine's own cross K / V of it"""
    mel = m.eng.compute_mel(m.clips[name])
    m.eng.encode_mel(mel)
    if name not in m.cache:
        m.cache[name] = (mel, *m.eng.get_cross_kv(0))
    return m.cache[name]


def measure(m, name, ids, heads=None):
    """one alignment of `ids` over the clip -> (the engine's result, the float64 reference, matrix error, log-probability error)"""
    _, ck, cv = encoded(m, name)
    fr = frames_of(m.clips[name])
    got = m.eng.align_tokens([ids], [fr], want_matrix=True)[0]
    ref = wr.find_alignment(m.cfg, m.case.weights, ck, cv, ids, fr, m.lang_tok, heads=heads)
    assert got["matrix"].shape == ref["matrix"].shape and np.isfinite(got["matrix"]).all()
    return got, ref, float(np.abs(got["matrix"] - ref["matrix"]).max()), float(np.abs(got["token_logprob"] - ref["token_logprob"]).max())


def test_matrix_jumps_and_logprobs(model):
    """(a) the matrix and the token log-probabilities against float64 within the measured tolerances; (b) the jumps are the float32 DTW
    of the returned matrix, bit for bit; (d) on admissible cases they are the float64 reference's jumps, and every model has one"""
    m = model
    eot = int(m.cfg["eot"])
    worst_m = worst_lp = 0.0
    n_admissible = 0
    for name in CLIPS:
        compared = False
        for sd in range(wr.MAX_SEEDS):  # every seed enters the error bound; the first admissible one of a clip the jump comparison
            ids = wr.case_ids(eot, sd)
            got, ref, em, elp = measure(m, name, ids)
            worst_m, worst_lp = max(worst_m, em), max(worst_lp, elp)
            n = len(ids)
            assert np.array_equal(got["jump"], wr.align_path(got["matrix"][3: n + 4], np.float32)), (name, sd)
            if not compared and wr.admissible(ref["matrix"], n, m.meps):
                compared = True
                n_admissible += 1
                assert np.array_equal(got["jump"], ref["jump"]), (name, sd, got["jump"], ref["jump"])
    print(f"{m.case.model_type}: matrix error {worst_m:.3e} (bound {m.meps:.1e}), log-probability error {worst_lp:.3e} "
          f"(bound {m.lpeps:.1e}), admissible cases {n_admissible}")
    assert worst_m <= m.meps and worst_lp <= m.lpeps
    assert n_admissible >= 1


def test_gpu_route_and_host_route_agree(model, monkeypatch):
    """(e) AX_WHISPER_WORD_ALIGN=host: normalisation, median and path in C++ on the host give the same jumps (and the same matrix to the
    bit: the host code adds in the kernel's order)"""
    m = model
    assert m.eng.get_config_int("word_align") == 0
    monkeypatch.setenv("AX_WHISPER_WORD_ALIGN", "host")
    host = m.lib.Whisper(m.case.model_type, m.case.root, "zh", device=0, max_batch=1)
    monkeypatch.delenv("AX_WHISPER_WORD_ALIGN")
    try:
        assert host.get_config_int("word_align") == 1
        for name in CLIPS:
            ids = wr.case_ids(int(m.cfg["eot"]), 3)
            mel, _, _ = encoded(m, name)
            fr = frames_of(m.clips[name])
            a = m.eng.align_tokens([ids], [fr], want_matrix=True)[0]
            host.encode_mel(mel)
            b = host.align_tokens([ids], [fr], want_matrix=True)[0]
            assert np.array_equal(a["jump"], b["jump"]) and np.array_equal(a["token_logprob"], b["token_logprob"])
            assert np.array_equal(a["matrix"], b["matrix"])
    finally:
        host.close()


def test_batches_ragged_lengths_and_refusals(model):
    """(f) batches of 1, 2 and 5 clips with ragged id counts: every clip's result is that of the clip alone; no ids give nothing; a
    context beyond n_text_ctx is refused"""
    m = model
    eot = int(m.cfg["eot"])
    demo = m.clips["demo"]
    pcms = [demo, m.clips["1s"], demo[:40000], demo[8000:30000], demo[20000:]]
    mels = [m.eng.compute_mel(p) for p in pcms]
    ns = [14, 1, 0, 70, 33]
    ids = [wr.case_ids(eot, 20 + b, ns[b]) for b in range(5)]
    alone = []
    for b in range(5):
        m.eng.encode_mel(mels[b])
        alone.append(m.eng.align_tokens([ids[b]], [frames_of(pcms[b])], want_matrix=True)[0])
    assert alone[2]["jump"].size == 0 and alone[2]["token_logprob"].size == 0 and alone[2]["matrix"].size == 0
    for B in (2, 5):
        m.eng.encode_mel(np.stack(mels[:B]))
        got = m.eng.align_tokens(ids[:B], [frames_of(p) for p in pcms[:B]], want_matrix=True)
        for b in range(B):
            # (the GEMMs of a longer pass may add in another order: the clip alone is matched within the tolerances, not to the bit)
            assert got[b]["matrix"].shape == alone[b]["matrix"].shape and got[b]["jump"].shape == alone[b]["jump"].shape
            if ns[b] == 0:
                continue
            assert np.abs(got[b]["matrix"] - alone[b]["matrix"]).max() <= m.meps, (B, b)
            assert np.abs(got[b]["token_logprob"] - alone[b]["token_logprob"]).max() <= m.lpeps, (B, b)
            assert np.array_equal(got[b]["jump"], wr.align_path(got[b]["matrix"][3: ns[b] + 4], np.float32)), (B, b)
    with pytest.raises(RuntimeError):
        m.eng.align_tokens([[1] * (m.eng.n_text_ctx - 4)], [3000])
    with pytest.raises(RuntimeError):
        m.eng.align_tokens([[eot]], [3000])  # not a text id
    with pytest.raises(RuntimeError):
        m.eng.align_tokens([[1, 2]], [1])  # no encoder frame to align against


def test_words_are_the_host_rule_on_the_calls_own_alignment(model):
    """(c) run_word_timestamps_batch: the words are the Python rule applied to the jumps, log-probabilities and ids the call returns;
    under zh (unicode groups) and under en (the space rule), batches 1, 2 and 5"""
    m = model
    demo = m.clips["demo"]
    pcms = [demo, m.clips["1s"], demo[:40000], demo[8000:30000], demo[20000:]]
    T, eot = m.eng.timestamp_begin, int(m.cfg["eot"])
    n_words = 0
    for B, langs in ((1, None), (2, ["en", "zh"]), (5, ["en", "en", "zh", "de", "ja"])):
        res = m.eng.run_word_timestamps_batch(pcms[:B], languages=langs)
        plain = m.eng.run_timestamp_lang_batch(pcms[:B], languages=langs) if langs else [dict(ids=i) for i in m.eng.run_timestamp_tokens_batch(pcms[:B])]
        for b, r in enumerate(res):
            assert r["ids"] == plain[b]["ids"], (B, b)  # the ids of the greedy timestamp decode
            spans = m.lib.split_segments(r["ids"], T, eot, min(len(pcms[b]) / 16000.0, 30.0))
            seg_tokens = [sum(1 for t in r["ids"][tb:te] if t < eot) for (_, _, tb, te) in spans]
            # (a clip that never reaches eot has more text ids than a context holds: the call aligns the first n_text_ctx - 5)
            n_text = min(sum(seg_tokens), m.eng.n_text_ctx - 5)
            for k in range(len(seg_tokens)):
                seg_tokens[k] = min(seg_tokens[k], n_text - sum(seg_tokens[:k]))
            assert n_text == len(r["text_ids"]) == len(r["token_logprob"]) and len(r["jump"]) == n_text + 1
            ref, rs, re_ = wr.words_from_alignment(m.table, r["text_ids"], eot, r["language"], seg_tokens, [s[0] for s in spans], [s[1] for s in spans],
                                                   r["jump"], r["token_logprob"])
            assert [w[:4] for w in r["words_bytes"]] == [w[:4] for w in ref], (B, b)
            assert np.allclose([w[4] for w in r["words_bytes"]], [w[4] for w in ref], rtol=2e-7, atol=0)
            assert [s[0] for s in r["segments"]] == rs and [s[1] for s in r["segments"]] == re_
            n_words += len(ref)
    assert n_words > 0
    segs = m.eng.run_word_timestamps(demo)
    assert segs == m.eng.run_word_timestamps_batch([demo])[0]["segments"]


def test_head_list_changes_the_matrix(model):
    """(g) a handle's own alignment heads: the matrix is the reference's under that list, and another than the default one"""
    m = model
    ids = wr.case_ids(int(m.cfg["eot"]), 5)
    base, _, _, _ = measure(m, "1s", ids)
    assert m.eng.get_config_int("n_alignment_heads") == len(wr.default_heads(m.cfg))
    m.eng.set_alignment_heads([(0, 1), (1, 0)])
    try:
        assert m.eng.get_config_int("n_alignment_heads") == 2
        got, ref, em, _ = measure(m, "1s", ids, heads=[(0, 1), (1, 0)])
        assert em <= m.meps and not np.allclose(got["matrix"], base["matrix"], atol=10 * m.meps)
        with pytest.raises(RuntimeError):
            m.eng.set_alignment_heads([(0, 99)])
    finally:
        m.eng.set_alignment_heads(None)
    again, _, _, _ = measure(m, "1s", ids)
    assert np.array_equal(again["matrix"], base["matrix"])


def test_config_file_heads_are_the_handles_heads(model, tmp_path):
    """a model directory whose config names alignment_heads: a handle on it aligns with them from the start, and n = 0 restores them"""
    import modelgen

    m = model
    heads = [(0, 1), (1, 0)]
    modelgen.write_model_dir(str(tmp_path), m.case.model_type, m.case.dims, weights=m.case.weights, dtype=m.case.dtype, tiktoken_path=TABLE_PATH,
                             alignment_heads=heads)
    ids = wr.case_ids(int(m.cfg["eot"]), 5)
    mel, ck, cv = encoded(m, "1s")
    fr = frames_of(m.clips["1s"])
    m.eng.set_alignment_heads(heads)
    try:
        want = m.eng.align_tokens([ids], [fr], want_matrix=True)[0]
    finally:
        m.eng.set_alignment_heads(None)
    e = m.lib.Whisper(m.case.model_type, str(tmp_path), "zh", device=0, max_batch=1)
    try:
        assert e.get_config_int("n_alignment_heads") == 2
        e.encode_mel(mel)
        got = e.align_tokens([ids], [fr], want_matrix=True)[0]
        assert np.array_equal(got["matrix"], want["matrix"]) and np.array_equal(got["jump"], want["jump"])
        e.set_alignment_heads([(1, 1)])
        assert e.get_config_int("n_alignment_heads") == 1
        e.set_alignment_heads(None)
        assert e.get_config_int("n_alignment_heads") == 2
        assert np.array_equal(e.align_tokens([ids], [fr], want_matrix=True)[0]["matrix"], want["matrix"])
    finally:
        e.close()


def test_alignment_leaves_the_decode_alone(model):
    """(h) a timestamp decode after an alignment call on the same handle is bit-equal to one before it"""
    m = model
    pcms = [m.clips["demo"], m.clips["1s"]]
    before = m.eng.run_timestamp_scores_batch(pcms)
    m.eng.run_word_timestamps_batch(pcms)
    encoded(m, "demo")
    m.eng.align_tokens([wr.case_ids(int(m.cfg["eot"]), 9, 100)], [frames_of(m.clips["demo"])])
    after = m.eng.run_timestamp_scores_batch(pcms)
    for a, b in zip(before, after):
        assert a["ids"] == b["ids"] and np.array_equal(a["token_logprob"], b["token_logprob"]) and a["no_speech_logprob"] == b["no_speech_logprob"]


def test_cli_prints_words(model):
    """(i) whisper_cli --timestamps --word_timestamps: one indented line per word under its segment's line"""
    m = model
    cli = os.path.join(os.path.dirname(m.lib.LIB_PATH), "whisper_cli")
    args = [cli, "-w", os.path.join(GOLDEN, "demo.wav"), "-t", m.case.model_type, "-p", m.case.root, "--language", "zh", "--timestamps"]
    r = subprocess.run(args + ["--word_timestamps"], capture_output=True, timeout=120)
    out = r.stdout.decode("utf-8", "replace")
    assert r.returncode == 0, (out[-400:], r.stderr[-400:])
    want = m.eng.run_word_timestamps_batch([m.clips["demo"]])[0]
    # (a word may hold any bytes, a line break included: the lines are recognised by their indented time stamps)
    word_lines = re.findall(r"(?m)^  \[(\d\d):(\d\d\.\d\d\d) --> (\d\d):(\d\d\.\d\d\d)\] ", out)
    assert len(word_lines) == len(want["words_bytes"]) > 0
    for line, w in zip(word_lines, want["words_bytes"]):
        assert abs(int(line[0]) * 60 + float(line[1]) - w[2]) < 1e-3 and abs(int(line[2]) * 60 + float(line[3]) - w[3]) < 1e-3
    assert len(re.findall(r"(?m)^\[\d\d:", out)) == len(want["segments"])
    plain = subprocess.run(args, capture_output=True, timeout=120).stdout.decode("utf-8", "replace")
    assert not re.search(r"(?m)^  \[", plain)
    bad = subprocess.run(args[:-1] + ["--word_timestamps"], capture_output=True, timeout=120)
    assert bad.returncode != 0  # the flag needs --timestamps
