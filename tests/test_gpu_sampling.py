"""GPU: temperature fallback (DESIGN.md "Temperature fallback") — the sampled rules kernel against tests/sample_reference.py on
crafted and random rows, temperature 0 against scored mode, mixed batches, determinism of (seed, stream, history length), the sampled
greedy loop against the teacher-forced sampled step and against the reference on the GPU's own rows, the long-form loop under
fallback against the loop reference, and the CLI's flags.

Bars. The ids must equal the reference's except where the reference's two best Gumbel keys are closer than the float32 bound
derived in sample_reference.py (a near tie): at most 1 % of a test's decisions, and the reference's own near-tie count on the
chosen inputs must be within that share too. Log-probabilities: the bar of test_gpu_scores.py, 1e-4 + 1e-6 * max(|x[c]|, |lse|)."""
import math
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import longform_reference as lfr
import sample_reference as smp
import score_reference as sr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

MAX_NEW = 16
TEMPS = (0.2, 0.6, 1.0)
SEED = 0x5EED0123456789


def _bar(xc, lse):
    m = max(abs(xc) if math.isfinite(xc) else 0.0, abs(lse) if math.isfinite(lse) else 0.0)
    return 1e-4 + 1e-6 * m


def _close(got, want, bar):
    got, want = float(got), float(want)
    if not math.isfinite(want) or not math.isfinite(got):
        return got == want or (math.isnan(got) and math.isnan(want))
    return abs(got - want) <= bar


def _clips():
    pcm = load_demo_pcm()
    n = len(pcm)
    return [pcm, pcm[: n * 2 // 3] * np.float32(0.7), pcm[n // 5:], np.concatenate([pcm[n // 3:], pcm[: n // 3]]) * np.float32(1.3),
            np.zeros(16000, dtype=np.float32)]


class Model:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=24)
        self.T, self.E, self.nv = self.e.timestamp_begin, self.e.eot, self.e.n_vocab
        self.clips = _clips()
        self._rows = None

    def rows(self):
        """24 (name, row, history): every crafted case plus random rows of std 1, 3 and 10 under histories of several lengths and
        rule states. Built once, never changed."""
        if self._rows is None:
            T = self.T
            out = [(name, x, seq) for name, x, seq, _ in tsr.crafted_cases(self.nv)]
            rng = np.random.default_rng(41)
            hists = [[], [T, 5], [T, 5, 9, 11, 13], [T, 5, T + 30, T + 30], [T, 5, T + 30, T + 30, 8, T + 60], [T + 3, 7, 7, 7, 7, 7, 7, 7, 7]]
            for k in range(24 - len(out)):
                std = (1.0, 3.0, 10.0)[k % 3]
                out.append(("random_std%g_%d" % (std, k), (rng.standard_normal(self.nv) * std).astype(np.float32), hists[k % len(hists)]))
            x = np.full(self.nv, -10.0, dtype=np.float32); x[900] = np.inf; x[40] = np.inf
            out[-1] = ("two_plus_inf_lowest_id", x, [T, 5])
            self._rows = out
        return self._rows


PARAMS = [("micro", 11, "BF16"), ("miniturbo", 21, "F16")]


@pytest.fixture(scope="module", params=PARAMS, ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("smp_" + request.param[0]), *request.param)
    yield m
    m.e.close()


def _check_decisions(cases, got, lps, T, E, what):
    """cases: (name, row, history, t, stream, seed) per decision. Ids equal the reference's outside near ties, log-probabilities
    within the bar; the share left out and the reference's own near-tie share are asserted. Returns the number left out."""
    left_out = near = 0
    worst = 0.0
    for (name, x, seq, t, stream, seed), g, lp in zip(cases, got, lps):
        c, ref, info = smp.sample(x, seq, T, E, t, stream, seed)
        near += info["near_tie"]
        if g != c:
            assert info["near_tie"] and g == info["runner_up"], (what, name, t, stream, int(g), c, info)
            left_out += 1
            continue
        assert _close(lp, ref, _bar(info["x_chosen"], info["lse_allowed"])), (what, name, t, float(lp), float(ref))
        if math.isfinite(float(ref)):
            worst = max(worst, abs(float(lp) - float(ref)))
    n = len(cases)
    print("%s: %d decisions, %d near ties in the reference, %d left out, max |logprob - ref| = %.3g" % (what, n, near, left_out, worst))
    assert left_out * 100 <= n and near * 100 <= n, (what, left_out, near, n)
    return left_out


def test_sampled_kernel_on_crafted_and_random_rows(model):
    T, E = model.T, model.E
    rows = model.rows()
    logits = np.stack([r[1] for r in rows])
    hists = [r[2] for r in rows]
    cases, got, lps = [], [], []
    for j, t in enumerate(TEMPS):
        for rep in range(2):
            streams = [(b * 7 + rep) | ((j * 5 + b % 3) << 32) for b in range(len(rows))]
            g, lp = model.e.sample_timestamp_rules(logits, hists, t, streams, SEED + rep)
            cases += [(name, x, seq, t, s, SEED + rep) for (name, x, seq), s in zip(rows, streams)]
            got += g
            lps += list(lp)
    _check_decisions(cases, got, lps, T, E, "kernel alone")
    # the draws are draws: on the random rows the ids differ from the greedy ones somewhere, and between the temperatures
    greedy = model.e.score_timestamp_rules(logits, hists)[0]
    n = len(rows)
    assert any(got[k * n:(k + 1) * n] != greedy for k in range(6))
    # exact ties are never left out: two +inf logits, the lowest id at every temperature
    assert all(got[k * n + n - 1] == 40 for k in range(6))


def test_temperature_zero_is_scored_mode(model):
    rows = model.rows()
    logits = np.stack([r[1] for r in rows])
    hists = [r[2] for r in rows]
    want, want_lp = model.e.score_timestamp_rules(logits, hists)
    got, lp = model.e.sample_timestamp_rules(logits, hists, 0.0, list(range(len(rows))), SEED)
    assert got == want
    for (name, x, seq), a, b in zip(rows, lp, want_lp):
        _, _, info = sr.token_logprob(x, seq, model.T, model.E)
        assert _close(a, b, _bar(info["x_chosen"], info["lse_allowed"])), (name, float(a), float(b))
    print("temperature 0: log-probabilities bit-equal to scored mode: %s" % np.array_equal(lp, want_lp, equal_nan=True))
    # a NaN or negative temperature is refused on the host
    for bad in (-0.5, float("nan"), float("inf"), 1e-30):
        with pytest.raises(RuntimeError, match="temperature"):
            model.e.sample_timestamp_rules(logits[:1], hists[:1], bad, 0, SEED)


def test_mixed_batch_and_determinism(model):
    rows = model.rows()[15:23]  # the random rows
    logits = np.stack([r[1] for r in rows])
    hists = [r[2] for r in rows]
    B = len(rows)
    temps = [0.0, 0.6, 0.0, 1.0, 0.2, 0.0, 1.0, 0.6]
    streams = [100 + b for b in range(B)]
    got, lp = model.e.sample_timestamp_rules(logits, hists, temps, streams, SEED)
    # each clip gets what it gets alone
    for b in range(B):
        g1, lp1 = model.e.sample_timestamp_rules(logits[b:b + 1], hists[b:b + 1], temps[b], streams[b], SEED)
        assert g1[0] == got[b] and (lp1[0] == lp[b] or (math.isnan(lp1[0]) and math.isnan(lp[b]))), (b, g1, got[b], lp1, lp[b])
    scored = model.e.score_timestamp_rules(logits, hists)[0]
    assert all(got[b] == scored[b] for b in range(B) if temps[b] == 0.0)
    # the same (seed, stream, n) at another batch position and in another batch
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    got_p, lp_p = model.e.sample_timestamp_rules(logits[perm], [hists[i] for i in perm], [temps[i] for i in perm], [streams[i] for i in perm], SEED)
    assert got_p == [got[i] for i in perm] and np.array_equal(lp_p, lp[perm])
    wide = np.concatenate([logits, logits, logits])
    got_w, _ = model.e.sample_timestamp_rules(wide, hists * 3, temps * 3, streams * 3, SEED)
    assert got_w == got * 3
    # another seed or another stream changes some of the decisions (the t = 0 clips stay)
    hot = [1.0] * B
    base = model.e.sample_timestamp_rules(logits, hists, hot, streams, SEED)[0]
    other_seed = model.e.sample_timestamp_rules(logits, hists, hot, streams, SEED + 1)[0]
    other_stream = model.e.sample_timestamp_rules(logits, hists, hot, [s + (1 << 32) for s in streams], SEED)[0]
    assert base != other_seed and base != other_stream
    # the history length is part of the counter: the same row one id later draws other noise
    longer = [h + [9] if h and h[-1] < model.T else h + [model.T + 1400] for h in hists]
    assert model.e.sample_timestamp_rules(logits, longer, hot, streams, SEED)[0] != base


@pytest.mark.parametrize("batch", [1, 4, 24])
def test_sampled_loop_against_the_kernel(model, batch):
    """Batches 1, 4 and 24: the GEMV family, the clip-block step and the multi-branch step. The ids the loop returns, teacher-forced
    through the sampled step with the same seed and streams on the same encoder output, come out again with their log-probabilities;
    the reference sampler on the GPU's own dumped rows draws the same ids."""
    T, E = model.T, model.E
    nc = len(model.clips)
    temps = [(0.6, 1.0, 0.0, 0.2)[b % 4] for b in range(batch)]
    streams = [(b * 3 + 1) | (b << 32) for b in range(batch)]
    got = model.e.run_timestamp_sampled_batch([model.clips[b % nc] for b in range(batch)], temps, streams, SEED, max_new=MAX_NEW)
    n = [len(g["ids"]) for g in got]
    assert max(n) == MAX_NEW  # (seeded weights do not emit eot early; the budget ends the clips)
    f = np.zeros((batch, MAX_NEW), dtype=np.int32)
    for b, g in enumerate(got):
        f[b, : n[b]] = g["ids"]
    # the slots still hold this call's cross K/V: the forced step runs on the same encoder output
    logits, chosen, lp, nsp, _ = model.e.decode_forced_timestamp_sampled(batch, f, temps, streams, SEED)
    cases, gids, glps = [], [], []
    for b in range(batch):
        g = got[b]
        assert chosen[b, : n[b]].tolist() == g["ids"], (batch, b)
        assert g["ended_eot"] == (int(chosen[b, n[b]]) == E)
        for i in range(n[b] + 1):
            assert _close(lp[b, i], g["token_logprob"][i], _bar(float(g["token_logprob"][i]), 0.0)), (batch, b, i, lp[b, i], g["token_logprob"][i])
        assert _close(nsp[b], g["no_speech_logprob"], _bar(g["no_speech_logprob"], 0.0))
        want = sr.avg_logprob(g["token_logprob"], n[b], g["ended_eot"])
        assert _close(g["avg_logprob"], want, 1e-6 * max(1.0, abs(float(want))))
        for i in range(n[b] + 1):  # every clip, every step
            cases.append(("clip%d_step%d" % (b, i), logits[b, i], g["ids"][:i], temps[b], streams[b], SEED))
            gids.append(int(chosen[b, i]))
            glps.append(lp[b, i])
    _check_decisions(cases, gids, glps, T, E, "loop, batch %d" % batch)
    # the clips at temperature 0 are scored mode's
    scored = model.e.run_timestamp_scores_batch([model.clips[b % nc] for b in range(batch)], max_new=MAX_NEW)
    assert all(got[b]["ids"] == scored[b]["ids"] for b in range(batch) if temps[b] == 0.0)
    assert any(got[b]["ids"] != scored[b]["ids"] for b in range(batch) if temps[b] > 0.0)


# ---------------------------------------------------------------------------------------------------- long-form
LONG_TEMPS = [0.0, 0.4, 1.0]


class LongModel:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=2)
        self.T, self.E = self.e.timestamp_begin, self.e.eot
        demo = load_demo_pcm()
        self.files = [lfr.make_file(demo, 1), lfr.make_file(demo, 3)]  # 12 s and 45 s


@pytest.fixture(scope="module", params=PARAMS, ids=["micro_bf16", "miniturbo_fp16"])
def long_model(request, built_lib, oracle_mod, tmp_path_factory):
    m = LongModel(built_lib, tmp_path_factory.mktemp("smpl_" + request.param[0]), *request.param)
    yield m
    m.e.close()


def _follows_the_loop_reference(m, n_samples, log, cr_thr, lp_thr, ns_thr):
    """One file's log against sample_reference.loop_fallback fed with the log's own ids and scores."""
    by_key = {(w[0], w[9]): w for w in log}
    assert len(by_key) == len(log)

    def decode(seek, wf, a, t):
        w = by_key[(seek, a)]
        return w[3], w[6], w[7], smp.window_text(w[3], m.E, m.e.detokenize)

    nan = lambda v: math.nan if v is None else v
    want = smp.loop_fallback(n_samples, decode, m.T, m.E, LONG_TEMPS, nan(cr_thr), nan(lp_thr), nan(ns_thr))
    assert len(want) == len(log)
    for w, r in zip(log, want):
        seek, wf, adv, ids, a, t, cr, kept, skipped = r
        assert (w[0], w[1], w[2], w[3], w[9], w[12], w[8]) == (seek, wf, adv, ids, a, kept, skipped), (w, r)
        assert w[10] == t and w[11] == cr, (w[10:12], t, cr)


def test_long_form_fallback(long_model, monkeypatch):
    """Ids do not depend on the audio on synthetic weights, so the thresholds steer: the fixtures' greedy avg_logprob is about -8."""
    m = long_model
    scored = m.e.run_long_windows(m.files, max_new=MAX_NEW, scores=True)
    assert all(-30.0 < w[7] < -1.5 for f in scored for w in f)
    # logprob_threshold above every average: every window goes through all attempts, the last is kept
    every = m.e.run_long_windows(m.files, max_new=MAX_NEW, logprob_threshold=-1.0, temperatures=LONG_TEMPS, seed=SEED)
    for k, f in enumerate(every):
        assert [w[9] for w in f] == [0, 1, 2] * (len(f) // 3) and [w[12] for w in f] == [False, False, True] * (len(f) // 3), k
        assert [w[10] for w in f] == [float(np.float32(t)) for t in LONG_TEMPS] * (len(f) // 3)
        assert all(w[2] == 0 for w in f if not w[12]) and all(w[2] > 0 for w in f if w[12])
        _follows_the_loop_reference(m, len(m.files[k]), f, None, -1.0, None)
        # the first attempts are greedy: the scored loop's first window; the sampled ones differ from it
        assert f[0][3] == scored[k][0][3] and f[2][3] != f[0][3]
    # logprob_threshold below every average: one attempt per window, the scored loop's log
    once = m.e.run_long_windows(m.files, max_new=MAX_NEW, logprob_threshold=-30.0, temperatures=LONG_TEMPS, seed=SEED)
    none = m.e.run_long_windows(m.files, max_new=MAX_NEW, logprob_threshold=-30.0)
    assert [[w[:9] for w in f] for f in once] == none
    assert all(w[9] == 0 and w[10] == 0.0 and w[12] for f in once for w in f)
    # compression_ratio_threshold 0: the ratio branch alone (any text at all compresses by more than 0)
    ratio = m.e.run_long_windows(m.files, max_new=MAX_NEW, compression_ratio_threshold=0.0, temperatures=LONG_TEMPS, seed=SEED)
    for k, f in enumerate(ratio):
        assert all(w[11] > 0.0 for w in f) and [w[12] for w in f] == [False, False, True] * (len(f) // 3)
        _follows_the_loop_reference(m, len(m.files[k]), f, 0.0, None, None)
        assert [w[:4] + w[9:] for w in f] == [w[:4] + w[9:] for w in every[k]]  # the same streams: the same draws as above
    # each file alone: the windows it gets beside the other. The stream is numbered by (seek, file id, attempt), the id defaulting to
    # the index in the call: file 0 alone as it is, file 1 alone under its id 1 — and under id 0 it draws other noise
    key = lambda f: [w[:4] + w[9:] for w in f]
    fb = dict(max_new=MAX_NEW, logprob_threshold=-1.0, temperatures=LONG_TEMPS, seed=SEED)
    alone0 = m.e.run_long_windows(m.files[:1], **fb)[0]
    alone1 = m.e.run_long_windows(m.files[1:], file_ids=[1], **fb)[0]
    assert key(alone0) == key(every[0]) and key(alone1) == key(every[1])
    assert key(m.e.run_long_windows(m.files[1:], **fb)[0]) != key(every[1])
    # ids travel with the files: the two in the other order, and under ids of the caller's choice
    swapped = m.e.run_long_windows(m.files[::-1], file_ids=[1, 0], **fb)
    assert key(swapped[0]) == key(every[1]) and key(swapped[1]) == key(every[0])
    named = m.e.run_long_windows(m.files, file_ids=[700, 3], **fb)
    assert key(named[0]) == key(m.e.run_long_windows(m.files[:1], file_ids=[700], **fb)[0]) != key(every[0])
    with pytest.raises(RuntimeError):
        m.e.run_long_windows(m.files[:1], file_ids=[-1], **fb)
    # another seed: other draws
    other = m.e.run_long_windows(m.files[:1], max_new=MAX_NEW, logprob_threshold=-1.0, temperatures=LONG_TEMPS, seed=SEED + 1)[0]
    assert other[0][3] == alone0[0][3] and [w[3] for w in other] != [w[3] for w in alone0]
    # text and segments: the kept attempts only
    segs = m.e.run_long_scored(m.files[0], max_new=MAX_NEW, logprob_threshold=-1.0, temperatures=LONG_TEMPS, seed=SEED)
    kept = [w for w in alone0 if w[12] and not w[8]]
    want = [m.e.transcript(w[3][tb:te]) for w in kept for _, _, tb, te in m.lib.split_window(w[3], m.T, m.E, w[1])[0]]
    assert [s[2] for s in segs] == want and len(segs) >= 1
    # two engines on one device: the files are split 1 + 1, every file's windows are the single engine's
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    two = m.lib.Whisper(m.case.model_type, m.case.root, "zh", devices=[0, 0], max_batch=2)
    try:
        log2 = two.run_long_windows(m.files, max_new=MAX_NEW, logprob_threshold=-1.0, temperatures=LONG_TEMPS, seed=SEED)
        swap2 = two.run_long_windows(m.files[::-1], file_ids=[1, 0], **fb)
    finally:
        two.close()
    assert [[w[:4] + w[9:] for w in f] for f in log2] == [[w[:4] + w[9:] for w in f] for f in every]
    assert key(swap2[0]) == key(every[1]) and key(swap2[1]) == key(every[0])


def test_cli_fallback_flags(long_model, tmp_path):
    """--long with the fallback flags prints what the ABI returns for the same file."""
    m = long_model
    cli = os.path.join(os.path.dirname(m.lib.LIB_PATH), "whisper_cli")
    wav = str(tmp_path / "f12.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(m.files[0], -1.0, 1.0) * 32767.0).astype(np.int16).tobytes())
    args = [cli, "-w", wav, "-t", m.case.model_type, "-p", m.case.root, "--language", "zh"]
    flags = ["--compression_ratio_threshold", "0", "--temperature_increment", "0.5", "--seed", "77"]
    r = subprocess.run(args + ["--long"] + flags, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.decode("utf-8", "replace")
    text = out.split("\nResult: ", 1)[1]
    want = m.e.run_long_text(wav, compression_ratio_threshold=0.0, temperatures=[0.0, 0.5, 1.0], seed=77)
    assert text.startswith(want + "\n") and want
    assert want != m.e.run_long_text(wav)  # the kept attempt is the one at temperature 1.0
    assert re.search(r"temperature 1\.0, compression_ratio \d+\.\d{3}\)\n", text)
    bad = subprocess.run(args + flags, capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"need" in bad.stderr and b"--long" in bad.stderr
