"""GPU: decode confidence (DESIGN.md "Confidence") — the scored rules kernel and the no-speech kernel against
tests/score_reference.py on crafted rows and on the engine's own dumped rows, the scores of the greedy loop against the oracle
teacher-forced with the engine's ids, scored ids against unscored ids, the long-form loop under the silent-window rule, and the
CLI's two flags.

Bars. On the GPU's own rows the only error is the kernel's float32 arithmetic: 1e-4 + 1e-6 * max(|x[c]|, |logsumexp|) (one
float32 ulp at 324 is 3e-5). Against the oracle the rows themselves differ by the 16-bit storage error, measured at every step:
|logprob - ref| <= 2 * max|gpu_row - oracle_row| + 1e-4 (one error for the chosen logit, one for the normaliser). A step whose
decision differs from the Python rules' is left out only if that row's decision margin is below 1e-4, at most one per clip."""
import math
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import longform_reference as lfr
import score_reference as sr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

MAX_NEW = 48


def _clips():
    pcm = load_demo_pcm()
    n = len(pcm)
    return [pcm, pcm[: n * 2 // 3] * np.float32(0.7), pcm[n // 5:], np.concatenate([pcm[n // 3:], pcm[: n // 3]]) * np.float32(1.3),
            np.zeros(16000, dtype=np.float32)]


def _bar(xc, lse):
    m = max(abs(xc) if math.isfinite(xc) else 0.0, abs(lse) if math.isfinite(lse) else 0.0)
    return 1e-4 + 1e-6 * m


def _close(got, want, bar):
    got, want = float(got), float(want)
    if not math.isfinite(want) or not math.isfinite(got):
        return got == want or (math.isnan(got) and math.isnan(want))
    return abs(got - want) <= bar


class Model:
    def __init__(self, built_lib, tmp, model_type, seed, dtype, kind):
        import oracle

        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype, kind=kind)
        self.kind = kind
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=24)
        self.T, self.E, self.NS = self.e.timestamp_begin, self.e.eot, self.e.no_speech
        assert self.NS == int(self.case.cfg["no_speech"]) == self.T - 2
        self.clips = _clips()
        self.mels = [oracle.log_mel(c, self.case.dims["n_mels"])[0] for c in self.clips]
        self.orc = self.case.oracle_bf16
        self.prefix = self.orc.sot_seq("zh")[:3]
        self._kv, self._greedy, self._rows, self._gpu_rows = {}, {}, {}, {}

    def kv(self, k):
        if k not in self._kv:
            self._kv[k] = self.orc.encoder(self.mels[k])
        return self._kv[k]

    def oracle_ids(self, k):
        if k not in self._greedy:
            self._greedy[k] = tsr.greedy_ts(self.orc, *self.kv(k), self.prefix, max_new=MAX_NEW)[0]
        return self._greedy[k]

    def oracle_rows(self, k, ids):
        key = (k, tuple(ids))
        if key not in self._rows:
            self._rows[key] = sr.oracle_rows(self.orc, *self.kv(k), self.prefix, ids)
        return self._rows[key]

    def gpu_rows(self, k, ids, family):
        """The engine teacher-forced with `ids` on clip k -> (row of offset 0, rows of the decisions), through the GEMV family (one
        clip) or through the clip-block step (four slots holding the same clip, slot 0 read)."""
        key = (k, tuple(ids), family)
        if key not in self._gpu_rows:
            nb = 1 if family == "gemv" else 4
            self.e.encode_mel(np.stack([self.mels[k]] * nb))
            f = np.array([list(ids)] * nb, dtype=np.int32).reshape(nb, len(ids))
            logits, _, _, _, l0 = self.e.decode_forced_timestamp_scores(nb, f)
            self._gpu_rows[key] = (l0[0].copy(), logits[0].copy())
        return self._gpu_rows[key]


PARAMS = [("micro", 11, "BF16", "benign"), ("miniturbo", 21, "F16", "benign"), ("micro", 11, "BF16", "realistic")]


@pytest.fixture(scope="module", params=PARAMS, ids=["micro_bf16", "miniturbo_fp16", "micro_bf16_realistic"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("sc_" + request.param[0] + request.param[3]), *request.param)
    yield m
    m.e.close()


def test_scored_kernel_on_crafted_rows(model):
    """Item 6: chosen ids as crafted_cases expects, log-probabilities within the float32 bar of the Python reference; the no-speech
    kernel on the same rows."""
    nv, T, E = model.e.n_vocab, model.T, model.E
    cases = tsr.crafted_cases(nv)
    rng = np.random.default_rng(17)
    x = rng.uniform(-80.0, 80.0, nv).astype(np.float32); x[:2000] = 80.0; x[T:] = np.minimum(x[T:], 0.0)
    cases.append(("near_pm80_text", x, [T, 5], 0))
    x = rng.uniform(-80.0, 80.0, nv).astype(np.float32)
    cases.append(("near_pm80_rule5", x, [T, 5], tsr.decide(x, [T, 5], T, E)[0]))
    x = np.full(nv, -10.0, dtype=np.float32); x[7] = np.inf
    cases.append(("chosen_plus_inf", x, [T, 5], 7))
    x = (rng.standard_normal(nv) * 12.0 + 300.0).astype(np.float32); x[model.NS] = -20.0
    cases.append(("large_magnitudes", x, [T, 5, 9], tsr.decide(x, [T, 5, 9], T, E)[0]))
    rows = np.stack([c[1] for c in cases])
    got, lps = model.e.score_timestamp_rules(rows, [c[2] for c in cases])
    assert got == model.e.apply_timestamp_rules(rows, [c[2] for c in cases])  # the scored kernel decides as the unscored one
    worst = 0.0
    for (name, x, seq, want), g, lp in zip(cases, got, lps):
        assert g == want, (name, g, want)
        c, ref, info = sr.token_logprob(x, seq, T, E)
        assert _close(lp, ref, _bar(info["x_chosen"], info["lse_allowed"])), (name, float(lp), float(ref))
        if math.isfinite(float(ref)):
            worst = max(worst, abs(float(lp) - float(ref)))
    nsp = model.e.no_speech_logprob(rows)
    worst_ns = 0.0
    for (name, x, _, _), g in zip(cases, nsp):
        ref = sr.no_speech_logprob(x, model.NS)
        lse = tsr._lse(np.asarray(x, dtype=np.float64))
        assert _close(g, ref, _bar(float(x[model.NS]), lse)), (name, float(g), float(ref))
        if math.isfinite(float(ref)):
            worst_ns = max(worst_ns, abs(float(g) - float(ref)))
    print("crafted rows: max |logprob - ref| = %.3g, max |no_speech - ref| = %.3g" % (worst, worst_ns))


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_scored_kernel_on_real_rows(model, batch):
    """Item 7: teacher-forced with the oracle's ids; every step's log-probability against the reference on the GPU's OWN row,
    the no-speech value against the reference on the GPU's own offset-0 row."""
    T, E = model.T, model.E
    ids = model.oracle_ids(0)
    nc = len(model.clips)
    model.e.encode_mel(np.stack([model.mels[b % nc] for b in range(batch)]))
    f = np.array([ids] * batch, dtype=np.int32).reshape(batch, len(ids))
    logits, chosen, lp, nsp, l0 = model.e.decode_forced_timestamp_scores(batch, f)
    _, plain_chosen = model.e.decode_forced_timestamps(batch, f, want_logits=False)
    assert np.array_equal(chosen, plain_chosen)  # the scored step decides as the unscored one
    assert lp.shape == (batch, len(ids) + 1)
    worst = worst_ns = 0.0
    for b in range(batch if batch <= 3 else nc + 1):  # (16 slots: the five clips once, and one repeat)
        left_out = 0
        for i in range(len(ids) + 1):
            c, ref, info = sr.token_logprob(logits[b, i], ids[:i], T, E)
            if chosen[b, i] != c:
                assert info["margin"] < 1e-4, (b, i, int(chosen[b, i]), c, info)
                left_out += 1
                continue
            assert _close(lp[b, i], ref, _bar(info["x_chosen"], info["lse_allowed"])), (b, i, float(lp[b, i]), float(ref), info)
            worst = max(worst, abs(float(lp[b, i]) - float(ref)))
        assert left_out * 49 <= len(ids) + 1, (b, left_out)
        ref = sr.no_speech_logprob(l0[b], model.NS)
        assert _close(nsp[b], ref, _bar(float(l0[b, model.NS]), tsr._lse(l0[b].astype(np.float64)))), (b, float(nsp[b]), float(ref))
        worst_ns = max(worst_ns, abs(float(nsp[b]) - float(ref)))
    print("%s batch %d: max |logprob - ref| = %.3g, max |no_speech - ref| = %.3g on the GPU's own rows" % (model.kind, batch, worst, worst_ns))


@pytest.mark.parametrize("batch", [1, 2, 4, 16, 24])
def test_scores_against_the_oracle(model, batch):
    """Item 8: the oracle teacher-forced with the ENGINE's ids; bounds from the logit error measured at each step."""
    T, E = model.T, model.E
    nc = len(model.clips)
    got = model.e.run_timestamp_scores_batch([model.clips[b % nc] for b in range(batch)], max_new=MAX_NEW)
    family = "gemv" if batch <= 2 else "cblock"
    worst_bound = 0.0
    for b in (range(batch) if batch <= 4 else list(range(nc)) + [batch - 1]):
        k = b % nc
        g = got[b]
        ids, n = g["ids"], len(g["ids"])
        assert len(g["token_logprob"]) == n + 1
        r0, rows = model.oracle_rows(k, ids)
        l0, grows = model.gpu_rows(k, ids, family)
        left_out, bounds, ref_sum = 0, [], 0.0
        for i in range(n + 1):
            c, ref, info = sr.token_logprob(rows[i], ids[:i], T, E)
            decision = ids[i] if i < n else (E if g["ended_eot"] else None)
            differs = (decision != c) if decision is not None else (c == E)
            counts = i < n or g["ended_eot"]
            if differs:
                assert info["margin"] < 1e-4, (batch, b, i, decision, c, info)
                left_out += 1
                ref_sum += float(g["token_logprob"][i]) if counts else 0.0
                continue
            err = float(np.abs(grows[i] - rows[i]).max())
            bound = 2 * err + 1e-4
            assert _close(g["token_logprob"][i], ref, bound), (batch, b, i, float(g["token_logprob"][i]), float(ref), "logit err", err)
            if counts:
                bounds.append(bound)
                ref_sum += float(ref)
        assert left_out * 49 <= n + 1, (batch, b, left_out)
        err0 = float(np.abs(l0 - r0).max())
        assert _close(g["no_speech_logprob"], sr.no_speech_logprob(r0, model.NS), 2 * err0 + 1e-4), (batch, b, g["no_speech_logprob"], err0)
        if bounds and math.isfinite(ref_sum):
            assert abs(g["avg_logprob"] - ref_sum / (n + 1)) <= float(np.mean(bounds)) + 1e-6 * abs(ref_sum), (batch, b, g["avg_logprob"], ref_sum / (n + 1))
            worst_bound = max(worst_bound, max(bounds), 2 * err0 + 1e-4)
        if b == 0:
            print("%s batch %d clip 0: avg_logprob %.4f no_speech_logprob %.4f (n_ids %d, ended_eot %s)" %
                  (model.kind, batch, g["avg_logprob"], g["no_speech_logprob"], n, g["ended_eot"]))
    print("%s batch %d: largest bound %.3g" % (model.kind, batch, worst_bound))


def test_scored_ids_equal_unscored_ids(model):
    """Item 9: the same ids, ragged budgets included; plain and timestamp calls are unchanged by scored calls in between; the
    record of a clip cut by its budget and of one that is not."""
    clips = model.clips
    budgets = [5, 0, 17, 9, 3]
    plain_before = model.e.run_tokens_batch(clips[:4], max_new=MAX_NEW)
    one_before = model.e.run_tokens(clips[0], max_new=MAX_NEW)
    ts_before = model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW)
    rag_before = model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW, max_new_clip=budgets)
    full = model.e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
    rag = model.e.run_timestamp_scores_batch(clips, max_new=MAX_NEW, max_new_clip=budgets)
    one = model.e.run_timestamp_scores_batch(clips[:1], max_new=MAX_NEW)
    assert [g["ids"] for g in full] == ts_before
    assert [g["ids"] for g in rag] == rag_before
    assert one[0]["ids"] == model.e.run_timestamp_tokens_batch(clips[:1], max_new=MAX_NEW)[0]
    assert model.e.run_tokens_batch(clips[:4], max_new=MAX_NEW) == plain_before
    assert model.e.run_tokens(clips[0], max_new=MAX_NEW) == one_before
    assert model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW) == ts_before
    assert model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW, max_new_clip=budgets) == rag_before
    cut = 0
    for f, r, m in zip(full, rag, budgets):
        for g in (f, r):
            n = len(g["ids"])
            assert len(g["token_logprob"]) == n + 1 and np.all(g["token_logprob"] <= 0.0)
            want = sr.avg_logprob(g["token_logprob"], n, g["ended_eot"])
            assert _close(g["avg_logprob"], want, 1e-6 * max(1.0, abs(float(want)))), (g["avg_logprob"], want)
            if n < (m if g is r and m > 0 else MAX_NEW):
                assert g["ended_eot"]  # stopped before its budget: only eot does that
        if m > 0 and len(f["ids"]) > m:  # the budget cuts this clip: the same decisions up to the cut, the dropped id's value last
            cut += 1
            assert len(r["ids"]) == m
            for a, c in zip(r["token_logprob"], f["token_logprob"][: m + 1]):
                assert _close(a, c, _bar(float(c), 0.0)), (a, c)
            assert not r["ended_eot"]  # (ids never hold eot: the decision dropped at the cut was an id)
            assert _close(r["no_speech_logprob"], f["no_speech_logprob"], _bar(f["no_speech_logprob"], 0.0))
    assert cut >= 1
    # one clip alone, cut and not cut: ended_eot and the n + 1 values against the teacher-forced scored step
    for m in (7, MAX_NEW):
        g = model.e.run_timestamp_scores_batch(clips[:1], max_new=m)[0]
        n = len(g["ids"])
        model.e.encode_mel(model.mels[0])
        _, chosen, lp, nsp, _ = model.e.decode_forced_timestamp_scores(1, np.array([g["ids"]], dtype=np.int32).reshape(1, n), want_logits=False)
        assert chosen[0, :n].tolist() == g["ids"]
        assert g["ended_eot"] == (int(chosen[0, n]) == model.E)
        assert all(_close(a, c, _bar(float(c), 0.0)) for a, c in zip(lp[0], g["token_logprob"])), (lp[0], g["token_logprob"])
        assert _close(nsp[0], g["no_speech_logprob"], _bar(g["no_speech_logprob"], 0.0))


def test_ended_eot_on_a_model_that_stops(built_lib, oracle_mod, tmp_path):
    """Item 9, the other half: seeded weights never emit eot, so ended_eot is checked on the eot-shaped model of tests/eot_case.py in
    timestamp mode — clips that end on eot beside clips the budget cuts. The eot decision's log-probability counts in the
    average, a dropped id's does not."""
    from eot_case import EotCase, eot_clips

    budget = 40
    ec = EotCase("micro", 31, "BF16", budget=budget)
    e = built_lib.Whisper("micro", ec.write(tmp_path), "zh", device=0, max_batch=4)
    try:
        clips = eot_clips(4)
        got = e.run_timestamp_scores_batch(clips, max_new=budget)
        assert [g["ids"] for g in got] == e.run_timestamp_tokens_batch(clips, max_new=budget)
        assert {g["ended_eot"] for g in got} == {True, False}, [(len(g["ids"]), g["ended_eot"]) for g in got]
        for k, g in enumerate(got):
            n = len(g["ids"])
            assert len(g["token_logprob"]) == n + 1
            if n < budget:
                assert g["ended_eot"]  # stopped before the budget: only eot does that (at the budget the dropped decision may be eot too)
            want = sr.avg_logprob(g["token_logprob"], n, g["ended_eot"])
            assert _close(g["avg_logprob"], want, 1e-6 * max(1.0, abs(float(want))))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- long-form
class LongModel:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=3)
        self.T, self.E = self.e.timestamp_begin, self.e.eot
        demo = load_demo_pcm()
        self.files = [lfr.make_file(demo, k) for k in range(1, 6)]


@pytest.fixture(scope="module", params=PARAMS[:2], ids=["micro_bf16", "miniturbo_fp16"])
def long_model(request, built_lib, oracle_mod, tmp_path_factory):
    m = LongModel(built_lib, tmp_path_factory.mktemp("scl_" + request.param[0]), *request.param[:3])
    yield m
    m.e.close()


# thresholds a clear distance from every window's values on these fixtures (the oracle: avg_logprob -8.1 / -8.3,
# no_speech_logprob -11.0 / -10.7, i.e. a probability of 2e-5): ln(1e-9) = -20.7 and ln(0.6) = -0.5 are 9.7 and 10.2 away from
# the no-speech values, -1.0 is 7 away from the averages; the largest bound of test_scores_against_the_oracle is below 0.05
SKIP_ALL = dict(no_speech_threshold=1e-9, logprob_threshold=-1.0)
SKIP_NONE = dict(no_speech_threshold=0.6, logprob_threshold=-1.0)


def test_long_form_scores_and_silent_windows(long_model, monkeypatch):
    """Item 10. Files 1-5 in three slots (files wait, slots compact)."""
    m = long_model
    plain = m.e.run_long_windows(m.files, max_new=MAX_NEW)
    scored = m.e.run_long_windows(m.files, max_new=MAX_NEW, scores=True)
    assert [[w[:6] for w in f] for f in scored] == plain  # without thresholds: today's loop, window for window
    every = [w for f in scored for w in f]
    assert len(every) >= 9 and not any(w[8] for w in every)
    for w in every:  # the thresholds below do stand clear of every window
        assert math.log(1e-9) + 5 < w[6] < math.log(0.6) - 5 and w[7] < -1.0 - 3, w[6:]
    # the scores of a window are those of the same window fed as a clip: the first window of a file is the clip entry point's
    # input (test_gpu_longform.py: check 2), and pass 0 holds files 1-3 in the three slots as this batch does
    as_clips = m.e.run_timestamp_scores_batch(m.files[:3], max_new=MAX_NEW)
    for k in range(3):
        w = scored[k][0]
        assert w[0] == 0 and w[4] == 0 and w[5] == k and w[3] == as_clips[k]["ids"]
        assert _close(w[6], as_clips[k]["no_speech_logprob"], _bar(w[6], 0.0)) and _close(w[7], as_clips[k]["avg_logprob"], _bar(w[7], 0.0)), (k, w[6:], as_clips[k])
    none = m.e.run_long_windows(m.files, max_new=MAX_NEW, **SKIP_NONE)
    assert [[w[:6] for w in f] for f in none] == plain and not any(w[8] for f in none for w in f)
    assert [[w[6:8] for w in f] for f in none] == [[w[6:8] for w in f] for f in scored]
    skipped = m.e.run_long_windows(m.files, max_new=MAX_NEW, **SKIP_ALL)
    for k, f in enumerate(skipped):
        want = sr.loop_scored(len(m.files[k]), lambda s, w: [], lambda s, w: (0.0, -9.0), m.T, m.E, 0.6, -1.0)
        assert [(w[0], w[1], w[2]) for w in f] == [(w[0], w[1], w[2]) for w in want], k  # every advance is window_frames
        assert all(w[8] and w[2] == w[1] for w in f)
    assert [len(f) for f in skipped] == [1, 1, 2, 3, 4]
    # passes: files 1-3 start in pass 0, files 4 and 5 take the places of files 1 and 2 in pass 1; file 5's fourth window is pass 4
    assert [[w[4] for w in f] for f in skipped] == [[0], [0], [0, 1], [1, 2, 3], [1, 2, 3, 4]]
    assert m.e.run_long_text(m.files[2], **SKIP_ALL) == ""
    assert m.e.run_long_text(m.files[2], **SKIP_NONE) == m.e.run_long_text(m.files[2])
    assert m.e.run_long_scored(m.files[2], max_new=MAX_NEW, **SKIP_ALL) == []
    segs, segs_scored = m.e.run_long(m.files[2], max_new=MAX_NEW), m.e.run_long_scored(m.files[2], max_new=MAX_NEW, **SKIP_NONE)
    assert [s[:3] for s in segs_scored] == segs and len(segs) >= 1
    assert all(s[3] < -4.0 and 0.0 < s[4] < 1e-3 for s in segs_scored)
    # two engines on one device: the files are split 3 + 2, every file's windows are the single engine's
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    two = m.lib.Whisper(m.case.model_type, m.case.root, "zh", devices=[0, 0], max_batch=3)
    try:
        log2 = two.run_long_windows(m.files, max_new=MAX_NEW, **SKIP_NONE)
        skip2 = two.run_long_windows(m.files, max_new=MAX_NEW, **SKIP_ALL)
    finally:
        two.close()
    assert [[w[:4] for w in f] for f in log2] == [[w[:4] for w in f] for f in none]
    # (files 4 and 5 decode in two slots there, through the GEMV family: their rows differ by the 16-bit storage error — bfloat16
    # keeps 8 bits, logits of magnitude ~10: 0.04)
    for f2, f1 in zip(log2, none):
        for w2, w1 in zip(f2, f1):
            assert abs(w2[6] - w1[6]) < 0.05 and abs(w2[7] - w1[7]) < 0.05 and not w2[8]
    assert [[(w[0], w[1], w[2], w[8]) for w in f] for f in skip2] == [[(w[0], w[1], w[2], w[8]) for w in f] for f in skipped]


def test_cli_thresholds(long_model, tmp_path):
    """Item 11: --long on a 45 s file with and without the two flags."""
    m = long_model
    cli = os.path.join(os.path.dirname(m.lib.LIB_PATH), "whisper_cli")
    wav = str(tmp_path / "f45.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(m.files[2], -1.0, 1.0) * 32767.0).astype(np.int16).tobytes())
    args = [cli, "-w", wav, "-t", m.case.model_type, "-p", m.case.root, "--language", "zh", "--long"]
    run = lambda extra: subprocess.run(args + extra, capture_output=True, timeout=300)
    base, none, every = run([]), run(["--no_speech_threshold", "0.6", "--logprob_threshold=-1.0"]), run(["--no_speech_threshold", "1e-9", "--logprob_threshold", "-1.0"])
    assert base.returncode == 0 and none.returncode == 0 and every.returncode == 0, (base.stderr, none.stderr, every.stderr)
    hdr = re.compile(r"(?m)^\[\d+:\d\d\.\d{3} --> \d+:\d\d\.\d{3}\] ")
    tail = re.compile(r" \(avg_logprob -?\d+\.\d{4}, no_speech [0-9.e+-]+\)\n$")

    def parts(r):
        """(lines before Result:, the Result: text, the segment blocks — a segment's text may hold line breaks —, what follows RTF:)"""
        out = r.stdout.decode("utf-8", "replace")
        head, rest = out.split("\nResult: ", 1)
        rest, rtf = rest[: rest.rindex("RTF: ")], rest[rest.rindex("RTF: "):]
        heads = list(hdr.finditer(rest))
        text = rest[: heads[0].start()] if heads else rest
        blocks = [rest[h.start(): heads[j + 1].start() if j + 1 < len(heads) else len(rest)] for j, h in enumerate(heads)]
        return [l for l in head.splitlines() if not l.startswith("Init whisper success")], text, blocks, rtf

    bh, bt, bb, _ = parts(base)
    nh, nt, nb, _ = parts(none)
    ah, at, ab, _ = parts(every)
    assert bh == nh == ah and bt == nt and len(bb) == len(nb) >= 1
    for lb, ln in zip(bb, nb):
        assert tail.search(ln) and not tail.search(lb) and tail.sub("\n", ln) == lb, (lb, ln)
    assert at == "\n" and ab == []  # every window skipped: an empty text, no segment line
    bad = subprocess.run(args[:-1] + ["--no_speech_threshold", "0.6"], capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"need --long" in bad.stderr
