"""GPU: the timestamp rules inside the one-clip persistent launch — one clip in timestamp or scored mode takes the
launch's rules instantiation. Teacher-forced decisions and scores on the launch's own dumped rows against tests/ts_reference.py
and tests/score_reference.py, greedy ids against the oracle loop and against a handle with the route switched off
(the default; AX_WHISPER_PERSIST_TS=1 switches it on), the stop conditions, token suppression, the requests that stay on the launch-per-phase path, the give-up
fallback, and the long-form seek loop. Every test reads `persistent_ts_launches`: the counter moves by the launches the test expects.

Bars are those of test_gpu_timestamps.py and test_gpu_scores.py: a decision may differ from the Python rules only where the row's
margin is below 1e-4, at most one per clip; log-probabilities on the launch's own rows within 1e-4 + 1e-6 * max(|x[c]|, |lse|); a
greedy divergence only as a measured tie, margin < 2 * logit error + 1e-4."""
import math
import os

import numpy as np
import pytest

import score_reference as sr
import suppress_reference as supr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

MAX_NEW = 48


def _clips():
    pcm = load_demo_pcm()
    n = len(pcm)
    return [pcm, pcm[: n * 2 // 3] * np.float32(0.7), pcm[n // 5:], np.concatenate([pcm[n // 3:], pcm[: n // 3]]) * np.float32(1.3)]


def _bar(xc, lse):
    m = max(abs(xc) if math.isfinite(xc) else 0.0, abs(lse) if math.isfinite(lse) else 0.0)
    return 1e-4 + 1e-6 * m


def _close(got, want, bar):
    got, want = float(got), float(want)
    if not math.isfinite(want) or not math.isfinite(got):
        return got == want or (math.isnan(got) and math.isnan(want))
    return abs(got - want) <= bar


class Model:
    """A handle with the route on (AX_WHISPER_PERSIST_TS=1), one with it off (the default), the clips, and the oracle's timestamp-mode loop."""

    def __init__(self, built_lib, monkeypatch_env, tmp, model_type, seed, dtype, env=()):
        import oracle

        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        for k, v in env:
            monkeypatch_env.setenv(k, v)
        monkeypatch_env.setenv("AX_WHISPER_PERSIST_TS", "1")
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=4)
        monkeypatch_env.setenv("AX_WHISPER_PERSIST_TS", "0")
        self.off = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=4)
        monkeypatch_env.delenv("AX_WHISPER_PERSIST_TS")
        for k, _ in env:
            monkeypatch_env.delenv(k)
        self.T, self.E, self.NS = self.e.timestamp_begin, self.e.eot, self.e.no_speech
        self.clips = _clips()
        self.mels = [oracle.log_mel(c, self.case.dims["n_mels"])[0] for c in self.clips]
        self.orc = self.case.oracle_bf16
        self.prefix = self.orc.sot_seq("zh")[:3]
        self._orc = {}

    def count(self):
        return self.e.persistent_ts_launches

    def oracle_run(self, k):
        if k not in self._orc:
            ck, cv = self.orc.encoder(self.mels[k])
            self._orc[k] = tsr.greedy_ts(self.orc, ck, cv, self.prefix, max_new=MAX_NEW, want_logits=True)
        return self._orc[k]

    def close(self):
        self.e.close()
        self.off.close()


# micro: d 128, resident rows; miniturbo: 51866 ids, fp16; w1280: no resident rows, the wide-row loop; then the unfolded launch
# (AX_WHISPER_QFOLD=0) and the launch without resident rows (AX_WHISPER_VOCAB_RESIDENT=0)
PARAMS = [("micro", 11, "BF16", ()), ("miniturbo", 21, "F16", ()), ("w1280", 23, "BF16", ()),
          ("micro", 11, "BF16", (("AX_WHISPER_QFOLD", "0"),)), ("miniturbo", 21, "F16", (("AX_WHISPER_VOCAB_RESIDENT", "0"),))]
IDS = ["micro_bf16", "miniturbo_fp16", "w1280", "micro_unfolded", "miniturbo_streamed"]


@pytest.fixture(scope="module", params=PARAMS, ids=IDS)
def model(request, built_lib, oracle_mod, tmp_path_factory):
    mp = pytest.MonkeyPatch()
    m = Model(built_lib, mp, tmp_path_factory.mktemp("pts_" + request.param[0]), *request.param[:3], env=request.param[3])
    mp.undo()
    assert m.e.get_config_int("persistent_ts") == 1 and m.off.get_config_int("persistent_ts") == 0
    if request.param[3] == (("AX_WHISPER_QFOLD", "0"),):
        assert m.e.get_config_int("persistent_qfold") == 0
    if request.param[3] == (("AX_WHISPER_VOCAB_RESIDENT", "0"),):
        assert m.e.get_config_int("vocab_resident_rows") == 0
    yield m
    m.close()


def _check_forced(m, logits, chosen, ids, lp=None):
    """Every decision against the Python rules on the launch's own row; scored: its log-probability as well."""
    left_out = 0
    for i in range(len(ids) + 1):
        c, ref, info = sr.token_logprob(logits[i], ids[:i], m.T, m.E)
        py, tinfo = tsr.decide(logits[i], ids[:i], m.T, m.E)
        assert c == py
        if chosen[i] != py:
            assert tinfo["margin"] < 1e-4, (i, int(chosen[i]), py, tinfo)
            left_out += 1
            continue
        if lp is not None:
            assert _close(lp[i], ref, _bar(info["x_chosen"], info["lse_allowed"])), (i, float(lp[i]), float(ref), info)
    assert left_out <= 1, left_out


def test_forced_timestamp_mode(model):
    """Mode 1, one clip, teacher-forced with the oracle's ids: ONE launch, every step's decision as the Python rules decide on the
    launch's own dumped row; the switched-off handle dumps rows that agree to the 16-bit storage error and moves no counter."""
    m = model
    ids, _, rows = m.oracle_run(0)
    f = np.array([ids], dtype=np.int32).reshape(1, len(ids))
    m.e.encode_mel(m.mels[0])
    c0 = m.count()
    logits, chosen = m.e.decode_forced_timestamps(1, f)
    assert m.count() == c0 + 1
    assert chosen.shape == (1, len(ids) + 1)
    _check_forced(m, logits[0], chosen[0], ids)
    m.off.encode_mel(m.mels[0])
    lo, co = m.off.decode_forced_timestamps(1, f)
    assert m.off.persistent_ts_launches == 0
    err = float(np.abs(logits[0] - lo[0]).max())
    print("forced rows: launch against launch-per-phase max |diff| %.3g, against the oracle %.3g" % (err, float(np.abs(logits[0] - rows).max())))
    assert err < 5e-2


def test_forced_scored_mode(model):
    """Mode 2: decisions, log-probabilities and the no-speech value on the launch's own rows (offset 0 included)."""
    m = model
    ids, _, _ = m.oracle_run(1)
    f = np.array([ids], dtype=np.int32).reshape(1, len(ids))
    m.e.encode_mel(m.mels[1])
    c0 = m.count()
    logits, chosen, lp, nsp, l0 = m.e.decode_forced_timestamp_scores(1, f)
    assert m.count() == c0 + 1
    _check_forced(m, logits[0], chosen[0], ids, lp[0])
    ref = sr.no_speech_logprob(l0[0], m.NS)
    assert _close(nsp[0], ref, _bar(float(l0[0, m.NS]), tsr._lse(l0[0].astype(np.float64)))), (float(nsp[0]), float(ref))
    _, plain_chosen = m.e.decode_forced_timestamps(1, f, want_logits=False)
    assert np.array_equal(chosen, plain_chosen) and m.count() == c0 + 2  # the scored launch decides as the unscored one


def _tie_or_equal(m, k, got, want_ids, infos, rows, what):
    """`got` equals the oracle's ids, or the first divergence is a measured tie (test_greedy_ids_match_the_oracle's rule)."""
    if got == want_ids:
        return
    n = min(len(got), len(want_ids))
    i = next((i for i in range(n) if got[i] != want_ids[i]), n)
    m.e.encode_mel(m.mels[k])
    lg, _ = m.e.decode_forced_timestamps(1, np.array([want_ids[:i]], dtype=np.int32).reshape(1, i))
    err = float(np.abs(lg[0, i] - rows[i]).max())
    assert infos[i]["margin"] < 2 * err + 1e-4, (what, k, "step", i, infos[i], "logit err", err, want_ids, got)


@pytest.mark.parametrize("k", [0, 2])
def test_greedy_ids(model, k):
    """Greedy ids of one clip: against the oracle loop and against the switched-off handle; scored ids equal unscored ids; two runs
    on the same handle are bit-equal, scores included."""
    m = model
    ids, infos, rows = m.oracle_run(k)
    c0 = m.count()
    got = m.e.run_timestamp_tokens_batch([m.clips[k]], max_new=MAX_NEW)[0]
    again = m.e.run_timestamp_tokens_batch([m.clips[k]], max_new=MAX_NEW)[0]
    sc = m.e.run_timestamp_scores_batch([m.clips[k]], max_new=MAX_NEW)[0]
    sc2 = m.e.run_timestamp_scores_batch([m.clips[k]], max_new=MAX_NEW)[0]
    assert m.count() == c0 + 4
    assert got == again == sc["ids"] == sc2["ids"]
    assert np.array_equal(sc["token_logprob"], sc2["token_logprob"]) and sc["no_speech_logprob"] == sc2["no_speech_logprob"]
    assert any(t >= m.T for t in got)
    _tie_or_equal(m, k, got, ids, infos, rows, "oracle")
    want = m.off.run_timestamp_tokens_batch([m.clips[k]], max_new=MAX_NEW)[0]
    assert m.off.persistent_ts_launches == 0
    if got != want:  # both routes against the oracle: each one equal or tied at ITS first divergence
        _tie_or_equal(m, k, want, ids, infos, rows, "switched off")


def test_stop_conditions(model):
    """A budget of 5 and the context end (445 ids: every position of the 448 behind the three-id prefix); neither sets ended_eot."""
    m = model
    c0 = m.count()
    full = m.e.run_timestamp_scores_batch([m.clips[0]], max_new=MAX_NEW)[0]
    cut = m.e.run_timestamp_scores_batch([m.clips[0]], max_new=5)[0]
    assert len(full["ids"]) > 5 and cut["ids"] == full["ids"][:5] and not cut["ended_eot"]
    assert len(cut["token_logprob"]) == 6 and np.array_equal(cut["token_logprob"], full["token_logprob"][:6])
    if len(full["ids"]) < MAX_NEW:
        assert full["ended_eot"]
    long_ids = m.e.run_timestamp_tokens_batch([m.clips[0]], max_new=0)[0]
    long_sc = m.e.run_timestamp_scores_batch([m.clips[0]], max_new=0)[0]
    assert m.count() == c0 + 4
    n_ctx = m.e.n_text_ctx
    # no eot in reach of these seeded weights (the eot stop: test_loop_ends_on_eot below): the loop runs to the context end, 445 ids
    # behind the three-id prefix, and the decision at the last position is dropped
    assert len(long_ids) == n_ctx - 3 == 445 and long_ids[: len(full["ids"])] == full["ids"] and long_sc["ids"] == long_ids
    assert len(long_sc["token_logprob"]) == 446
    want = m.off.run_timestamp_scores_batch([m.clips[0]], max_new=0)[0]
    if want["ids"] == long_ids:
        assert want["ended_eot"] == long_sc["ended_eot"]
    print("context run: %d ids, ended_eot %s (switched off: %d ids)" % (len(long_ids), long_sc["ended_eot"], len(want["ids"])))


def test_suppression(model):
    """The "non_speech" set installed: no decision is in the set, and every decision is the Python rules' on the launch's own row
    with the set's ids at -inf (suppress_reference.suppress_rows)."""
    m = model
    try:
        m.e.set_suppress_tokens("non_speech")
        sup = m.e.suppress_tokens
        assert sup and m.e.get_config_int("n_suppress_tokens") == len(sup)
        c0 = m.count()
        got = m.e.run_timestamp_tokens_batch([m.clips[0]], max_new=MAX_NEW)[0]
        assert not (set(got) & set(sup))
        m.e.encode_mel(m.mels[0])
        f = np.array([got], dtype=np.int32).reshape(1, len(got))
        logits, chosen, lp, _, _ = m.e.decode_forced_timestamp_scores(1, f)
        assert m.count() == c0 + 2
        assert chosen[0, : len(got)].tolist() == got
        rows = supr.suppress_rows(logits[0], sup)
        left_out = 0
        for i in range(len(got) + 1):
            c, ref, info = sr.token_logprob(rows[i], got[:i], m.T, m.E)
            assert c not in sup
            if int(chosen[0, i]) != c:
                assert info["margin"] < 1e-4, (i, int(chosen[0, i]), c, info)
                left_out += 1
                continue
            assert _close(lp[0, i], ref, _bar(info["x_chosen"], info["lse_allowed"])), (i, float(lp[0, i]), float(ref))
        assert left_out <= 1
    finally:
        m.e.set_suppress_tokens(None)


def test_requests_that_stay_on_the_step_path(model):
    """A prompt, a language per clip, two clips: the counter stays, the ids are the switched-off handle's."""
    m = model
    c0 = m.count()
    prompts = [[17, 23, 5]]
    ids = lambda res: [list(r["ids"]) for r in res]  # noqa: E731
    assert ids(m.e.run_timestamp_prompted_batch([m.clips[0]], prompts, max_new=12)) == ids(m.off.run_timestamp_prompted_batch([m.clips[0]], prompts, max_new=12))
    assert ids(m.e.run_timestamp_lang_batch([m.clips[0]], languages=["en"], max_new=12)) == ids(m.off.run_timestamp_lang_batch([m.clips[0]], languages=["en"], max_new=12))
    assert m.e.run_timestamp_tokens_batch(m.clips[:2], max_new=12) == m.off.run_timestamp_tokens_batch(m.clips[:2], max_new=12)
    assert m.count() == c0


def test_give_up_falls_back(built_lib, oracle_mod, tmp_path, monkeypatch):
    """The launch's fault hook once, in timestamp mode: the fallback's ids, persistent_giveups rises, the counter does not."""
    case = ModelCase(tmp_path, "micro", 11)
    clip = load_demo_pcm()
    monkeypatch.setenv("AX_WHISPER_PERSIST_TS", "0")
    off = built_lib.Whisper("micro", case.root, "zh", device=0, max_batch=1)
    monkeypatch.setenv("AX_WHISPER_PERSIST_TS", "1")
    e = built_lib.Whisper("micro", case.root, "zh", device=0, max_batch=1)
    monkeypatch.delenv("AX_WHISPER_PERSIST_TS")
    try:
        want = off.run_timestamp_tokens_batch([clip], max_new=20)[0]
        e.run_timestamp_tokens_batch([clip], max_new=20)
        assert e.persistent_ts_launches == 1 and e.get_config_int("persistent_giveups") == 0
        monkeypatch.setenv("AX_WHISPER_PERSIST_FAULT", "1")
        got = e.run_timestamp_tokens_batch([clip], max_new=20)[0]
        monkeypatch.delenv("AX_WHISPER_PERSIST_FAULT")
        assert got == want
        assert e.persistent_ts_launches == 1 and e.get_config_int("persistent_giveups") == 1 and e.get_config_int("persistent_decode") == 0
        assert off.persistent_ts_launches == 0
    finally:
        e.close()
        off.close()


def _assert_window_tie(m, audio, seek, a, b):
    """Two id lists of one window part at step j: the oracle's decision margin there is below 2 x the logit error of the launch's
    own row + 1e-4 (test_greedy_ids_match_the_oracle's rule)."""
    n = min(len(a), len(b))
    j = next((j for j in range(n) if a[j] != b[j]), n)
    mel = m.e.compute_mel_window(audio, seek)
    ck, cv = m.orc.encoder(mel)
    _, rows = sr.oracle_rows(m.orc, ck, cv, m.prefix, a[:j])
    _, info = tsr.decide(rows[j], a[:j], m.T, m.E)
    m.e.encode_mel(mel)
    lg, _ = m.e.decode_forced_timestamps(1, np.array([a[:j]], dtype=np.int32).reshape(1, j))
    err = float(np.abs(lg[0, j] - rows[j]).max())
    assert info["margin"] < 2 * err + 1e-4, ("seek", seek, "step", j, info, "logit err", err)


def _route_error(m, mel, ids):
    """Both handles teacher-forced with `ids` on `mel` (scored): the largest difference of their dumped rows, offset 0 included, and
    the largest magnitude in them. A log-probability is x[c] - logsumexp(x[A]) on such a row, so the two routes' values differ by at
    most 2 x that difference plus each route's own float32 bar (test_gpu_scores.py: 1e-4 + 1e-6 * magnitude)."""
    f = np.array([ids], dtype=np.int32).reshape(1, len(ids))
    m.e.encode_mel(mel)
    la, _, _, _, l0a = m.e.decode_forced_timestamp_scores(1, f)
    m.off.encode_mel(mel)
    lb, _, _, _, l0b = m.off.decode_forced_timestamp_scores(1, f)
    err = max(float(np.abs(la - lb).max()), float(np.abs(l0a - l0b).max()))
    mag = max(float(np.abs(la[np.isfinite(la)]).max()), float(np.abs(l0a[np.isfinite(l0a)]).max()))
    return 2 * err + 2 * (1e-4 + 1e-6 * mag)


@pytest.mark.parametrize("thresholds", [False, True], ids=["plain", "thresholds"])
def test_long_form_windows(model, thresholds):
    """One file of three windows through run_long_windows: one launch per decoded window; the log is the switched-off handle's —
    seek, window length, advance, ids, pass and slot of every window, and with thresholds the skip decision and the two scores
    within the routes' row error — or the first window that differs has the same seek and its ids part at a measured tie."""
    m = model
    pcm = load_demo_pcm()
    reps = int(math.ceil(70 * 16000 / len(pcm)))
    audio = np.concatenate([pcm * np.float32(1.0 - 0.1 * (i % 3)) for i in range(reps)])[: 70 * 16000]
    kw = dict(no_speech_threshold=0.6, logprob_threshold=-1.0) if thresholds else {}
    c0 = m.count()
    log = m.e.run_long_windows([audio], max_new=MAX_NEW, **kw)[0]
    n_launch = m.count() - c0
    want = m.off.run_long_windows([audio], max_new=MAX_NEW, **kw)[0]
    assert len(log) >= 3
    assert n_launch == len(log), (n_launch, len(log))  # every window of the log was decoded, skipped or not
    key = lambda w: tuple(w[:6])  # noqa: E731  (seek, window frames, advance, ids, pass, slot)
    n_same = next((i for i, (wa, wb) in enumerate(zip(log, want)) if key(wa) != key(wb)), min(len(log), len(want)))
    for wa, wb in zip(log[:n_same], want[:n_same]):
        if thresholds:
            bound = _route_error(m, m.e.compute_mel_window(audio, wa[0]), wa[3])
            assert wa[8] == wb[8] and abs(wa[6] - wb[6]) <= bound and abs(wa[7] - wb[7]) <= bound, (wa, wb, bound)
    if n_same < max(len(log), len(want)):
        i = n_same
        assert i < min(len(log), len(want)) and log[i][0] == want[i][0] and log[i][3] != want[i][3], (i, log[i:i + 1], want[i:i + 1])
        _assert_window_tie(m, audio, log[i][0], log[i][3], want[i][3])


class EotModel:
    """A seeded model whose greedy loop ENDS ON eot: eot's row of the tied token embedding times 64 (a power of two: the weights
    stay 16-bit values; eot is never fed, so nothing but its own logit moves). On the CPU oracle the timestamp-mode loop then ends
    on eot after 13 ids (micro, seed 11, smallest margin 2.0e-3, 4.1 at the stop) and after 1 id (miniturbo, seed 21, 5.7e-2, 3.8)."""

    def __init__(self, built_lib, mp, tmp, model_type, seed, dtype):
        import modelgen
        import oracle
        from conftest import GOLDEN

        self.dims = modelgen.DIMS[model_type]
        w = modelgen.synth_weights(self.dims, seed, bf16=(dtype != "F16"))
        if dtype == "F16":
            w = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
        self.cfg = modelgen.make_config(model_type, self.dims)
        emb = w["decoder.token_embedding.weight"].copy()
        emb[int(self.cfg["eot"])] *= np.float32(64.0)
        w["decoder.token_embedding.weight"] = emb
        self.root = str(tmp)
        modelgen.write_model_dir(self.root, model_type, self.dims, weights=w, dtype=dtype, tiktoken_path=os.path.join(GOLDEN, "multilingual.tiktoken"))
        self.orc = oracle.Oracle(self.cfg, w, bf16_policy=2 if dtype == "F16" else True)
        mp.setenv("AX_WHISPER_PERSIST_TS", "1")
        self.e = built_lib.Whisper(model_type, self.root, "zh", device=0, max_batch=1)
        mp.setenv("AX_WHISPER_PERSIST_TS", "0")
        self.off = built_lib.Whisper(model_type, self.root, "zh", device=0, max_batch=1)
        mp.delenv("AX_WHISPER_PERSIST_TS")
        self.T, self.E, self.NS = self.e.timestamp_begin, self.e.eot, self.e.no_speech
        self.clip = load_demo_pcm()
        self.mel = oracle.log_mel(self.clip, self.dims["n_mels"])[0]
        self.prefix = self.orc.sot_seq("zh")[:3]


@pytest.mark.parametrize("model_type,seed,dtype,n_ids", [("micro", 11, "BF16", 13), ("miniturbo", 21, "F16", 1)])
def test_loop_ends_on_eot(built_lib, oracle_mod, tmp_path, model_type, seed, dtype, n_ids):
    """The launch's eot stop end to end: the ids are the oracle's and stop where it decides eot, ended_eot is set, the eot decision's
    log-probability stands at index n_ids and counts in avg_logprob, every value against score_reference on the launch's own rows,
    and all of it against the switched-off handle."""
    mp = pytest.MonkeyPatch()
    m = EotModel(built_lib, mp, tmp_path, model_type, seed, dtype)
    mp.undo()
    try:
        assert m.e.get_config_int("persistent_ts") == 1
        ck, cv = m.orc.encoder(m.mel)
        ids, infos = tsr.greedy_ts(m.orc, ck, cv, m.prefix, max_new=MAX_NEW)
        assert len(ids) == n_ids and len(infos) == n_ids + 1 and min(i["margin"] for i in infos) > 1e-3  # the oracle ends on eot, no tie
        g = m.e.run_timestamp_scores_batch([m.clip], max_new=MAX_NEW)[0]
        plain = m.e.run_timestamp_tokens_batch([m.clip], max_new=MAX_NEW)[0]
        assert m.e.persistent_ts_launches == 2
        assert g["ids"] == ids == plain and g["ended_eot"] and m.E not in g["ids"]
        n = len(ids)
        assert len(g["token_logprob"]) == n + 1
        # the launch's own rows, teacher-forced with the ids over the cross K/V the two runs above left in the slot (the engine's own
        # front-end, not the oracle's log-mel): decision n is eot, every log-probability is the reference's
        logits, chosen, lp, nsp, l0 = m.e.decode_forced_timestamp_scores(1, np.array([ids], dtype=np.int32).reshape(1, n))
        assert chosen[0].tolist() == ids + [m.E]
        for i in range(n + 1):
            c, ref, info = sr.token_logprob(logits[0, i], ids[:i], m.T, m.E)
            assert c == (ids[i] if i < n else m.E)
            bar = _bar(info["x_chosen"], info["lse_allowed"])
            assert _close(g["token_logprob"][i], ref, bar) and _close(lp[0, i], ref, bar), (i, float(g["token_logprob"][i]), float(lp[0, i]), float(ref))
        ref_ns = sr.no_speech_logprob(l0[0], m.NS)
        assert _close(g["no_speech_logprob"], ref_ns, _bar(float(l0[0, m.NS]), tsr._lse(l0[0].astype(np.float64))))
        want_avg = sr.avg_logprob(g["token_logprob"], n, True)  # the eot decision's value counts: sum of n + 1 values / (n + 1)
        assert _close(g["avg_logprob"], want_avg, 1e-6 * max(1.0, abs(float(want_avg)))), (g["avg_logprob"], want_avg)
        assert _close(g["avg_logprob"], float(np.sum(g["token_logprob"].astype(np.float64))) / (n + 1), 1e-5)
        # the switched-off handle: the same ids and stop, scores within the routes' row error
        o = m.off.run_timestamp_scores_batch([m.clip], max_new=MAX_NEW)[0]
        assert m.off.persistent_ts_launches == 0
        assert o["ids"] == ids and o["ended_eot"] and len(o["token_logprob"]) == n + 1
        bound = _route_error(m, m.mel, ids)
        assert np.all(np.abs(g["token_logprob"] - o["token_logprob"]) <= bound), (g["token_logprob"], o["token_logprob"], bound)
        assert abs(g["avg_logprob"] - o["avg_logprob"]) <= bound and abs(g["no_speech_logprob"] - o["no_speech_logprob"]) <= bound
    finally:
        m.e.close()
        m.off.close()
