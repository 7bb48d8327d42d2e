"""GPU: token suppression (DESIGN.md "Token suppression") — the rules kernels under a suppress set S against the same kernels with
the empty set on rows that hold -inf at the ids of S (bit for bit) and against the numpy references on those rows, the decode
loops under a set, and the plumbing (config key, setter, stream, CLI).

Bars. With S on rows X against the empty set on suppress_rows(X, S): exact, ids and the bits of every float. Against the references
on suppress_rows(X, S): the bars of the tests those references come with — ids exact except where the reference's own decision
margin is below 1e-4 (scored, beam: rule 5 near ties) or its two best keys are a near tie (sampled), at most 1 % of the decisions;
log-probabilities within 1e-4 + 1e-6 * max(|x[c]|, |logsumexp|)."""
import collections
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import beam_reference as br
import longform_reference as lfr
import sample_reference as smp
import score_reference as sr
import suppress_reference as sup
import ts_reference as tsr
from conftest import GOLDEN, ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

MAX_NEW = 12
SEED = 0x5EED
NON_SPEECH = json.load(open(os.path.join(GOLDEN, "non_speech_multilingual.json")))


def _bar(xc, lse):
    m = max(abs(xc) if math.isfinite(xc) else 0.0, abs(lse) if math.isfinite(lse) else 0.0)
    return 1e-4 + 1e-6 * m


def _close(got, want, bar):
    got, want = float(got), float(want)
    if not math.isfinite(want) or not math.isfinite(got):
        return got == want or (math.isnan(got) and math.isnan(want))
    return abs(got - want) <= bar


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


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
        assert self.e.get_config_int("n_suppress_tokens") == 0 and self.e.suppress_tokens == []
        # what a handle that never had a set returns on the base rows (taken before this handle gets its first one)
        self.base, self.hists = self._base_rows()
        self.never = self.kernels(self.base)
        self._greedy = {}

    def _base_rows(self):
        """16 seeded rows, four under each history: none (timestamps only), text on, pair open (text off), pair just closed."""
        T = self.T
        rng = np.random.default_rng(2718)
        hists = [[], [T, 5, 9], [T, 5, T + 30], [T, 5, T + 30, T + 30]]
        rows, hs = [], []
        for k in range(16):
            std = (1.0, 3.0, 10.0, 3.0)[k // 4]
            rows.append((rng.standard_normal(self.nv) * std).astype(np.float32))
            hs.append(hists[k % 4])
        return np.stack(rows), hs

    def rows_for(self, ids):
        """The base rows with each row's largest text logit placed on an id of the set below eot; rows 1 and 5 (text on) are the
        crafted ones. Row 1: the timestamps' mass lies between the best and the second-best text logit, so rule 5 fires only under
        the set. Row 5: eot is the best id that is left, and stays allowed."""
        T, E = self.T, self.E
        text = sorted({i for i in ids if i < E})
        assert text
        x = self.base.copy()
        for b in range(len(x)):
            x[b, text[b % len(text)]] = x[b, :E].max() + np.float32(2.0)
        rng = np.random.default_rng(31)
        x[1, :E + 1] = (rng.standard_normal(E + 1) * 0.3).astype(np.float32)
        x[1, T:] = (-5.0 + 0.1 * rng.standard_normal(self.nv - T)).astype(np.float32)  # logsumexp about 2.3
        x[1, text[0]] = 6.0
        x[5, :E] = (rng.standard_normal(E) * 0.3).astype(np.float32)
        x[5, T:] = (-9.0 + 0.1 * rng.standard_normal(self.nv - T)).astype(np.float32)
        x[5, text[-1]] = 7.0
        x[5, E] = 4.0
        return x

    def kernels(self, x):
        """Every rules entry point on rows x under the handle's set -> dict of outputs (ids as lists, floats as arrays)."""
        e, h = self.e, self.hists
        n = len(x)
        out = {"plain": e.apply_timestamp_rules(x, h)}
        out["scored"] = e.score_timestamp_rules(x, h)
        for t in (0.0, 0.7):
            for seed in (SEED, SEED + 1):
                out["sampled", t, seed] = e.sample_timestamp_rules(x, h, t, self.streams(n), seed)
        for M in (2, 9):
            out["beam", M] = e.beam_candidates(x, h, M)
        o = e.stream_rules_stage(x, [len(s) + 2 for s in h], [0] * n, [0] * n, h, [[11, 22, 33, 44]] * n)
        out["stream"] = (o["chosen"].tolist(), o["logprob"])
        return out

    @staticmethod
    def streams(n):
        return [(b * 7 + 1) | ((b % 3) << 32) for b in range(n)]

    def greedy(self, batch):
        """run_timestamp_scores_batch of `batch` clips with the empty set, once per batch size"""
        if batch not in self._greedy:
            assert self.e.suppress_tokens == []
            nc = len(self.clips)
            self._greedy[batch] = self.e.run_timestamp_scores_batch([self.clips[b % nc] for b in range(batch)], max_new=MAX_NEW)
        return self._greedy[batch]

    def loop_set(self, outputs):
        """the non-speech ids plus the three text ids most frequent in the given id lists"""
        count = collections.Counter(i for ids in outputs for i in ids if i < self.E)
        top = [i for i, _ in count.most_common(3)]
        assert len(top) == 3, count
        return sorted(set(NON_SPEECH) | set(top)), top


def _same(a, b, what):
    """two results of Model.kernels: equal ids (and their order), equal bits of every float"""
    assert a.keys() == b.keys()
    for k in a:
        for u, v in zip(*([[a[k]], [b[k]]] if isinstance(a[k], list) else [a[k], b[k]])):
            if isinstance(u, list):
                assert u == v, (what, k, u, v)
            elif u.dtype.kind == "f":
                assert _bits(u) == _bits(v), (what, k, u, v)
            else:
                assert np.array_equal(u, v), (what, k, u, v)


PARAMS = [("micro", 11, "BF16"), ("miniturbo", 21, "F16")]


@pytest.fixture(scope="module", params=PARAMS, ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("sup_" + request.param[0]), *request.param)
    yield m
    m.e.close()


def _sets(E, T):
    return {"non_speech": NON_SPEECH, "id0": [0], "ids3_4": [3, 4], "ids31_32_33": [31, 32, 33], "ids1023_1024": [1023, 1024],
            "eot_minus_1": [E - 1], "all_text": list(range(E)), "special_and_duplicates": [5, 5, E + 1, T - 1, 77, 77, E + 1, 40000]}


# ---------------------------------------------------------------------------------------------------- 1: the kernels alone
@pytest.mark.parametrize("name", list(_sets(50257, 50364)))
def test_kernels_under_a_set_equal_the_empty_set_on_filtered_rows(model, name):
    m, e, T, E = model, model.e, model.T, model.E
    S = _sets(E, T)[name]
    x = m.rows_for(S)
    y = sup.suppress_rows(x, S)
    # the crafted rows do what they are there for
    assert not tsr.decide(x[1], m.hists[1], T, E)[1]["rule5"] and tsr.decide(y[1], m.hists[1], T, E)[1]["rule5"]
    assert tsr.decide(x[1], m.hists[1], T, E)[0] < E and tsr.decide(y[1], m.hists[1], T, E)[0] >= T
    assert tsr.decide(y[5], m.hists[5], T, E)[0] == E
    e.set_suppress_tokens(S)
    try:
        assert e.suppress_tokens == sorted(set(S)) and e.get_config_int("n_suppress_tokens") == len(set(S))
        with_set = m.kernels(x)
    finally:
        e.set_suppress_tokens([])
    assert e.suppress_tokens == [] and e.get_config_int("n_suppress_tokens") == 0
    _same(with_set, m.kernels(y), name)
    # back to the empty set: what a handle that never had one returns
    _same(m.kernels(m.base), m.never, name + ": empty again")
    # ---- and the references on the filtered rows
    text = set(i for i in S if i < E)
    n = len(x)
    assert with_set["plain"] == with_set["scored"][0] == with_set["stream"][0]
    assert _bits(with_set["scored"][1]) == _bits(with_set["stream"][1])
    assert with_set["plain"][1] >= T and with_set["plain"][5] == E
    left_out = 0
    for b in range(n):
        c, ref, info = sr.token_logprob(y[b], m.hists[b], T, E)
        g = with_set["scored"][0][b]
        assert g not in text
        if g != c:
            assert info["margin"] < 1e-4, (name, b, g, c, info)
            left_out += 1
            continue
        assert _close(with_set["scored"][1][b], ref, _bar(info["x_chosen"], info["lse_allowed"])), (name, b, float(with_set["scored"][1][b]), float(ref))
    assert left_out == 0, (name, left_out)  # (16 rows: 1 % is none)
    near = 0
    for t in (0.0, 0.7):
        for seed in (SEED, SEED + 1):
            got, lps = with_set["sampled", t, seed]
            for b in range(n):
                c, ref, info = smp.sample(y[b], m.hists[b], T, E, t, m.streams(n)[b], seed)
                assert got[b] not in text
                if got[b] != c:
                    assert info["near_tie"] and got[b] == info["runner_up"], (name, t, seed, b, got[b], c, info)
                    near += 1
                    continue
                assert _close(lps[b], ref, _bar(info["x_chosen"], info["lse_allowed"])), (name, t, seed, b, float(lps[b]), float(ref))
    assert near == 0, (name, near)  # (64 decisions: 1 % is none)
    for M in (2, 9):
        cid, clp, nc = with_set["beam", M]
        for b in range(n):
            ids, lps, info = br.candidates(y[b], m.hists[b], T, E, M)
            g = [int(v) for v in cid[b, : nc[b]]]
            assert not text & set(g)
            assert g == ids, (name, M, b, g, ids, info)  # (no row here is a rule-5 near tie: asserted by the reference's margin)
            assert not br.rule5_near_tie(info)
            for q, c in enumerate(ids):
                assert _close(clp[b, q], lps[q], _bar(float(y[b, c]), info["lse_allowed"])), (name, M, b, q)
    if name == "all_text":  # only eot and the timestamps remain
        assert all(g == E or g >= T for g in with_set["plain"])
        assert all(int(v) == E or int(v) >= T for v in with_set["beam", 9][0].reshape(-1))


def test_setter_refusals(model):
    e, T, E, nv = model.e, model.T, model.E, model.nv
    for bad, text in (([E], "eot"), ([T], "timestamp id"), ([nv - 1], "timestamp id"), ([nv], "outside the vocabulary"), ([-1], "outside the vocabulary"),
                      ([0] * (nv + 1), "entries for a vocabulary")):
        with pytest.raises(RuntimeError, match=text):
            e.set_suppress_tokens(bad)
        assert e.suppress_tokens == []
    e.set_suppress_tokens("non_speech")
    assert e.suppress_tokens == NON_SPEECH
    e.stream_open(2, timestamps=True)
    try:
        with pytest.raises(RuntimeError, match="stream"):
            e.set_suppress_tokens([7])
        assert e.suppress_tokens == NON_SPEECH
    finally:
        e.stream_close()
    e.set_suppress_tokens(None)
    assert e.suppress_tokens == []


# ---------------------------------------------------------------------------------------------------- 2: the loops
def _check_scored_rows(m, S, got, logits, chosen, lp, clips_to_check, what):
    """Every step of the checked clips: the reference's decision on the filtered row is the decoded id, log-probabilities within the bar"""
    T, E = m.T, m.E
    left_out = total = 0
    for b in clips_to_check:
        ids = got[b]["ids"]
        for i in range(len(ids) + 1):
            c, ref, info = sr.token_logprob(sup.suppress_rows(logits[b, i], S), ids[:i], T, E)
            total += 1
            if int(chosen[b, i]) != c:
                assert info["margin"] < 1e-4, (what, b, i, int(chosen[b, i]), c, info)
                left_out += 1
                continue
            assert _close(lp[b, i], ref, _bar(info["x_chosen"], info["lse_allowed"])), (what, b, i, float(lp[b, i]), float(ref))
            assert _close(got[b]["token_logprob"][i], ref, _bar(info["x_chosen"], info["lse_allowed"])), (what, b, i)
    assert left_out * 49 <= total, (what, left_out, total)


@pytest.mark.parametrize("batch", [1, 4, 24])
def test_scored_loop_under_a_set(model, batch):
    """Batches 1, 4 and 24: the GEMV family, the one-branch and the multi-branch step."""
    m, e = model, model.e
    nc = len(m.clips)
    clips = [m.clips[b % nc] for b in range(batch)]
    before = m.greedy(batch)
    S, top = m.loop_set([g["ids"] for g in before])
    e.set_suppress_tokens(S)
    try:
        got = e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
        n = [len(g["ids"]) for g in got]
        assert all(not set(g["ids"]) & set(S) for g in got)
        assert any(g["ids"] != b4["ids"] for g, b4 in zip(got, before))
        f = np.zeros((batch, max(n)), dtype=np.int32)
        for b, g in enumerate(got):
            f[b, : n[b]] = g["ids"]
        # the slots still hold this call's cross K/V
        logits, chosen, lp, _, _ = e.decode_forced_timestamp_scores(batch, f)
        for b in range(batch):
            assert chosen[b, : n[b]].tolist() == got[b]["ids"], (batch, b)
        _check_scored_rows(m, S, got, logits, chosen, lp, range(min(batch, nc + 1)), "scored loop, batch %d" % batch)
    finally:
        e.set_suppress_tokens([])
    # the step graphs of the empty set are the ones the handle replays again
    again = e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
    assert [g["ids"] for g in again] == [g["ids"] for g in before]
    assert all(_bits(a["token_logprob"]) == _bits(b4["token_logprob"]) for a, b4 in zip(again, before))


def test_sampled_loop_under_a_set(model):
    m, e, T, E = model, model.e, model.T, model.E
    batch = 4
    clips = m.clips[:batch]
    temps, streams = [0.7] * batch, [(b * 3 + 1) | (b << 32) for b in range(batch)]
    before = e.run_timestamp_sampled_batch(clips, temps, streams, SEED, max_new=MAX_NEW)
    S, _ = m.loop_set([g["ids"] for g in before])
    e.set_suppress_tokens(S)
    try:
        got = e.run_timestamp_sampled_batch(clips, temps, streams, SEED, max_new=MAX_NEW)
        n = [len(g["ids"]) for g in got]
        assert all(not set(g["ids"]) & set(S) for g in got)
        f = np.zeros((batch, max(n)), dtype=np.int32)
        for b, g in enumerate(got):
            f[b, : n[b]] = g["ids"]
        logits, chosen, lp, _, _ = e.decode_forced_timestamp_sampled(batch, f, temps, streams, SEED)
    finally:
        e.set_suppress_tokens([])
    left_out = total = 0
    for b in range(batch):
        assert chosen[b, : n[b]].tolist() == got[b]["ids"], b
        for i in range(n[b] + 1):
            c, ref, info = smp.sample(sup.suppress_rows(logits[b, i], S), got[b]["ids"][:i], T, E, temps[b], streams[b], SEED)
            total += 1
            if int(chosen[b, i]) != c:
                assert info["near_tie"] and int(chosen[b, i]) == info["runner_up"], (b, i, int(chosen[b, i]), c, info)
                left_out += 1
                continue
            assert _close(lp[b, i], ref, _bar(info["x_chosen"], info["lse_allowed"])), (b, i, float(lp[b, i]), float(ref))
    assert left_out * 100 <= total, (left_out, total)


def test_beam_under_a_set(model):
    m, e = model, model.e
    clips = m.clips[:2]
    before = m.greedy(4)[:2]  # (the first two clips of the batch of four are these two)
    S, _ = m.loop_set([g["ids"] for g in before] + [r["ids"] for r in e.run_beam_batch(clips, 5, MAX_NEW)])
    e.set_suppress_tokens(S)
    try:
        greedy = e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
        one = e.run_beam_batch(clips, 1, MAX_NEW)
        assert [r["ids"] for r in one] == [g["ids"] for g in greedy]  # K = 1 is scored greedy, under the set too
        batch5 = e.run_beam_batch(clips, 5, MAX_NEW)
        assert all(len(r["ids"]) >= 1 and not set(r["ids"]) & set(S) for r in batch5)
        mels = np.stack([e.compute_mel(c) for c in clips])
        e.encode_mel(mels)
        five, _ = e.decode_beam(2, 5, MAX_NEW)
        for r in five:
            assert not set(r["ids"]) & set(S)
            assert len(r["records"]) >= 1 and all(not set(int(i) for i in ids) & set(S) for ids, _, _ in r["records"])
        assert [r["ids"] for r in five] == [r["ids"] for r in batch5]  # the batch call is the stage-level one behind the front-end
    finally:
        e.set_suppress_tokens([])


def test_long_form_under_a_set(model):
    m, e = model, model.e
    f = lfr.make_file(load_demo_pcm(), 3)  # 45 s: two windows
    before = e.run_long_windows([f], max_new=MAX_NEW)[0]
    assert len(before) >= 2
    S, _ = m.loop_set([w[3] for w in before])
    e.set_suppress_tokens(S)
    try:
        got = e.run_long_windows([f], max_new=MAX_NEW)[0]
    finally:
        e.set_suppress_tokens([])
    assert len(got) >= 2 and all(len(w[3]) >= 1 and not set(w[3]) & set(S) for w in got)
    assert e.run_long_windows([f], max_new=MAX_NEW)[0] == before


def test_stream_under_a_set(model):
    m, e = model, model.e
    clips = m.clips[:3]
    before = e.run_stream_timestamps(clips, 2, max_new=MAX_NEW)
    S, _ = m.loop_set([r[1] for r in before])
    e.set_suppress_tokens(S)
    try:
        got = e.run_stream_timestamps(clips, 2, max_new=MAX_NEW)  # a stream opened after the set uses it
        scored = e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
    finally:
        e.set_suppress_tokens([])
    assert all(len(r[1]) >= 1 and not set(r[1]) & set(S) for r in got)
    assert [list(r[1]) for r in got] == [g["ids"] for g in scored]  # as the batch call under the same set
    assert [list(r[1]) for r in e.run_stream_timestamps(clips, 2, max_new=MAX_NEW)] == [list(r[1]) for r in before]


# ---------------------------------------------------------------------------------------------------- 3: plumbing
def test_config_key_installs_the_set(model, tmp_path):
    m = model
    t = m.case.model_type
    d = tmp_path / t
    d.mkdir()
    for name in os.listdir(os.path.join(m.case.root, t)):
        if not name.endswith("_config.json"):
            os.symlink(os.path.join(m.case.root, t, name), d / name)
    cfg = dict(m.case.cfg, suppress_tokens=[-1])
    (d / (t + "_config.json")).write_text(json.dumps(cfg))
    e = m.lib.Whisper(t, str(tmp_path), "zh", device=0, max_batch=2)
    try:
        assert e.get_config_int("n_suppress_tokens") == 82 and e.suppress_tokens == NON_SPEECH
        x = m.rows_for(NON_SPEECH)
        want = m.e.score_timestamp_rules(sup.suppress_rows(x, NON_SPEECH), m.hists)
        got = e.score_timestamp_rules(x, m.hists)
        assert got[0] == want[0] and _bits(got[1]) == _bits(want[1])
        e.set_suppress_tokens([3, 4])
        assert e.suppress_tokens == [3, 4] and e.get_config_int("n_suppress_tokens") == 2
        e.set_suppress_tokens([])  # back to what the config file gave
        assert e.get_config_int("n_suppress_tokens") == 82 and e.suppress_tokens == NON_SPEECH
        got = e.score_timestamp_rules(x, m.hists)
        assert got[0] == want[0] and _bits(got[1]) == _bits(want[1])
    finally:
        e.close()


def _cli_segments(out):
    rest = out.decode("utf-8", "replace").split("\nResult: ", 1)[1]
    rest = rest[: rest.rindex("RTF: ")]
    hdr = re.compile(r"(?m)^\[(\d\d):(\d\d)\.(\d\d\d) --> (\d\d):(\d\d)\.(\d\d\d)\] ")
    heads = list(hdr.finditer(rest))
    return [(h.group(0), rest[h.end(): heads[j + 1].start() if j + 1 < len(heads) else len(rest)]) for j, h in enumerate(heads)]


def test_cli_suppress_tokens(model):
    """--timestamps --suppress_tokens prints the segments of the decode under the set: those of the run without the flag where that
    one decoded no id of the set, other ones where it did."""
    m, e = model, model.e
    cli = os.path.join(os.path.dirname(m.lib.LIB_PATH), "whisper_cli")
    args = [cli, "-w", os.path.join(GOLDEN, "demo.wav"), "-t", m.case.model_type, "-p", m.case.root, "--language", "zh", "--timestamps"]
    pcm = load_demo_pcm()
    ids0 = e.run_timestamp_tokens_batch([pcm])[0]
    top = [i for i, _ in collections.Counter(i for i in ids0 if i < m.E).most_common(3)]
    plain = subprocess.run(args, capture_output=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    for flag, S in (("-1", NON_SPEECH), (",".join(map(str, top)), top)):
        r = subprocess.run(args + ["--suppress_tokens", flag], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert ("suppress_tokens: %d ids" % len(S)).encode() in r.stdout
        e.set_suppress_tokens(S)
        try:
            ids = e.run_timestamp_tokens_batch([pcm])[0]
        finally:
            e.set_suppress_tokens([])
        assert not set(ids) & set(S)
        want = e.segments(ids, len(pcm))
        got = _cli_segments(r.stdout)
        assert [t[:-1] for _, t in got] == [t for _, _, t in want]
        hit = bool(set(ids0) & set(S))
        assert (ids != ids0) == hit
        assert (got != _cli_segments(plain.stdout)) == (want != e.segments(ids0, len(pcm)))
    assert set(ids0) & set(top)  # the list flag did change the decode
    bad = subprocess.run(args[:-1] + ["--suppress_tokens", "-1"], capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"--suppress_tokens needs --timestamps or --long" in bad.stderr
    bad = subprocess.run(args + ["--suppress_tokens", str(m.E)], capture_output=True, timeout=300)
    assert bad.returncode != 0 and b"eot" in bad.stdout
