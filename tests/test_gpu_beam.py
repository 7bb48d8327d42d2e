"""GPU: beam search (DESIGN.md "Beam search") — the candidates and the selection kernel alone against tests/beam_reference.py, the
loop against the reference on the GPU's own rows at every step, the cache reorder by teacher-forcing every returned record, K = 1
against scored greedy mode, the loop against the CPU oracle, completion on a model that emits eot, and the entry points.

Bars. Candidate ids and their order: exact (both sides compare the same float32 logits), except where rule 5 decides the other way
and the reference's two sides of it are closer than 1e-4 (beam_reference.rule5_near_tie): at most 1 % of the rows, and the reference's
own count of such rows is asserted to be within 1 % too. Log-probabilities: the scored bar 1e-4 + 1e-6 * max(|x[c]|, |logsumexp|).
Selection: exact, bit for bit (float32 adds and comparisons of the caller's numbers). Teacher-forced against traced rows:
2 * err + 1e-4 with err the largest logit difference between the two rows of that step."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import beam_cases
import beam_reference as br
import score_reference as scr
import ts_reference as tsr
from conftest import GOLDEN, ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

MAX_NEW = 12
CANDS = (2, 4, 6, 9)


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
    def __init__(self, built_lib, tmp, model_type, seed, dtype, case=None):
        import oracle

        self.lib = built_lib
        self.case = case or ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=24)
        self.T, self.E, self.nv, self.NS = self.e.timestamp_begin, self.e.eot, self.e.n_vocab, self.e.no_speech
        self.clips = _clips()
        self.mels = [oracle.log_mel(c, self.case.dims["n_mels"])[0] for c in self.clips]
        self._rows = None
        self._traced = {}

    def rows(self):
        """(name, row, history): the 24 rows of test_gpu_sampling.py's recipe (every crafted case, random rows of std 1, 3 and 10 under
        histories of several lengths and rule states), then three rows whose final allowed set holds fewer than M finite entries.
        Built once, never changed."""
        if self._rows is None:
            T, nv = self.T, self.nv
            out = [(name, x, seq) for name, x, seq, _ in tsr.crafted_cases(nv)]
            rng = np.random.default_rng(41)
            hists = [[], [T, 5], [T, 5, 9, 11, 13], [T, 5, T + 30, T + 30], [T, 5, T + 30, T + 30, 8, T + 60], [T + 3, 7, 7, 7, 7, 7, 7, 7, 7]]
            for k in range(24 - len(out)):
                std = (1.0, 3.0, 10.0)[k % 3]
                out.append(("random_std%g_%d" % (std, k), (rng.standard_normal(nv) * std).astype(np.float32), hists[k % len(hists)]))
            x = np.full(nv, -10.0, dtype=np.float32); x[900] = np.inf; x[40] = np.inf
            out[-1] = ("two_plus_inf_lowest_id", x, [T, 5])
            # an open pair at the last timestamp: eot and that timestamp are all that is left
            x = (rng.standard_normal(nv) * 3.0).astype(np.float32); x[50257] = 5.0; x[nv - 1] = 1.0  # (eot above the timestamp: rule 5 stays off)
            out.append(("open_pair_at_30s", x, [T, 5, T + 1500]))
            out.append(("all_nan", np.full(nv, np.nan, dtype=np.float32), [T, 5]))
            x = np.full(nv, -np.inf, dtype=np.float32); x[900] = np.inf; x[40] = np.inf
            out.append(("only_two_plus_inf", x, [T, 5]))
            self._rows = out
        return self._rows

    def traced(self, clips, K, max_new=MAX_NEW):
        """decode_beam(trace=True) over the first `clips` clips, once per configuration -> (results, trace)."""
        key = (clips, K, max_new)
        if key not in self._traced:
            self.e.encode_mel(np.stack(self.mels[:clips]))
            self._traced[key] = self.e.decode_beam(clips, K, max_new, trace=True)
        return self._traced[key]


PARAMS = [("micro", 11, "BF16"), ("miniturbo", 21, "F16")]


@pytest.fixture(scope="module", params=PARAMS, ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("beam_" + request.param[0]), *request.param)
    yield m
    m.e.close()


class Tally:
    def __init__(self):
        self.rows = self.left_out = self.near = 0
        self.worst = 0.0

    def check(self, what):
        print("%s: %d rows, %d rule-5 near ties in the reference, %d left out, max |logprob - ref| = %.3g" %
              (what, self.rows, self.near, self.left_out, self.worst))
        assert self.left_out * 100 <= self.rows and self.near * 100 <= self.rows, (what, self.left_out, self.near, self.rows)


def _check_row(tally, x, seq, T, E, M, gid, glp, gn, what):
    """One row's candidates against the reference: ids and order exact, log-probabilities within the scored bar."""
    ids, lps, info = br.candidates(x, seq, T, E, M)
    near = br.rule5_near_tie(info)
    tally.rows += 1
    tally.near += near
    g = [int(v) for v in gid[:gn]]
    if g != ids:
        flipped, _, _ = br.candidates(x, seq, T, E, M, flip_rule5=True)
        assert near and info["margin"] < 1e-4 and g == flipped, (what, g, ids, info)
        tally.left_out += 1
        return
    for q, c in enumerate(ids):
        assert _close(glp[q], lps[q], _bar(float(x[c]), info["lse_allowed"])), (what, q, c, float(glp[q]), float(lps[q]))
        if math.isfinite(float(lps[q])):
            tally.worst = max(tally.worst, abs(float(glp[q]) - float(lps[q])))
    assert all(int(v) == E for v in gid[gn:]) and all(v == -np.inf for v in glp[gn:]), (what, "padding")


# ---------------------------------------------------------------------------------------------------- 1: the candidates kernel alone
def test_candidates_kernel_on_crafted_and_random_rows(model):
    T, E = model.T, model.E
    rows = model.rows()
    logits = np.stack([r[1] for r in rows])
    hists = [r[2] for r in rows]
    tally = Tally()
    for M in CANDS:
        cid, clp, nc = model.e.beam_candidates(logits, hists, M)
        for b, (name, x, seq) in enumerate(rows):
            _check_row(tally, x, seq, T, E, M, cid[b], clp[b], int(nc[b]), (name, M))
    tally.check("candidates kernel alone")
    by_name = {r[0]: b for b, r in enumerate(rows)}
    cid, clp, nc = model.e.beam_candidates(logits, hists, 9)
    # fewer than M entries in the allowed set
    b = by_name["open_pair_at_30s"]
    assert E == 50257 and nc[b] == 2 and cid[b, :2].tolist() == [E, T + 1500]
    assert nc[by_name["all_nan"]] == 0
    b = by_name["only_two_plus_inf"]
    assert nc[b] == 2 and cid[b, :2].tolist() == [40, 900] and clp[b, :2].tolist() == [0.0, 0.0]
    assert nc[by_name["rule6_all_minus_inf_is_eot"]] == 0
    # a random row under a long history: M entries, strictly ordered
    b = next(i for i, r in enumerate(rows) if r[0].startswith("random_std10"))
    assert nc[b] == 9 and all(logits[b, cid[b, q]] >= logits[b, cid[b, q + 1]] for q in range(8))
    with pytest.raises(RuntimeError):
        model.e.beam_candidates(logits[:1], hists[:1], 10)


# ---------------------------------------------------------------------------------------------------- 2: the selection kernel alone
@pytest.mark.parametrize("case", beam_cases.CASES, ids=[c["name"] for c in beam_cases.CASES])
def test_selection_kernel_on_hand_worked_cases(model, case):
    state, cid, clp, nc = beam_cases.build(case)
    beam_cases.check(case, model.e.beam_select(state, cid, clp, nc, eot=beam_cases.E))


def _random_state(rng):
    K = int(rng.choice([1, 2, 3, 5, 8]))
    clips, n, stride, E = int(rng.integers(1, 4)), int(rng.integers(0, 6)), 8, beam_cases.E
    M, S = K + 1, clips * K
    st = br.initial_state(clips, K, stride, fill=E)
    st["n"] = n
    st["hist"][:, :n] = rng.integers(10, 40, (S, n))
    # scores on a grid of 1/8: ties between candidates of different ranks are common
    st["S"][:] = np.where(rng.random(S) < 0.25, -np.inf, -rng.integers(0, 24, S) / 8.0)
    for c in range(clips):
        st["slot"][c * K:(c + 1) * K] = c * K + rng.permutation(K)
        st["complete"][c] = rng.random() < 0.15
        st["pool_n"][c] = K if st["complete"][c] and rng.random() < 0.5 else rng.integers(0, K)
    st["pool_ids"][:] = rng.integers(10, 40, (S, stride))
    st["pool_len"][:] = rng.integers(0, stride, S)
    st["pool_score"][:] = -rng.integers(0, 64, S) / 8.0
    nc = rng.integers(0, M + 1, S).astype(np.int32)
    cid = rng.integers(0, 14, (S, M)).astype(np.int32)  # (9 is eot: about one candidate in fourteen)
    clp = (-np.sort(rng.integers(0, 16, (S, M)), axis=1) / 8.0).astype(np.float32)
    return st, cid, clp, nc, E


def test_selection_kernel_on_random_states(model):
    rng = np.random.default_rng(2024)
    seen_eot = seen_dead = seen_complete = seen_tie = 0
    for k in range(200):
        st, cid, clp, nc, E = _random_state(rng)
        want = br.select(st, cid, clp, nc, E)
        got = model.e.beam_select(st, cid, clp, nc, eot=E)
        for key in ("S", "slot", "pool_n", "pool_ids", "pool_len", "pool_score", "complete", "tok", "src", "hist", "slot_score"):
            assert np.array_equal(got[key], want[key]), (k, key, got[key], want[key])
        assert got["n_completed"] == want["n_completed"] and got["n"] == want["n"], k
        assert br.check_no_read_and_write(got["src"]), (k, got["src"])
        seen_eot += int((want["pool_n"] > st["pool_n"]).any())
        seen_dead += int((np.isinf(want["S"]) & ~np.isinf(st["S"])).any())
        seen_complete += want["n_completed"]
        seen_tie += int(len(set(want["S"][np.isfinite(want["S"])].tolist())) < int(np.isfinite(want["S"]).sum()))
    # the states reach what they are meant to reach
    assert seen_eot >= 20 and seen_dead >= 10 and seen_complete >= 5 and seen_tie >= 20, (seen_eot, seen_dead, seen_complete, seen_tie)


# ---------------------------------------------------------------------------------------------------- 3: the loop on the GPU's own rows
def _follow(m, results, trace, clips, K, what):
    """The reference walked along the trace: at every step the reference candidates of the dumped rows under the reference's
    histories, and the reference selection fed with the trace's candidates, must be what the trace holds. Returns the final
    reference state and the state before every step."""
    T, E = m.T, m.E
    M, S = K + 1, clips * K
    st = br.initial_state(clips, K, m.e.n_text_ctx, fill=E)
    befores, tally = [], Tally()
    assert trace["n_steps"] >= 1 and trace["rows"].shape == (trace["n_steps"], S, m.nv)
    for n in range(trace["n_steps"]):
        befores.append(br._copy(st))
        rank_of = {int(st["slot"][i]): i for i in range(S)}
        for s in range(S):
            gn = int(trace["n_cand"][n, s])
            if st["complete"][s // K] or st["S"][rank_of[s]] == -np.inf:
                assert gn == 0, (what, n, s, "a dead or frozen slot proposed")
                continue
            _check_row(tally, trace["rows"][n, s], st["hist"][s, :n].tolist(), T, E, M, trace["cand_id"][n, s], trace["cand_logprob"][n, s], gn, (what, n, s))
        new = br.select(st, trace["cand_id"][n], trace["cand_logprob"][n], trace["n_cand"][n], E)
        for key in ("S", "slot", "src", "tok", "pool_n"):
            assert np.array_equal(new[key], trace[key][n]), (what, n, key, new[key], trace[key][n])
        assert br.check_no_read_and_write(trace["src"][n]), (what, n, trace["src"][n])
        for c in range(clips):
            assert sorted(trace["slot"][n, c * K:(c + 1) * K].tolist()) == list(range(c * K, (c + 1) * K)), (what, n, c)
        st = br.apply_reorder(new, new["src"])
    tally.check(what)
    # what the call returned is the reference finalisation of that state: histories and pool came back from the device
    for c, (w, g) in enumerate(zip(br.finalize(st), results)):
        assert g["ids"] == w["ids"] and g["winner"] == w["winner"] and g["ended_eot"] == w["ended_eot"], (what, c, g["ids"], w["ids"])
        assert g["sum_logprob"] == w["sum_logprob"] and g["avg_logprob"] == w["avg_logprob"], (what, c)
        assert [(i, float(s), p) for i, s, p in g["records"]] == [(i, float(s), p) for i, s, p in w["records"]], (what, c)
    return st, befores


CONFIGS = [(1, 2), (2, 5), (3, 8)]  # GEMV family (2 slots), one-branch clip-block step (10), multi-branch step (24)


@pytest.mark.parametrize("clips,K", CONFIGS, ids=["1x2_gemv", "2x5_cblock", "3x8_branches"])
def test_loop_follows_the_reference_on_its_own_rows(model, clips, K):
    results, trace = model.traced(clips, K)
    assert trace["n_steps"] == MAX_NEW  # (seeded weights do not emit eot early: the budget ends the loop)
    st, _ = _follow(model, results, trace, clips, K, "loop %d x %d" % (clips, K))
    assert all(len(r["ids"]) == MAX_NEW and not r["ended_eot"] for r in results)
    if K > 1:  # hypotheses did change slots
        assert any((trace["src"][n] != np.arange(clips * K)).any() for n in range(1, MAX_NEW))


# ---------------------------------------------------------------------------------------------------- 4: the cache reorder
# Two correct evaluations of one step differ by summation order and kernel family only: the largest such error this suite has
# measured between engine and oracle on these models is 4.1e-4 (DESIGN.md "Confidence": largest bound 2 err + 1e-4 = 9.2e-4). One wrong key in a self-attention cache
# moves these models' logits by 0.1 (measured with the oracle: the same ids with one id two steps back replaced). 5e-3 sits an order
# of magnitude from either.
ERR_MAX = 5e-3


def _lineage(trace, befores, st, c, K, ids, pooled, E):
    """[(step, slot the hypothesis sat in before that step, id chosen at it)] of one record, first step first."""
    path = []
    if pooled:
        L = len(ids)
        rank_of = {int(befores[L]["slot"][i]): i for i in range(len(befores[L]["S"]))}
        cands = [s for s in range(c * K, (c + 1) * K) if befores[L]["hist"][s, :L].tolist() == ids and befores[L]["S"][rank_of[s]] > -np.inf
                 and E in trace["cand_id"][L, s, : trace["n_cand"][L, s]].tolist()]
        assert cands, ("no parent proposed eot for the record", c, ids)
        path.append((L, cands[0], E))
        cur, last = cands[0], L - 1
    else:
        L = len(ids)
        cur = next(int(st["slot"][r]) for r in range(c * K, (c + 1) * K) if st["S"][r] > -np.inf and st["hist"][st["slot"][r], :L].tolist() == ids)
        last = L - 1
    for n in range(last, -1, -1):
        parent = int(trace["src"][n, cur])
        path.append((n, parent, int(trace["tok"][n, cur])))
        cur = parent
    return path[::-1]


def _check_reorder(m, clips, K, max_new, what):
    T, E = m.T, m.E
    results, trace = m.traced(clips, K, max_new)
    st, befores = _follow(m, results, trace, clips, K, what)
    n_rec = max(len(r["records"]) for r in results)
    worst_err = worst = 0.0
    for i in range(n_rec):
        recs = [r["records"][i] if i < len(r["records"]) else ([], 0.0, False) for r in results]
        L = max(len(ids) for ids, _, _ in recs)
        f = np.full((clips, max(L, 1)), E, dtype=np.int32)
        for c, (ids, _, _) in enumerate(recs):
            f[c, : len(ids)] = ids
        m.e.encode_mel(np.stack(m.mels[:clips]))  # (the beam call spread its cross K/V over the slots)
        logits, _, _, _, _ = m.e.decode_forced_timestamp_scores(clips, f, want_logits0=False)
        for c, (ids, score, pooled) in enumerate(recs):
            if i >= len(results[c]["records"]):
                continue
            path = _lineage(trace, befores, st, c, K, ids, pooled, E)
            assert [t for _, _, t in path][: len(ids)] == ids, (what, c, i)
            total = np.float32(0.0)
            for j, (n, slot, tok) in enumerate(path):
                assert n == j
                q = trace["cand_id"][n, slot, : trace["n_cand"][n, slot]].tolist().index(tok)
                lp_trace = trace["cand_logprob"][n, slot, q]
                total = np.float32(total + lp_trace)
                row_t, row_f = trace["rows"][n, slot], logits[c, j]
                err = float(np.abs(row_t - row_f).max())
                assert err <= ERR_MAX, (what, c, i, j, "the row of the beam's slot is not the row of the same ids teacher-forced", err)
                worst_err = max(worst_err, err)
                lp_ref, info = br.token_logprob(row_f, ids[:j], T, E, tok)
                if br.token_logprob(row_t, ids[:j], T, E, tok)[1]["rule5"] != info["rule5"]:
                    assert abs(info["lse"] - info["max_text"]) < 2 * err + 1e-4, (what, c, i, j, info)
                    continue
                assert _close(lp_trace, lp_ref, 2 * err + 1e-4), (what, c, i, j, float(lp_trace), float(lp_ref), err)
                worst = max(worst, abs(float(lp_trace) - float(lp_ref)))
            assert total == np.float32(score), (what, c, i, float(total), float(score))  # the record's score is the float32 sum along its path
    print("%s: %d records per clip teacher-forced, max logit err %.3g, max |logprob - ref| %.3g" % (what, n_rec, worst_err, worst))
    return trace


@pytest.mark.parametrize("clips,K", CONFIGS, ids=["1x2_gemv", "2x5_cblock", "3x8_branches"])
def test_reordered_caches_are_the_records_caches(model, clips, K):
    _check_reorder(model, clips, K, MAX_NEW, "reorder %d x %d" % (clips, K))


def test_reorder_across_the_64_key_block_edge(model):
    trace = _check_reorder(model, 1, 3, 70, "reorder 1 x 3, 70 ids")
    assert trace["n_steps"] == 70
    moved = [n for n in range(70) if (trace["src"][n] != np.arange(3)).any()]
    assert any(n + 2 > 64 for n in moved), moved  # decode offset = n + 2: a copy of two blocks per (layer, head)


# ---------------------------------------------------------------------------------------------------- 5: K = 1 is scored greedy mode
@pytest.mark.parametrize("batch", [1, 4, 24])
def test_beam_of_one_is_scored_greedy_mode(model, batch):
    nc = len(model.clips)
    clips = [model.clips[b % nc] for b in range(batch)]
    got = model.e.run_beam_batch(clips, 1, MAX_NEW)
    want = model.e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["ids"] == w["ids"] and g["ended_eot"] == w["ended_eot"], (batch, b)
        total = float(np.sum(w["token_logprob"][: len(w["ids"])], dtype=np.float64)) + (float(w["token_logprob"][len(w["ids"])]) if w["ended_eot"] else 0.0)
        # one scored bar per summed term
        assert _close(g["sum_logprob"], total, (len(w["ids"]) + 1) * _bar(total, 0.0)), (batch, b, g["sum_logprob"], total)
        assert _close(g["avg_logprob"], w["avg_logprob"], _bar(total, 0.0)), (batch, b, g["avg_logprob"], w["avg_logprob"])
        assert _close(g["no_speech_logprob"], w["no_speech_logprob"], _bar(w["no_speech_logprob"], 0.0)), (batch, b)


# ---------------------------------------------------------------------------------------------------- 6: against the CPU oracle
def test_loop_against_the_oracle(built_lib, oracle_mod, tmp_path_factory):
    """micro, seed 11 (of seeds 1 .. 40 the one whose oracle run keeps the largest boundary gaps: 0.0098 at the least, a step's
    gap over its step number 1.0e-3 at the least), the first two clips, K = 3, 12 ids."""
    m = Model(built_lib, tmp_path_factory.mktemp("beam_orc"), "micro", 11, "BF16")
    try:
        K, clips = 3, 2
        T, E = m.T, m.E
        orc = m.case.oracle_bf16
        prefix = orc.sot_seq("zh")[:3]
        kvs = [orc.encoder(mel) for mel in m.mels[:clips]]
        want, wst, log = br.oracle_beam(orc, kvs, prefix, K, MAX_NEW, T, E)
        gaps = [min(e["gap"]) for e in log]
        print("oracle beam: smallest boundary gap per step", ["%.3g" % g for g in gaps])
        results, trace = m.traced(clips, K)
        # err_i: the engine teacher-forced with the oracle's own hypotheses (the K final ones of every clip), against the oracle's rows
        errs = np.zeros(MAX_NEW)
        for r in range(K):
            f = np.stack([wst["hist"][wst["slot"][c * K + r], :MAX_NEW] for c in range(clips)]).astype(np.int32)
            m.e.encode_mel(np.stack(m.mels[:clips]))
            logits, _, _, _, _ = m.e.decode_forced_timestamp_scores(clips, f, want_logits0=False)
            for c in range(clips):
                _, rows = scr.oracle_rows(orc, *kvs[c], prefix, f[c].tolist())
                errs = np.maximum(errs, np.abs(logits[c, :MAX_NEW] - rows[:MAX_NEW]).max(axis=1))
        bound = np.cumsum(2 * errs + 1e-4)
        print("accumulated bound per step", ["%.3g" % b for b in bound], "gap / (2 bound)", ["%.3g" % (g / (2 * b)) for g, b in zip(gaps, bound)])
        # the inputs were picked so that no step of the oracle's run is a numerical tie: the tie escape below must stay unused
        assert all(g > 2 * b for g, b in zip(gaps, bound)), ("a step of the oracle's beam is within twice the accumulated bound", gaps, bound.tolist())
        # the selected (parent, id) sets, as the sets of histories after every step
        st, diverged = br.initial_state(clips, K, m.e.n_text_ctx, fill=E), None
        for n in range(trace["n_steps"]):
            st = br.apply_reorder(br.select(st, trace["cand_id"][n], trace["cand_logprob"][n], trace["n_cand"][n], E), trace["src"][n])
            ost = log[n]["state"]
            for c in range(clips):
                live = lambda s_: {tuple(s_["hist"][s_["slot"][r], : n + 1].tolist()) for r in range(c * K, (c + 1) * K) if s_["S"][r] > -np.inf}
                if live(st) != live(ost):
                    diverged = (n, c)
                    break
            if diverged:
                break
        # (a first divergence would be acceptable only below twice the accumulated bound; with every gap above it, none is)
        assert diverged is None, ("the engine's beam left the oracle's", diverged, log[diverged[0]]["gap"][diverged[1]], bound[diverged[0]])
        for c in range(clips):
            assert results[c]["ids"] == want[c]["ids"], (c, results[c]["ids"], want[c]["ids"])
            assert abs(float(results[c]["sum_logprob"]) - float(want[c]["sum_logprob"])) <= bound[-1], c
    finally:
        m.e.close()


# ---------------------------------------------------------------------------------------------------- 7: completion
EOT_TWIN, EOT_GAIN = 46781, 1.0  # the eot row of the tied embedding gets this multiple of a text row the micro model chooses often


def test_every_clip_completes_before_the_budget(built_lib, oracle_mod, tmp_path_factory):
    import modelgen
    import oracle
    import torch

    tmp = tmp_path_factory.mktemp("beam_eot")
    case = types.SimpleNamespace(model_type="micro", root=str(tmp), dims=modelgen.DIMS["micro"])
    w = dict(modelgen.synth_weights(case.dims, 11))
    emb = w["decoder.token_embedding.weight"].copy()
    E = int(modelgen.make_config("micro", case.dims)["eot"])
    mixed = emb[E] + np.float32(EOT_GAIN) * emb[EOT_TWIN]
    emb[E] = torch.from_numpy(mixed).to(torch.bfloat16).to(torch.float32).numpy()  # (still bfloat16 values: both sides hold the same weights)
    w["decoder.token_embedding.weight"] = emb
    case.weights, case.cfg = w, modelgen.make_config("micro", case.dims)
    modelgen.write_model_dir(case.root, "micro", case.dims, weights=w, dtype="BF16", tiktoken_path=os.path.join(os.path.dirname(__file__), "golden", "multilingual.tiktoken"))
    case.oracle_bf16 = oracle.Oracle(case.cfg, w, bf16_policy=True)
    m = Model(built_lib, tmp, "micro", 11, "BF16", case=case)
    try:
        K, clips, budget = 3, 2, 40
        orc = case.oracle_bf16
        kvs = [orc.encoder(mel) for mel in m.mels[:clips]]
        want, wst, log = br.oracle_beam(orc, kvs, orc.sot_seq("zh")[:3], K, budget, m.T, m.E)
        print("oracle beam on the eot model: %d steps, pools %s, winners %s" % (len(log), wst["pool_n"].tolist(), [(len(o["ids"]), o["ended_eot"]) for o in want]))
        assert len(log) < budget - 16 and wst["complete"].all() and (wst["pool_n"] == K).all()
        results, trace = m.traced(clips, K, budget)
        # the loop ended because every clip completed: fewer steps than the budget, every pool full, and the steps past the last
        # completion (the counter is polled every 8 steps, two deep) changed nothing
        assert trace["n_steps"] < budget, trace["n_steps"]
        assert (trace["pool_n"][-1] == K).all()
        done_at = max(int(np.argmax(trace["pool_n"][:, c] == K)) for c in range(clips))
        assert trace["n_steps"] - (done_at + 1) <= 16
        for n in range(done_at + 1, trace["n_steps"]):
            assert (trace["n_cand"][n] == 0).all() and np.array_equal(trace["S"][n], trace["S"][done_at]) and np.array_equal(trace["slot"][n], trace["slot"][done_at])
            assert np.array_equal(trace["src"][n], np.arange(clips * K))
        _follow(m, results, trace, clips, K, "completion")  # (the returned winner is the reference finalisation of the trace)
        assert all(r["ended_eot"] and len(r["records"]) == K and all(p for _, _, p in r["records"]) for r in results)
        assert all(len(r["ids"]) < budget for r in results)
        # the same call without a trace, and through the whole pipeline's encoder on the same mel-exact clips
        m.e.encode_mel(np.stack(m.mels[:clips]))
        again, none = m.e.decode_beam(clips, K, budget)
        assert none is None and [r["ids"] for r in again] == [r["ids"] for r in results]
    finally:
        m.e.close()


# ---------------------------------------------------------------------------------------------------- 8: entry points
def test_run_beam_batch_is_decode_beam_after_encode_mel(model):
    K, clips = 3, 2
    # the whole pipeline on the clips' own front-end: compare with the stage-level call on the engine's own mels
    mels = np.stack([model.e.compute_mel(c) for c in model.clips[:clips]])
    model.e.encode_mel(mels)
    staged, _ = model.e.decode_beam(clips, K, MAX_NEW)
    whole = model.e.run_beam_batch(model.clips[:clips], K, MAX_NEW)
    for s, w in zip(staged, whole):
        assert s["ids"] == w["ids"] and s["ended_eot"] == w["ended_eot"]
        assert _close(s["sum_logprob"], w["sum_logprob"], (MAX_NEW + 1) * _bar(float(w["sum_logprob"]), 0.0))
        assert _close(s["avg_logprob"], w["avg_logprob"], _bar(float(w["sum_logprob"]), 0.0))
        assert _close(s["no_speech_logprob"], w["no_speech_logprob"], _bar(float(w["no_speech_logprob"]), 0.0))
    # two clips alone and side by side
    for c in range(clips):
        alone = model.e.run_beam_batch([model.clips[c]], K, MAX_NEW)[0]
        assert alone["ids"] == whole[c]["ids"], c
        assert _close(alone["sum_logprob"], whole[c]["sum_logprob"], (MAX_NEW + 1) * _bar(float(whole[c]["sum_logprob"]), 0.0)), c
    assert model.e.timings()["steps"] == MAX_NEW + 2


def test_slots_beyond_the_capacity_are_refused(model):
    with pytest.raises(RuntimeError, match=r"beam search needs 32 slots \(4 clips x beam_size 8\), the engine holds 24"):
        model.e.run_beam_batch(model.clips[:4], 8, MAX_NEW)
    model.e.encode_mel(np.stack(model.mels[:4]))
    with pytest.raises(RuntimeError, match=r"beam search needs 28 slots \(4 clips x beam_size 7\), the engine holds 24"):
        model.e.decode_beam(4, 7, MAX_NEW)
    for bad in (0, 9):
        with pytest.raises(RuntimeError, match="beam_size"):
            model.e.run_beam_batch(model.clips[:1], bad, MAX_NEW)
    # the engine still works
    assert len(model.e.run_beam_batch(model.clips[:1], 2, 4)[0]["ids"]) == 4
    segs = model.e.run_timestamps(model.clips[0], max_new=MAX_NEW, beam_size=3)
    ids = model.e.run_beam_batch([model.clips[0]], 3, MAX_NEW)[0]["ids"]
    assert segs == model.e.segments(ids, len(model.clips[0]))
    assert model.e.run_timestamps(model.clips[0], max_new=MAX_NEW) == model.e.segments(model.e.run_timestamp_tokens_batch([model.clips[0]], MAX_NEW)[0], len(model.clips[0]))


def test_cli_beam_size(model):
    """--timestamps --beam_size 3 prints the segments of the winner; the flag alone, or with --long, is refused."""
    m = model
    cli = os.path.join(os.path.dirname(m.lib.LIB_PATH), "whisper_cli")
    wav = os.path.join(GOLDEN, "demo.wav")
    args = [cli, "-w", wav, "-t", m.case.model_type, "-p", m.case.root, "--language", "zh"]
    r = subprocess.run(args + ["--timestamps", "--beam_size", "3"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rest = r.stdout.decode("utf-8", "replace").split("\nResult: ", 1)[1]
    rest = rest[: rest.rindex("RTF: ")]
    hdr = re.compile(r"(?m)^\[(\d\d):(\d\d)\.(\d\d\d) --> (\d\d):(\d\d)\.(\d\d\d)\] ")
    heads = list(hdr.finditer(rest))
    parsed = []
    for j, h in enumerate(heads):
        g = h.groups()
        text = rest[h.end(): heads[j + 1].start() if j + 1 < len(heads) else len(rest)]
        assert text.endswith("\n")
        parsed.append((int(g[0]) * 60 + int(g[1]) + int(g[2]) / 1000, int(g[3]) * 60 + int(g[4]) + int(g[5]) / 1000, text[:-1]))
    pcm = load_demo_pcm()
    ids = m.e.run_beam_batch([pcm], 3)[0]["ids"]
    want = m.e.segments(ids, len(pcm))
    assert len(parsed) == len(want) and len(want) >= 1
    for (s, e, t), (ws, we, wt) in zip(parsed, want):
        assert abs(s - ws) < 6e-4 and abs(e - we) < 6e-4 and t == wt
    for flags in (["--beam_size", "3"], ["--beam_size", "3", "--long"], ["--timestamps", "--long", "--beam_size", "3"]):
        bad = subprocess.run(args + flags, capture_output=True, timeout=60)
        assert bad.returncode != 0 and b"--beam_size needs --timestamps" in bad.stderr and b"usage:" in bad.stderr, flags
    bad = subprocess.run(args + ["--timestamps", "--beam_size", "9"], capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"bad value: --beam_size" in bad.stderr
