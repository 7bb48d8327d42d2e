"""No GPU: the beam-search contract (DESIGN.md "Beam search") as tests/beam_reference.py states it — against exhaustive search on a
toy model, on hand-worked selection steps (tests/beam_cases.py), the finalisation; the resources of the kernels in decode_beam.hip;
the new C ABI symbols, their null-argument behaviour and the host-only AX_WHISPER_BeamFinalize against the reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_cases
import beam_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["AX_WHISPER_RunPCMBatchBeam", "AX_WHISPER_DecodeBeam", "AX_WHISPER_BeamCandidates", "AX_WHISPER_BeamSelect", "AX_WHISPER_BeamFinalize"]


# ------------------------------------------------------------------------------------------------ exhaustive search
NV, EOT, DEPTH = 6, 5, 4  # ids 0 .. 4 are text, 5 is eot; every id is allowed at every step


class Toy:
    """A table of next-token logits: one seeded row per history."""

    def __init__(self, seed):
        self.seed, self.rows = seed, {}

    def row(self, hist):
        key = tuple(hist)
        if key not in self.rows:
            rng = np.random.default_rng([self.seed] + [t + 1 for t in key])
            self.rows[key] = (rng.standard_normal(NV) * 2.0).astype(np.float32)
        return self.rows[key]


def _toy_logprobs(row):
    ids, lps, _ = br.candidates(row, [], NV, EOT, NV, allowed=np.ones(NV, dtype=bool))
    return dict(zip(ids, lps))


def _exhaustive(toy):
    """Every record a beam wide enough would hold -> (ids, float32 score): sequences ended by eot at any depth (the eot term in
    the score), and the DEPTH-long ones cut at the budget (no eot term). Scores are accumulated in float32, as the contract does."""
    recs = []

    def walk(hist, score):
        if len(hist) == DEPTH:
            recs.append((list(hist), score))
            return
        lp = _toy_logprobs(toy.row(hist))
        recs.append((list(hist), np.float32(score + lp[EOT])))
        for t in range(EOT):
            walk(hist + [t], np.float32(score + lp[t]))

    walk([], np.float32(0.0))
    return recs


def _toy_search(toy, K):
    rows_fn = lambda n, st: [toy.row(st["hist"][s, :n].tolist()) for s in range(K)]
    return br.beam_search(1, K, DEPTH, DEPTH + 1, NV, EOT, rows_fn, allowed=np.ones(NV, dtype=bool))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_wide_beam_is_exhaustive_search(seed):
    toy = Toy(seed)
    recs = _exhaustive(toy)
    assert len(recs) == sum(5 ** d for d in range(DEPTH)) + 5 ** DEPTH
    # live hypotheses never exceed 5^3 before the last step; K covers them and every record: pool 156 + 625 live ranks
    K = len(recs)
    out, st, _ = _toy_search(toy, K)
    key = lambda ids, sc: float(sc) / max(len(ids), 1)
    best = max(recs, key=lambda r: key(*r))
    w = out[0]
    assert sorted((tuple(i), float(s)) for i, s, _ in w["records"]) == sorted((tuple(i), float(s)) for i, s in recs)
    assert w["ids"] == best[0] and w["sum_logprob"] == best[1]
    assert key(w["ids"], w["sum_logprob"]) == max(key(*r) for r in recs)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_beam_of_one_is_greedy(seed):
    toy = Toy(seed)
    hist, score, eot = [], np.float32(0.0), False
    while len(hist) < DEPTH:
        lp = _toy_logprobs(toy.row(hist))
        t = max(range(NV), key=lambda i: (lp[i], -i))
        score = np.float32(score + lp[t])
        if t == EOT:
            eot = True
            break
        hist.append(t)
    out, _, _ = _toy_search(toy, 1)
    assert out[0]["ids"] == hist and out[0]["sum_logprob"] == score and out[0]["ended_eot"] == eot
    assert out[0]["avg_logprob"] == np.float32(float(score) / (len(hist) + 1))


def test_candidates_follow_the_scored_allowed_set():
    """Under the timestamp rules: the candidates are the best ids of score_reference.final_allowed, -inf and NaN left out, lower id
    first on ties, and the first candidate is scored mode's decision with its log-probability."""
    import score_reference as scr
    import ts_reference as tsr

    nv = 51865
    for name, x, seq, want in tsr.crafted_cases(nv):
        T, E = 50364, 50257
        ids, lps, info = br.candidates(x, seq, T, E, 4)
        A = scr.final_allowed(x, seq, T, E) & (np.asarray(x, dtype=np.float64) > -np.inf)
        assert len(ids) == min(4, int(A.sum())), name
        assert all(A[c] for c in ids), name
        vals = [float(x[c]) for c in ids]
        assert all(a > b or (a == b and i < j) for a, b, i, j in zip(vals, vals[1:], ids, ids[1:])), name
        if ids:
            c, lp, _ = scr.token_logprob(x, seq, T, E)
            assert ids[0] == c == want and lps[0] == lp, name
            rest = np.flatnonzero(A & ~np.isin(np.arange(nv), ids))
            assert rest.size == 0 or float(np.asarray(x)[rest].max()) <= vals[-1], name
        else:
            assert want == E, name


# ------------------------------------------------------------------------------------------------ hand-worked selection steps
@pytest.mark.parametrize("case", beam_cases.CASES, ids=[c["name"] for c in beam_cases.CASES])
def test_selection_case(case):
    state, cid, clp, nc = beam_cases.build(case)
    beam_cases.check(case, br.select(state, cid, clp, nc, beam_cases.E))


def test_complete_clip_is_frozen():
    case = next(c for c in beam_cases.CASES if c["name"] == "pool_fills_to_K_and_the_clip_completes")
    state, cid, clp, nc = beam_cases.build(case)
    st = br.select(state, cid, clp, nc, beam_cases.E)
    assert st["complete"][0] == 1
    br.apply_reorder(st, st["src"])
    again = br.select(st, cid, clp, nc, beam_cases.E)  # the same attractive candidates: nothing of the clip may change
    for k in ("hist", "S", "slot", "pool_n", "pool_ids", "pool_len", "pool_score", "complete"):
        assert np.array_equal(again[k], st[k]), k
    assert again["src"].tolist() == [0, 1] and again["n_completed"] == 0


def test_two_clips_do_not_mix():
    """Clip 1's slots start at K: the same step beside another clip gives the same result, shifted."""
    a = next(c for c in beam_cases.CASES if c["name"] == "equal_scores_go_by_parent_rank_then_position")
    b = next(c for c in beam_cases.CASES if c["name"] == "fewer_than_K_candidates_leave_dead_ranks")
    (sa, ca, la, na), (sb, cb, lb, nb) = beam_cases.build(a), beam_cases.build(b)
    K = 3
    both = {k: np.concatenate([sa[k], sb[k] + (K if k == "slot" else 0)]) for k in sa if isinstance(sa[k], np.ndarray)}
    both.update(K=K, n=2)
    st = br.select(both, np.concatenate([ca, cb]), np.concatenate([la, lb]), np.concatenate([na, nb]), beam_cases.E)
    one_a, one_b = br.select(sa, ca, la, na, beam_cases.E), br.select(sb, cb, lb, nb, beam_cases.E)
    assert st["S"].tolist() == one_a["S"].tolist() + one_b["S"].tolist()
    assert st["slot"].tolist() == one_a["slot"].tolist() + (one_b["slot"] + K).tolist()
    assert st["src"].tolist() == one_a["src"].tolist() + (one_b["src"] + K).tolist()
    assert st["tok"].tolist() == one_a["tok"].tolist() + one_b["tok"].tolist()
    assert st["pool_n"].tolist() == [0, 1] and st["n_completed"] == 0


# ------------------------------------------------------------------------------------------------ finalise
def _final_state(K, n, S, slot, pool):
    st = br.initial_state(1, K, 8, fill=beam_cases.E)
    st["n"] = n
    st["S"][:] = S
    st["slot"][:] = slot
    for s in range(K):
        st["hist"][s, :n] = beam_cases.hist_of(s, n)
    for i, (ids, sc) in enumerate(pool):
        st["pool_ids"][i, : len(ids)] = ids
        st["pool_len"][i] = len(ids)
        st["pool_score"][i] = sc
    st["pool_n"][0] = len(pool)
    return st


FINAL_CASES = [
    # (name, K, n, S by rank, slot by rank, pool, expected records [(ids, score, from_pool)], winner, avg_logprob)
    ("fill_from_live_ranks_in_rank_order", 3, 2, [-1.0, -np.inf, -4.0], [2, 0, 1], [([7], -3.0)],
     [([7], -3.0, True), (beam_cases.hist_of(2, 2), -1.0, False), (beam_cases.hist_of(1, 2), -4.0, False)], 1, -1.0 / 3),
    ("a_full_pool_takes_no_live_rank", 2, 3, [-0.5, -0.75], [0, 1], [([1, 2], -4.0), ([3], -3.0)],
     [([1, 2], -4.0, True), ([3], -3.0, True)], 0, -4.0 / 3),
    ("first_maximum_wins", 3, 2, [-2.0, -2.0, -6.0], [0, 1, 2], [],
     [(beam_cases.hist_of(0, 2), -2.0, False), (beam_cases.hist_of(1, 2), -2.0, False), (beam_cases.hist_of(2, 2), -6.0, False)], 0, -2.0 / 3),
    ("an_empty_record_divides_by_one", 2, 2, [-5.0, -np.inf], [0, 1], [([], -1.5)],
     [([], -1.5, True), (beam_cases.hist_of(0, 2), -5.0, False)], 0, -1.5),
    ("no_record_at_all", 2, 2, [-np.inf, -np.inf], [0, 1], [], [], -1, -np.inf),
]


@pytest.mark.parametrize("case", FINAL_CASES, ids=[c[0] for c in FINAL_CASES])
def test_finalize(case, built_lib):
    name, K, n, S, slot, pool, recs, winner, avg = case
    st = _final_state(K, n, S, slot, pool)
    for who, out in (("reference", br.finalize(st)[0]),
                     ("library", built_lib.beam_finalize(st["hist"], st["S"], st["slot"], st["pool_n"], st["pool_ids"], st["pool_len"], st["pool_score"], n)[0])):
        assert [(i, float(s), p) for i, s, p in out["records"]] == [(i, float(np.float32(s)), p) for i, s, p in recs], who
        assert out["winner"] == winner, who
        if winner < 0:
            assert out["ids"] == [] and out["sum_logprob"] == -np.inf and out["avg_logprob"] == -np.inf and not out["ended_eot"], who
        else:
            assert out["ids"] == recs[winner][0] and out["sum_logprob"] == np.float32(recs[winner][1]) and out["ended_eot"] == recs[winner][2], who
            assert out["avg_logprob"] == np.float32(avg), who


def test_finalize_binding_matches_reference_on_random_states(built_lib):
    rng = np.random.default_rng(5)
    for _ in range(100):
        clips, K, n = int(rng.integers(1, 4)), int(rng.integers(1, 9)), int(rng.integers(0, 7))
        st = br.initial_state(clips, K, 8, fill=3)
        st["n"] = n
        st["hist"][:] = rng.integers(0, 50, st["hist"].shape)
        st["pool_ids"][:] = rng.integers(0, 50, st["pool_ids"].shape)
        st["S"][:] = np.where(rng.random(clips * K) < 0.3, -np.inf, -rng.integers(0, 40, clips * K) / 4.0)
        st["pool_score"][:] = -rng.integers(0, 40, clips * K) / 4.0
        st["pool_len"][:] = rng.integers(0, 8, clips * K)
        st["pool_n"][:] = rng.integers(0, K + 1, clips)
        for c in range(clips):
            st["slot"][c * K:(c + 1) * K] = c * K + rng.permutation(K)
        want = br.finalize(st)
        got = built_lib.beam_finalize(st["hist"], st["S"], st["slot"], st["pool_n"], st["pool_ids"], st["pool_len"], st["pool_score"], n)
        for w, g in zip(want, got):
            assert g["ids"] == w["ids"] and g["winner"] == w["winner"] and g["ended_eot"] == w["ended_eot"]
            assert g["sum_logprob"] == w["sum_logprob"] and g["avg_logprob"] == w["avg_logprob"]
            assert [(i, float(s), p) for i, s, p in g["records"]] == [(i, float(s), p) for i, s, p in w["records"]]


# ------------------------------------------------------------------------------------------------ kernel resources
# vgpr_count rounded up to a multiple of 8 (DESIGN.md "Beam search" carries the same table)
KERNEL_VGPRS = {"beam_candidates_kernel": 64, "beam_select_kernel": 32, "beam_reorder_kernel": 16, "beam_spread_cross_kernel": 16}


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_beam_kernel_resources(f16, tmp_path):
    out = tmp_path / "beam.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out),
                        os.path.join(ROOT, "whisper.axera_amd", "csrc", "decode_beam.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    field = lambda f: [int(x) for x in re.findall(r"^\s+\.%s:\s+(\d+)" % f, text, re.M)]
    for kernel, vgprs in KERNEL_VGPRS.items():
        assert sum(kernel in n for n in names) == 1, (kernel, names)
        k = next(i for i, n in enumerate(names) if kernel in n)
        # a dynamically indexed register array would show here as scratch
        assert field("private_segment_fixed_size")[k] == 0, kernel
        assert field("vgpr_spill_count")[k] == 0 and field("sgpr_spill_count")[k] == 0, kernel
        assert (field("vgpr_count")[k] + 7) // 8 * 8 == vgprs, (kernel, field("vgpr_count")[k])
    assert len(names) == len(KERNEL_VGPRS), names


# ------------------------------------------------------------------------------------------------ bindings
def test_new_symbols_are_exported_and_bound(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    assert set(NEW_SYMBOLS) <= set(built_lib.SYMBOLS)
    for m in ("run_beam_batch", "decode_beam", "beam_candidates", "beam_select", "beam_finalize", "run_timestamps"):
        assert callable(getattr(built_lib.Whisper, m))
    assert callable(built_lib.beam_finalize)
    import inspect

    assert inspect.signature(built_lib.Whisper.run_timestamps).parameters["beam_size"].default == 1
    assert inspect.signature(built_lib.Whisper.run_beam_batch).parameters["beam_size"].default == 5


def test_beam_calls_reject_null_arguments(built_lib):
    L = built_lib.load_library()
    n = C.c_int()
    z = [None] * 32
    assert L.AX_WHISPER_RunPCMBatchBeam(None, None, None, 1, 5, 0, *z[:6]) == -1
    assert L.AX_WHISPER_DecodeBeam(None, 1, 5, 0, *z[:12], 0, *z[:9], C.byref(n)) == -1
    assert L.AX_WHISPER_BeamCandidates(None, None, None, None, 1, 6, None, None, None) == -1
    assert L.AX_WHISPER_BeamSelect(None, 1, 5, 9, 0, 8, *z[:14], C.byref(n)) == -1
    assert L.AX_WHISPER_BeamFinalize(1, 5, 0, 8, *z[:18]) == -1
    # host only: bad sizes are refused, not read
    one_i, one_f = (C.c_int32 * 8)(), (C.c_float * 8)()
    ints = C.cast(one_i, C.POINTER(C.c_int))
    assert L.AX_WHISPER_BeamFinalize(1, 9, 0, 8, one_i, one_f, ints, ints, one_i, ints, one_f, *z[:11]) == -1   # beam_size above 8
    assert L.AX_WHISPER_BeamFinalize(1, 2, 9, 8, one_i, one_f, ints, ints, one_i, ints, one_f, *z[:11]) == -1   # n above the stride
    bad_slot = (C.c_int * 2)(0, 7)
    assert L.AX_WHISPER_BeamFinalize(1, 2, 1, 8, one_i, one_f, bad_slot, ints, one_i, ints, one_f, *z[:11]) == -1
