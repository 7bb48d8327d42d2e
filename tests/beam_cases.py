"""Hand-worked selection steps of beam search (DESIGN.md "Beam search"), each with its expected outcome written out. The CPU suite
runs them through tests/beam_reference.py, the GPU suite through beam_select_kernel: both must give exactly `expect`.

A case: K, n (history length before the step), S and slot by rank, cands {rank: [(id, logprob), ...]} (what the rank's slot
proposes), optional pool [(ids, score)] and complete; expect: S and slot by rank, tok and src by slot, pool [(ids, score)], complete.
All numbers are exact in float32. eot is E; history of slot s is [100 + 10 s + i]."""
import numpy as np

E = 9
STRIDE = 8
INF = float("inf")


def hist_of(s, n):
    return [100 + 10 * s + i for i in range(n)]


CASES = [
    dict(name="eot_ranked_first", K=2, n=2, S=[0.0, -1.0], slot=[0, 1],
         cands={0: [(E, -0.25), (3, -1.5), (4, -3.0)], 1: [(5, -0.5), (6, -1.0), (E, -4.0)]},
         # order: eot(-0.25, r0), 3(-1.5, r0), 5(-1.5, r1) -> stop. eot is recorded with the parent's history.
         expect=dict(S=[-1.5, -1.5], slot=[0, 1], tok=[3, 5], src=[0, 1], pool=[(hist_of(0, 2), -0.25)], complete=0)),
    dict(name="eot_after_the_kth_is_not_recorded", K=2, n=2, S=[0.0, -1.0], slot=[0, 1],
         cands={0: [(3, -0.5), (4, -1.0), (E, -2.0)], 1: [(5, -1.5), (E, -1.75), (6, -2.0)]},
         # order: 3(-0.5), 4(-1.0) -> stop; both eot candidates come later and are dropped
         expect=dict(S=[-0.5, -1.0], slot=[0, 1], tok=[3, 4], src=[0, 0], pool=[], complete=0)),
    dict(name="pool_fills_to_K_and_the_clip_completes", K=2, n=2, S=[0.0, -1.0], slot=[0, 1], pool=[([7], -0.75)],
         cands={0: [(E, -0.25), (3, -1.0), (4, -2.0)], 1: [(E, -0.5), (5, -0.625), (6, -3.0)]},
         # order: eot(-0.25, r0), 3(-1.0), eot(-1.5, r1), 5(-1.625) -> stop. The pool had 1: only the first eot fits.
         expect=dict(S=[-1.0, -1.625], slot=[0, 1], tok=[3, 5], src=[0, 1], pool=[([7], -0.75), (hist_of(0, 2), -0.25)], complete=1)),
    dict(name="fewer_than_K_candidates_leave_dead_ranks", K=3, n=2, S=[0.0, -INF, -INF], slot=[0, 1, 2],
         cands={0: [(3, -0.5), (E, -1.0)]},
         expect=dict(S=[-0.5, -INF, -INF], slot=[0, 1, 2], tok=[3, E, E], src=[0, 1, 2], pool=[(hist_of(0, 2), -1.0)], complete=0)),
    dict(name="a_dead_rank_proposes_nothing", K=2, n=2, S=[-1.0, -INF], slot=[0, 1],
         cands={0: [(3, -0.5), (4, -0.75), (5, -1.0)], 1: [(6, 0.0), (7, 0.0), (8, 0.0)]},  # (the dead rank's slot holds stale candidates)
         expect=dict(S=[-1.5, -1.75], slot=[0, 1], tok=[3, 4], src=[0, 0], pool=[], complete=0)),
    dict(name="equal_scores_go_by_parent_rank_then_position", K=3, n=2, S=[-1.0, -1.0, -0.5], slot=[2, 0, 1],
         cands={0: [(3, -1.0), (4, -1.0), (5, -2.0)], 1: [(6, -1.0), (7, -2.0), (8, -3.0)], 2: [(1, -1.5), (2, -2.5), (E, -9.0)]},
         # four candidates at -2.0: r0p0, r0p1, r1p0, r2p0 in that order, whatever slots the ranks sit in. New ranks: 3 (r0), 4 (r0), 6 (r1).
         # r0 sits in slot 2 (its best child stays), r1 in slot 0 (stays); the second child of r0 takes the free slot 1.
         expect=dict(S=[-2.0, -2.0, -2.0], slot=[2, 1, 0], tok=[6, 4, 3], src=[0, 2, 2], pool=[], complete=0)),
    dict(name="first_step_with_one_live_rank", K=3, n=0, S=[0.0, -INF, -INF], slot=[0, 1, 2],
         cands={0: [(20, -0.125), (21, -0.25), (22, -0.5), (23, -1.0)]},
         expect=dict(S=[-0.125, -0.25, -0.5], slot=[0, 1, 2], tok=[20, 21, 22], src=[0, 0, 0], pool=[], complete=0)),
    dict(name="slot_assignment_no_slot_read_and_written", K=4, n=3, S=[-1.0, -5.0, 0.0, -6.0], slot=[3, 1, 0, 2],
         cands={0: [(6, -0.25), (7, -2.0)], 1: [(8, -1.0)], 2: [(3, -0.125), (4, -0.25), (5, -1.5), (2, -4.0)], 3: [(1, -1.0)]},
         # order: 3(-0.125, r2), 4(-0.25, r2), 6(-1.25, r0), 5(-1.5, r2) -> stop. r2 sits in slot 0, r0 in slot 3: their best children
         # stay; the other two children of r2 take the slots of the childless parents, 1 and 2, in ascending order.
         expect=dict(S=[-0.125, -0.25, -1.25, -1.5], slot=[0, 1, 3, 2], tok=[3, 4, 5, 6], src=[0, 0, 0, 3], pool=[], complete=0)),
    dict(name="no_candidate_at_all_completes_the_clip", K=2, n=2, S=[-1.0, -INF], slot=[1, 0], cands={0: []},
         expect=dict(S=[-INF, -INF], slot=[0, 1], tok=[E, E], src=[0, 1], pool=[], complete=1)),
]


def build(case):
    """-> (state dict in beam_reference's layout, cand_id, cand_logprob, n_cand)."""
    K, n = case["K"], case["n"]
    M = K + 1
    hist = np.full((K, STRIDE), E, dtype=np.int32)
    for s in range(K):
        hist[s, :n] = hist_of(s, n)
    pool = case.get("pool", [])
    pool_ids = np.zeros((K, STRIDE), dtype=np.int32)
    pool_len = np.zeros(K, dtype=np.int32)
    pool_score = np.zeros(K, dtype=np.float32)
    for i, (ids, sc) in enumerate(pool):
        pool_ids[i, : len(ids)] = ids
        pool_len[i] = len(ids)
        pool_score[i] = sc
    state = dict(K=K, n=n, hist=hist, S=np.array(case["S"], dtype=np.float32), slot=np.array(case["slot"], dtype=np.int32),
                 pool_n=np.array([len(pool)], dtype=np.int32), pool_ids=pool_ids, pool_len=pool_len, pool_score=pool_score,
                 complete=np.array([case.get("complete", 0)], dtype=np.int32))
    cid = np.full((K, M), E, dtype=np.int32)
    clp = np.full((K, M), -np.inf, dtype=np.float32)
    nc = np.zeros(K, dtype=np.int32)
    for r, cs in case["cands"].items():
        s = case["slot"][r]
        nc[s] = len(cs)
        for q, (t, lp) in enumerate(cs):
            cid[s, q] = t
            clp[s, q] = lp
    return state, cid, clp, nc


def check(case, new):
    """`new`: the state after the step (beam_reference.select's or Whisper.beam_select's) against the case's expectation."""
    ex, K = case["expect"], case["K"]
    name = case["name"]
    assert new["S"].tolist() == [np.float32(v) for v in ex["S"]], (name, new["S"])
    assert new["slot"].tolist() == ex["slot"], (name, new["slot"])
    assert new["tok"].tolist() == ex["tok"], (name, new["tok"])
    assert new["src"].tolist() == ex["src"], (name, new["src"])
    assert int(new["pool_n"][0]) == len(ex["pool"]), (name, new["pool_n"])
    for i, (ids, sc) in enumerate(ex["pool"]):
        assert new["pool_ids"][i, : new["pool_len"][i]].tolist() == ids and new["pool_score"][i] == np.float32(sc), (name, i)
    assert int(new["complete"][0]) == ex["complete"], name
    assert new["n_completed"] == ex["complete"] - case.get("complete", 0), name
    # by slot: the score of the rank that lives there; the chosen ids sit at the histories' index n
    for r in range(K):
        assert new["slot_score"][new["slot"][r]] == new["S"][r], name
    assert new["hist"][:, case["n"]].tolist() == ex["tok"], name
    # the reorder's rule: a slot that is read keeps its content
    src = new["src"]
    assert all(src[src[s]] == src[s] for s in range(K)), (name, src)
    assert sorted(new["slot"].tolist()) == list(range(K)), name
