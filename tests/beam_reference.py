"""Python restatement of the beam-search contract (DESIGN.md "Beam search"): the candidates a hypothesis proposes, the selection
step (openai-whisper's BeamSearchDecoder.update over this project's rules), the loop and the finalisation. float64 inside, float32
out — except the candidate score S + logprob, which the contract defines as a float32 sum.

The state is kept in the arrays the GPU kernels use (whisper.axera_amd/csrc/decode_beam.hip), so results compare element for
element: clip c owns slots [c * K, c * K + K); S and slot are indexed by rank, everything else by slot or by clip.

The candidates, selection and reorder kernels, Engine::beam_decode's loop and AX_WHISPER_BeamFinalize are checked against these."""
import math

import numpy as np

import score_reference as scr
import ts_reference as tsr

NEG_INF = np.float32(-np.inf)


# ------------------------------------------------------------------------------------------------ candidates
def candidates(logits, seq, T, E, M, allowed=None, flip_rule5=False):
    """The min(M, |A|) ids of the final allowed set A (scored mode's, -inf entries out) with the largest logit, equal logits to the
    lower id first -> (ids, float32 logprobs x[c] - logsumexp(x[A]), decide()'s info or None).
    allowed: bool [nv] instead of the timestamp rules (toy models). flip_rule5: A as if rule 5 had decided the other way (the GPU
    tests' numerical-tie exception)."""
    x = np.asarray(logits, dtype=np.float64)
    info = None
    if allowed is not None:
        A = np.asarray(allowed, dtype=bool) & ~np.isnan(x)
    else:
        _, info = tsr.decide(logits, seq, T, E)
        A = tsr.allowed(seq, T, E, x.size) & ~np.isnan(x)
        info["n_ts_finite"] = int((A[T:] & np.isfinite(x[T:])).sum())
        if info["rule5"] != bool(flip_rule5):
            A[:T] = False
    A &= x > -math.inf
    idx = np.flatnonzero(A)
    if idx.size == 0:
        return [], np.zeros(0, dtype=np.float32), dict(info or {}, lse_allowed=-math.inf)
    order = idx[np.lexsort((idx, -x[idx]))][:M]  # value descending, id ascending
    lse = tsr._lse(x[A])
    lps = np.array([scr._logprob(float(x[c]), lse) for c in order], dtype=np.float32)
    return [int(c) for c in order], lps, dict(info or {}, lse_allowed=lse)


def rule5_near_tie(info, bar=1e-4):
    """The one way a float32 implementation may propose from another set than this reference: rule 5's two sides, logsumexp of the
    timestamps and the best text logit, closer than `bar`. Not with a single finite timestamp: its logsumexp is that logit itself in
    any precision, and the comparison is between two of the caller's float32 numbers."""
    lse, mt = info["lse"], info["max_text"]
    return info["n_ts_finite"] > 1 and math.isfinite(lse) and math.isfinite(mt) and abs(lse - mt) < bar


def token_logprob(logits, seq, T, E, tok):
    """float32 log-probability of `tok` under the final allowed set of the row (-inf when it is not in it) + decide()'s info."""
    x = np.asarray(logits, dtype=np.float64)
    A = scr.final_allowed(logits, seq, T, E) & (x > -math.inf)
    _, info = tsr.decide(logits, seq, T, E)
    lse = tsr._lse(x[A])
    return np.float32(scr._logprob(float(x[tok]), lse) if A[tok] else -math.inf), dict(info, lse_allowed=lse)


def candidate_arrays(rows, hists, T, E, M, live=None):
    """candidates() of every slot -> (cand_id [S][M] int32 padded with E, cand_logprob [S][M] float32 padded with -inf, n_cand [S])."""
    S = len(hists)
    cid = np.full((S, M), E, dtype=np.int32)
    clp = np.full((S, M), -np.inf, dtype=np.float32)
    nc = np.zeros(S, dtype=np.int32)
    for s in range(S):
        if live is not None and not live[s]:
            continue
        ids, lps, _ = candidates(rows[s], hists[s], T, E, M)
        nc[s] = len(ids)
        cid[s, : len(ids)] = ids
        clp[s, : len(ids)] = lps
    return cid, clp, nc


# ------------------------------------------------------------------------------------------------ state
def initial_state(clips, K, stride, fill=0):
    S = np.full(clips * K, -np.inf, dtype=np.float32)
    S[::K] = 0.0
    return dict(K=K, n=0, hist=np.full((clips * K, stride), fill, dtype=np.int32), S=S, slot=np.arange(clips * K, dtype=np.int32),
                pool_n=np.zeros(clips, dtype=np.int32), pool_ids=np.zeros((clips * K, stride), dtype=np.int32),
                pool_len=np.zeros(clips * K, dtype=np.int32), pool_score=np.zeros(clips * K, dtype=np.float32),
                complete=np.zeros(clips, dtype=np.int32))


def _copy(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def select(state, cand_id, cand_logprob, n_cand, E):
    """One selection step. Returns the new state (n + 1; hist has the chosen ids at index n, the reorder's copies are NOT applied)
    with tok, src, slot_score [S] by slot and n_completed added. Entries of pool_* beyond pool_n keep what they held."""
    st = _copy(state)
    K, n = st["K"], st["n"]
    clips = len(st["pool_n"])
    S_old, slot_old, hist = state["S"], state["slot"], st["hist"]
    slots = clips * K
    tok = hist[:, n].copy()
    src = np.arange(slots, dtype=np.int32)
    slot_score = np.zeros(slots, dtype=np.float32)
    done = 0
    for c in range(clips):
        r0 = c * K
        if state["complete"][c]:  # frozen
            for r in range(K):
                slot_score[slot_old[r0 + r]] = S_old[r0 + r]
            continue
        cands = []
        for j in range(K):
            if S_old[r0 + j] == -np.inf:  # dead: proposes nothing
                continue
            s = int(slot_old[r0 + j])
            for q in range(int(n_cand[s])):
                with np.errstate(invalid="ignore", over="ignore"):
                    score = np.float32(S_old[r0 + j]) + np.float32(cand_logprob[s][q])  # THE float32 sum
                cands.append((score, j, q, int(cand_id[s][q])))
        order = sorted(cands, key=lambda t: t[0], reverse=True)  # stable: equal scores stay in (parent rank, position) order
        new, fin = [], []
        for score, j, q, t in order:
            if t != E:
                new.append((score, j, t))
                if len(new) == K:
                    break
            else:
                fin.append((score, j))
        for score, j in fin:  # the pool, in walk order
            if st["pool_n"][c] >= K:
                break
            i = r0 + int(st["pool_n"][c])
            st["pool_ids"][i, :n] = state["hist"][slot_old[r0 + j], :n]
            st["pool_len"][i] = n
            st["pool_score"][i] = score
            st["pool_n"][c] += 1
        # slots: a surviving parent's best child stays; the other children, then the dead ranks, take the free slots in ascending order
        new_slot = [-1] * K
        kept = {}
        for r, (_, j, _) in enumerate(new):
            ps = int(slot_old[r0 + j])
            if ps not in kept:
                kept[ps] = r
                new_slot[r] = ps
        free = [s for s in range(r0, r0 + K) if s not in kept]
        for r in range(K):
            if new_slot[r] < 0:
                new_slot[r] = free.pop(0)
        for r in range(K):
            s = new_slot[r]
            st["slot"][r0 + r] = s
            if r < len(new):
                st["S"][r0 + r] = new[r][0]
                tok[s] = new[r][2]
                src[s] = slot_old[r0 + new[r][1]]
            else:
                st["S"][r0 + r] = -np.inf
                tok[s] = E
                src[s] = s
            slot_score[s] = st["S"][r0 + r]
            hist[s, n] = tok[s]
        if st["pool_n"][c] >= K or not new:
            st["complete"][c] = 1
            done += 1
    st["n"] = n + 1
    st.update(tok=tok, src=src, slot_score=slot_score, n_completed=done)
    return st


def apply_reorder(state, src):
    """hist[slot][0, n) <- hist[src[slot]][0, n) for the step that produced `state` (n = its length - 1)."""
    n = state["n"] - 1
    before = state["hist"].copy()
    for s, f in enumerate(src):
        if f != s:
            state["hist"][s, :n] = before[f, :n]
    return state


def check_no_read_and_write(src):
    """The reorder's rule: a slot that is copied from keeps its own content."""
    src = np.asarray(src)
    moved = np.flatnonzero(src != np.arange(src.size))
    return all(src[src[s]] == src[s] for s in moved)


# ------------------------------------------------------------------------------------------------ finalise
def finalize(state):
    """Per clip: dict(ids, sum_logprob, avg_logprob, ended_eot, winner, records [(ids, float32 score, from_pool)])."""
    K, n = state["K"], state["n"]
    out = []
    for c in range(len(state["pool_n"])):
        r0 = c * K
        recs = [(state["pool_ids"][r0 + i, : state["pool_len"][r0 + i]].tolist(), np.float32(state["pool_score"][r0 + i]), True)
                for i in range(int(state["pool_n"][c]))]
        for r in range(K):
            if len(recs) >= K:
                break
            if state["S"][r0 + r] == -np.inf:
                continue
            recs.append((state["hist"][state["slot"][r0 + r], :n].tolist(), np.float32(state["S"][r0 + r]), False))
        if not recs:
            out.append(dict(ids=[], sum_logprob=NEG_INF, avg_logprob=NEG_INF, ended_eot=False, winner=-1, records=[]))
            continue
        keys = [float(sc) / max(len(ids), 1) for ids, sc, _ in recs]
        w = max(range(len(recs)), key=lambda i: (keys[i], -i))  # the first maximum
        ids, sc, pooled = recs[w]
        out.append(dict(ids=ids, sum_logprob=np.float32(sc), avg_logprob=np.float32(float(sc) / (len(ids) + 1)), ended_eot=pooled, winner=w,
                        records=recs))
    return out


# ------------------------------------------------------------------------------------------------ the loop
def beam_search(clips, K, max_new, stride, T, E, rows_fn, reorder_fn=None, allowed=None):
    """rows_fn(n, state) -> one row per slot (None for slots that need none) for the step at history length n; reorder_fn(src) is
    told every step's source map (a model with caches copies them). Returns (finalize()'s list, final state, log): log[n] =
    dict(cand_id, cand_logprob, n_cand, state after the step)."""
    st = initial_state(clips, K, stride, fill=E)
    M = K + 1
    log = []
    for n in range(max_new):
        if st["complete"].all():
            break
        rows = rows_fn(n, st)
        rank_of = {int(st["slot"][i]): i for i in range(clips * K)}
        cid = np.full((clips * K, M), E, dtype=np.int32)
        clp = np.full((clips * K, M), -np.inf, dtype=np.float32)
        nc = np.zeros(clips * K, dtype=np.int32)
        for s in range(clips * K):
            if st["complete"][s // K] or st["S"][rank_of[s]] == -np.inf:
                continue
            ids, lps, _ = candidates(rows[s], st["hist"][s, :n].tolist(), T, E, M, allowed=allowed)
            nc[s] = len(ids)
            cid[s, : len(ids)] = ids
            clp[s, : len(ids)] = lps
        st = select(st, cid, clp, nc, E)
        apply_reorder(st, st["src"])
        if reorder_fn is not None:
            reorder_fn(st["src"])
        log.append(dict(cand_id=cid, cand_logprob=clp, n_cand=nc, state=_copy(st)))
    return finalize(st), st, log


def boundary_gap(state_before, cand_id, cand_logprob, n_cand, E):
    """Per clip, how far the step is from selecting another set: the score gap between the last candidate the walk takes and the
    first it does not reach (inf when it takes them all)."""
    K = state_before["K"]
    gaps = []
    for c in range(len(state_before["pool_n"])):
        if state_before["complete"][c]:
            gaps.append(math.inf)
            continue
        r0 = c * K
        sc = []
        for j in range(K):
            if state_before["S"][r0 + j] == -np.inf:
                continue
            s = int(state_before["slot"][r0 + j])
            sc += [(float(np.float32(state_before["S"][r0 + j]) + np.float32(cand_logprob[s][q])), int(cand_id[s][q])) for q in range(int(n_cand[s]))]
        sc.sort(key=lambda t: -t[0])
        taken, stop = 0, None
        for i, (_, t) in enumerate(sc):
            if t != E:
                taken += 1
                if taken == K:
                    stop = i
                    break
        gaps.append(sc[stop][0] - sc[stop + 1][0] if stop is not None and stop + 1 < len(sc) else math.inf)
    return gaps


def oracle_beam(orc, kvs, prefix, K, max_new, T, E):
    """beam_search over oracle.Oracle.decoder_step: one self-attention cache per slot, copied on reorder; kvs: the cross K/V of
    every clip. Only live hypotheses are stepped. Returns beam_search's triple, log entries with `gap` (boundary_gap) and `before`."""
    clips, stride = len(kvs), int(orc.cfg["n_text_ctx"])
    caches = [orc.new_self_cache() for _ in range(clips * K)]
    for c in range(clips):  # sot and the language token through rank 0's slot; the other slots get their cache by the first reorder
        for off in range(2):
            orc.decoder_step(prefix[off], off, *kvs[c], *caches[c * K], want_logits=False)
    befores = []

    def rows_fn(n, st):
        befores.append(_copy(st))
        rank_of = {int(st["slot"][i]): i for i in range(clips * K)}
        rows = [None] * (clips * K)
        for s in range(clips * K):
            if st["complete"][s // K] or st["S"][rank_of[s]] == -np.inf:
                continue
            tok = prefix[2] if n == 0 else int(st["hist"][s, n - 1])
            rows[s] = orc.decoder_step(tok, n + 2, *kvs[s // K], *caches[s])
        return rows

    def reorder_fn(src):
        for s, f in enumerate(src):
            if f != s:
                caches[s] = (caches[f][0].copy(), caches[f][1].copy())

    out, st, log = beam_search(clips, K, max_new, stride, T, E, rows_fn, reorder_fn)
    for entry, before in zip(log, befores):
        entry["before"] = before
        entry["gap"] = boundary_gap(before, entry["cand_id"], entry["cand_logprob"], entry["n_cand"], E)
    return out, st, log
