"""Python restatement, in float64, of what the persistent launch's rules instantiation adds (DESIGN.md §11,
whisper.axera_amd/csrc/decode_persistent_rules.hpp): the allowed sets from four values of the history, a workgroup's partial record
over its own vocabulary range, the associative merge of records, and the decision from the merged record.

A record is the dict {tv, ti, sv, si, mt, st, m, s}: first-best allowed id of [0, E]; first-best allowed timestamp; (max, sum) of
the allowed ids of [0, E]; (max, sum) of the allowed timestamps. NaN counts as masked, ties go to the lower index."""
import math

import numpy as np

NONE = 0x7FFFFFFF


def state_of(seq, T):
    """The four values carried per token: n, id of the last timestamp (-1: none), last id is a timestamp, the one before it is."""
    n, last_ts, last_is, penult_is = 0, -1, False, False
    for t in seq:
        penult_is = last_is
        last_is = t >= T
        if t >= T:
            last_ts = t
        n += 1
    return n, last_ts, last_is, penult_is


def allowed_from_state(state, T, E, nv):
    """allowed_sets_from_state as a bool mask [nv]."""
    n, last_ts_id, last_is, penult_is = state
    last_ts = n >= 1 and last_is
    penult_ts = n < 2 or penult_is
    pair_open = last_ts and not penult_ts
    text_on = n > 0 and not pair_open
    eot_on = n > 0
    lo, hi = T, nv
    if n >= 1 and last_ts_id >= T:
        lo = min(last_ts_id + (0 if pair_open else 1), nv)
    if last_ts and penult_ts:
        hi = T
    if n == 0:
        hi = min(hi, T + 51)
    lo = min(lo, hi)
    ok = np.zeros(nv, dtype=bool)
    if text_on:
        ok[:E] = True
    if eot_on:
        ok[E] = True
    ok[lo:hi] = True
    return ok


def empty():
    return dict(tv=-math.inf, ti=NONE, sv=-math.inf, si=NONE, mt=-math.inf, st=0.0, m=-math.inf, s=0.0)


def lse_merge(m, s, m2, s2):
    if m2 > m:
        m, s, m2, s2 = m2, s2, m, s
    if m2 == -math.inf:
        return m, s
    if m == math.inf:
        return m, 1.0
    return m, s + s2 * math.exp(m2 - m)


def take(rec, ok, x, row, E, suppressed=False):
    """One logit into a record (rules_rec_take)."""
    x = float(x)
    if row <= E:
        on = bool(ok[row]) and not suppressed
        if on and x > rec["tv"]:
            rec["tv"], rec["ti"] = x, row
        if on and x == x:
            rec["mt"], rec["st"] = lse_merge(rec["mt"], rec["st"], x, 1.0)
    elif ok[row] and x == x:
        if x > rec["sv"]:
            rec["sv"], rec["si"] = x, row
        rec["m"], rec["s"] = lse_merge(rec["m"], rec["s"], x, 1.0)


def merge(a, b):
    """The associative merge of two records (argmax_take twice, lse_merge twice)."""
    r = dict(a)
    if b["tv"] > r["tv"] or (b["tv"] == r["tv"] and b["ti"] < r["ti"]):
        r["tv"], r["ti"] = b["tv"], b["ti"]
    if b["sv"] > r["sv"] or (b["sv"] == r["sv"] and b["si"] < r["si"]):
        r["sv"], r["si"] = b["sv"], b["si"]
    r["mt"], r["st"] = lse_merge(r["mt"], r["st"], b["mt"], b["st"])
    r["m"], r["s"] = lse_merge(r["m"], r["s"], b["m"], b["s"])
    return r


def range_record(x, ok, E, lo, hi, suppress=None):
    rec = empty()
    for row in lo + np.flatnonzero(ok[lo:hi]):  # (a row outside the sets leaves the record as it is)
        row = int(row)
        take(rec, ok, x[row], row, E, suppress is not None and row < E and bool(suppress[row]))
    return rec


def workgroup_ranges(nv, P):
    """[v0, v1) of workgroup w: the even deal of RowSet::prefetch."""
    return [(w * nv // P, (w + 1) * nv // P) for w in range(P)]


def split_records(x, ok, E, P, resident=0, suppress=None):
    """One record per workgroup; with `resident` > 0 each range is split into a streamed head and a resident tail of at most that
    many rows (the poller waves' rows), accumulated apart and merged head first, as compute wave 0 does."""
    out = []
    for v0, v1 in workgroup_ranges(len(x), P):
        vb = max(v0, v1 - resident) if resident > 0 else v1
        rec = range_record(x, ok, E, v0, vb, suppress)
        if vb < v1:
            rec = merge(rec, range_record(x, ok, E, vb, v1, suppress))
        out.append(rec)
    return out


def merge_all(records):
    r = empty()
    for q in records:
        r = merge(r, q)
    return r


def lse_value(m, s):
    return m if m in (-math.inf, math.inf) else m + math.log(s)


def decide(rec, E):
    """rule5_fires, final_pick, final_set_merge, logprob_of on a merged record -> (id, logprob)."""
    rule5 = lse_value(rec["m"], rec["s"]) > rec["tv"]
    if not rule5 and rec["tv"] > -math.inf and rec["tv"] >= rec["sv"]:
        cid, cv = rec["ti"], rec["tv"]
    elif rec["sv"] > -math.inf:
        cid, cv = rec["si"], rec["sv"]
    else:
        cid, cv = E, -math.inf
    m, s = rec["m"], rec["s"]
    if not rule5:
        m, s = lse_merge(m, s, rec["mt"], rec["st"])
    if m == -math.inf or cv == -math.inf:
        lp = -math.inf
    elif cv == math.inf:
        lp = 0.0
    else:
        lp = cv - lse_value(m, s)
    return cid, lp


def decide_split(x, seq, T, E, P, resident=0, suppress=None):
    """The launch's decision for one row: state -> sets -> a record per workgroup -> merge -> decision."""
    x = np.asarray(x, dtype=np.float64)
    ok = allowed_from_state(state_of(seq, T), T, E, x.size)
    return decide(merge_all(split_records(x, ok, E, P, resident, suppress)), E)
