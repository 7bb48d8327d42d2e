"""CPU: the persistent launch's rules in float64 (tests/persist_ts_reference.py) against tests/ts_reference.py — the allowed sets
from four carried values equal the sets from the history, and a row split into P workgroup ranges (with and without a resident
tail), accumulated per range and merged, decides as the whole row does."""
import math

import numpy as np
import pytest

import persist_ts_reference as ptr
import ts_reference as tsr

NVS = (51865, 51866)


def _ids(nv):
    return nv - tsr.N_TIMESTAMPS, 50257  # (T, E) of the two Whisper vocabularies, as tsr.crafted_cases has them


def _histories(T, E, rng, n_random=40):
    out = [[], [T], [T + 3, 7, 9], [T + 3, 7, 9, T + 20], [T + 3, 7, 9, T + 20, T + 20], [5, 6], [T + 1500], [T + 3, 8, T + 1500],
           [T + 3, 8, T + 1500, T + 1500], [T + 1499, 4]]
    for _ in range(n_random):
        seq, t = [], 0
        for _ in range(int(rng.integers(0, 14))):
            if rng.random() < 0.4 and t < 1500:
                t = int(rng.integers(t, 1501))
                seq.append(T + t)
            else:
                seq.append(int(rng.integers(0, E)))
        out.append(seq)
    return out


@pytest.mark.parametrize("nv", NVS)
def test_state_tracked_sets_equal_the_history_scan(nv):
    T, E = _ids(nv)
    assert 0 < E < T
    rng = np.random.default_rng(5)
    for seq in _histories(T, E, rng):
        st = ptr.state_of(seq, T)
        assert st[0] == len(seq)
        got, want = ptr.allowed_from_state(st, T, E, nv), tsr.allowed(seq, T, E, nv)
        assert np.array_equal(got, want), (seq, np.flatnonzero(got != want)[:8])


def _rows(nv, rng):
    T, E = _ids(nv)
    rows = [(name, x, seq) for name, x, seq, _ in tsr.crafted_cases(nv)]
    for name, x, seq, want in tsr.crafted_cases(nv):
        assert tsr.decide(x, seq, T, E)[0] == want, name  # (T, E) above are the crafted rows' own
    for i, seq in enumerate(_histories(T, E, rng, n_random=6)):
        x = (rng.standard_normal(nv) * 4.0).astype(np.float32)
        if i % 3 == 0:
            x[T:] += np.float32(3.0)  # rule 5 within reach
        if i % 4 == 1:
            x[rng.integers(0, nv, 50)] = np.nan
        rows.append(("random%d" % i, x, seq))
    return rows


@pytest.mark.parametrize("resident", [0, 96], ids=["streamed", "resident_tail"])
@pytest.mark.parametrize("P", [3, 128, 256])
@pytest.mark.parametrize("nv", NVS)
def test_split_and_merge_decides_as_the_whole_row(nv, P, resident):
    T, E = _ids(nv)
    rng = np.random.default_rng(100 + P)
    for name, x, seq in _rows(nv, rng):
        want, info = tsr.decide(x, seq, T, E)
        got, lp = ptr.decide_split(x, seq, T, E, P, resident)
        assert got == want, (name, P, resident, got, want, info)
        # the normaliser of the final set: float64 sums in two orders
        x64 = np.asarray(x, dtype=np.float64)
        ok = tsr.allowed(seq, T, E, nv) & ~np.isnan(x64)
        if info["rule5"]:
            ok[:T] = False
        ref = x64[want] - tsr._lse(x64[ok]) if ok.any() and math.isfinite(x64[want]) else None
        if ref is not None and math.isfinite(ref):
            assert abs(lp - ref) <= 1e-9 * max(1.0, abs(ref)), (name, lp, ref)


def test_ties_across_a_range_boundary_go_to_the_lower_index():
    nv = 51865
    T, E = _ids(nv)
    for P in (3, 128, 256):
        b = ptr.workgroup_ranges(nv, P)[1][0]  # first row of the second range
        x = np.full(nv, -5.0, dtype=np.float32)
        x[b - 1] = x[b] = 2.0                  # the best text id twice, on both sides of the boundary
        x[T:] = -50.0                          # (the timestamps' mass stays below it)
        assert ptr.decide_split(x, [T, 5], T, E, P)[0] == b - 1 == tsr.decide(x, [T, 5], T, E)[0]
        tb = next((v0 for v0, _ in ptr.workgroup_ranges(nv, P) if v0 > T + 10), None)
        if tb is None:                         # (P = 3: no boundary inside the timestamps)
            continue
        x[tb - 1] = x[tb] = 1.0                # the best timestamp twice, on both sides of a boundary
        x[:T] = -50.0                          # rule 5 fires: the timestamps' tie
        assert ptr.decide_split(x, [T, 5], T, E, P)[0] == tb - 1 == tsr.decide(x, [T, 5], T, E)[0]


def test_suppressed_ids_count_as_masked():
    nv = 51865
    T, E = _ids(nv)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(nv) * 3.0).astype(np.float32)
    x[T:] -= np.float32(20.0)
    best = int(np.argmax(x[:E]))
    sup = np.zeros(nv, dtype=bool)
    sup[best] = True
    xs = x.copy()
    xs[best] = -np.inf
    want = tsr.decide(xs, [T, 5], T, E)[0]
    assert want != best
    for P in (3, 256):
        assert ptr.decide_split(x, [T, 5], T, E, P, 96, sup)[0] == want
