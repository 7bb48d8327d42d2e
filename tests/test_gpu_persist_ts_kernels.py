"""GPU: the pieces of the persistent launch's rules instantiation alone (tests/cpp/persist_ts_driver.cpp) against float64
(tests/persist_ts_reference.py, tests/ts_reference.py): allowed_sets_from_state against allowed_sets on the same histories; a
workgroup's record over its range under the launch's lane layout, both row loops; publish and gather-merge for P in {3, 128, 256}
with the decision. The merge launch runs after the launch that published has finished: no test kernel waits on another workgroup.

Bars. Ids are exact: the rows are float32 and first-best over equal values is decided by index. The (max, sum) pairs are float32 sums
of at most 51866 terms in [0, 1] merged pairwise: |sum - ref| <= 2^-23 * n_terms * ref is the worst case of any summation order
(Higham, Accuracy and Stability, (4.4) with u = 2^-24 and the exponentials' own 2 ulp); the test uses that bound per pair, and for a
log-probability 1e-4 + 1e-6 * max(|x|, |lse|), the bar of tests/test_gpu_scores.py."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import kernel_driver as kd
import persist_ts_reference as ptr
import ts_reference as tsr

pytestmark = pytest.mark.gpu

NV = (51865, 51866)
E = 50257


@pytest.fixture(scope="module", params=kd.DTYPES)
def driver(request):
    dt = request.param
    return kd.driver_exe(dt, source="persist_ts_driver.cpp", linked=(), also=("common.hpp", "decode_rules.hpp", "decode_persistent_common.hpp",
                                                                              "decode_persistent_rules.hpp"))


def _run(driver, tmp_path, cases):
    """cases: list of bytes (form included) -> the driver's output bytes"""
    cin, cout = os.path.join(str(tmp_path), "cases.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<i", len(cases)) + b"".join(cases))
    r = subprocess.run([driver, cin, cout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return open(cout, "rb").read()


def _histories(T, rng, n_random=24):
    out = [[], [T], [T + 3, 7, 9], [T + 3, 7, 9, T + 20], [T + 3, 7, 9, T + 20, T + 20], [5, 6], [T + 1500], [T + 3, 8, T + 1500],
           [T + 3, 8, T + 1500, T + 1500], [T + 1499, 4]]
    for _ in range(n_random):
        seq, t = [], 0
        for _ in range(int(rng.integers(0, 40))):
            if rng.random() < 0.4 and t < 1500:
                t = int(rng.integers(t, 1501))
                seq.append(T + t)
            else:
                seq.append(int(rng.integers(0, E)))
        out.append(seq)
    return out


@pytest.mark.parametrize("nv", NV)
def test_sets_from_state_equal_the_history_scan(driver, tmp_path, nv):
    T = nv - tsr.N_TIMESTAMPS
    hs = _histories(T, np.random.default_rng(nv))
    cases = [struct.pack("<5i", 0, T, E, nv, len(h)) + np.asarray(h, dtype=np.int32).tobytes() for h in hs]
    got = np.frombuffer(_run(driver, tmp_path, cases), dtype=np.int32).reshape(len(hs), 2, 6)
    for h, g in zip(hs, got):
        assert np.array_equal(g[0], g[1]), (h, g)
        ok = tsr.allowed(h, T, E, nv)
        mine = np.zeros(nv, dtype=bool)
        if g[1][0]:
            mine[:E] = True
        if g[1][1]:
            mine[E] = True
        mine[g[1][2]:g[1][3]] = True
        assert np.array_equal(mine, ok), h


def _step_case(x, seq, T, nv, P, LD, resident, whole=False, ns=0, mask_ids=None):
    mask = np.zeros((nv + 127) // 128 * 4, dtype=np.uint32)
    for i in mask_ids or []:
        mask[i >> 5] |= np.uint32(1 << (i & 31))
    return (struct.pack("<11i", 1, T, E, nv, P, LD, resident, int(whole), ns, int(mask_ids is not None), len(seq)) +
            np.asarray(seq, dtype=np.int32).tobytes() + np.asarray(x, dtype=np.float32).tobytes() + mask.tobytes())


def _parse_steps(buf, Ps):
    out, pos = [], 0
    for P in Ps:
        rec = np.frombuffer(buf, dtype=np.uint32, count=8 * P, offset=pos).reshape(P, 8); pos += 32 * P
        cid = struct.unpack_from("<i", buf, pos)[0]
        val, lp = struct.unpack_from("<2f", buf, pos + 4); pos += 12
        grid = np.frombuffer(buf, dtype=np.uint32, count=8, offset=pos); pos += 32
        out.append((rec, cid, val, lp, grid))
    assert pos == len(buf)
    return out


def _f(u):
    return float(np.uint32(u).view(np.float32))


def _check_record(words, ref, n_rows, what):
    """A device record against the float64 one: ids and winners exact, (max, sum) pairs within the summation bound."""
    tv, ti, sv, si = _f(words[0]), int(np.uint32(words[1]).view(np.int32)), _f(words[2]), int(np.uint32(words[3]).view(np.int32))
    assert (ti, si) == (ref["ti"], ref["si"]), (what, ti, si, ref)
    for got, want in ((tv, ref["tv"]), (sv, ref["sv"])):
        assert got == want or (math.isnan(got) and math.isnan(want)), (what, got, want)
    for k, (gm, gs, wm, ws) in enumerate(((_f(words[4]), _f(words[5]), ref["mt"], ref["st"]), (_f(words[6]), _f(words[7]), ref["m"], ref["s"]))):
        assert gm == wm, (what, k, gm, wm)
        if math.isfinite(wm):
            assert abs(gs - ws) <= 2.0 ** -23 * max(n_rows, 1) * ws + 1e-30, (what, k, gs, ws)


def _rows(nv, rng):
    T = nv - tsr.N_TIMESTAMPS
    rows = [(name, x, seq, want) for name, x, seq, want in tsr.crafted_cases(nv)]
    for P in (3, 128, 256):  # the best text id and the best timestamp tie across a range boundary
        b = ptr.workgroup_ranges(nv, P)[1][0]
        x = np.full(nv, -5.0, dtype=np.float32); x[T:] = -50.0; x[b - 1] = x[b] = 2.0
        rows.append(("text_tie_P%d" % P, x, [T, 5], b - 1))
        tb = next((v0 for v0, _ in ptr.workgroup_ranges(nv, P) if v0 > T + 10), None)
        if tb is not None:
            x = np.full(nv, -50.0, dtype=np.float32); x[tb - 1] = x[tb] = 1.0
            rows.append(("timestamp_tie_P%d" % P, x, [T, 5], tb - 1))
    x = (rng.standard_normal(nv) * 4.0).astype(np.float32); x[T:] += np.float32(3.0)
    rows.append(("random_rule5", x, [T + 3, 7, 9], None))
    x = (rng.standard_normal(nv) * 4.0).astype(np.float32); x[rng.integers(0, nv, 80)] = np.nan
    rows.append(("random_nan", x, [T + 3, 7, 9, T + 20], None))
    return rows


@pytest.mark.parametrize("P,LD,resident", [(3, 32, 0), (128, 16, 160), (256, 32, 80), (256, 32, 0)])
@pytest.mark.parametrize("nv", NV)
def test_records_publish_and_merge(driver, tmp_path, nv, P, LD, resident):
    """Every workgroup's record (ranges that straddle E and T among them), the merged record and the decision: the crafted rows with
    their exact ids, ties across a range boundary, an empty allowed set, all-NaN and all -inf rows, random rows."""
    T = nv - tsr.N_TIMESTAMPS
    rows = _rows(nv, np.random.default_rng(7 * P + nv))
    got = _parse_steps(_run(driver, tmp_path, [_step_case(x, seq, T, nv, P, LD, resident) for _, x, seq, _ in rows]), [P] * len(rows))
    ranges = ptr.workgroup_ranges(nv, P)
    assert any(v0 <= E < v1 - 1 and v0 < E for v0, v1 in ranges) and any(v0 < T < v1 for v0, v1 in ranges)  # a range straddles E, one T
    for (name, x, seq, want), (rec, cid, val, lp, grid) in zip(rows, got):
        x64 = np.asarray(x, dtype=np.float64)
        ok = ptr.allowed_from_state(ptr.state_of(seq, T), T, E, nv)
        refs = ptr.split_records(x64, ok, E, P, resident)
        for w, (v0, v1) in enumerate(ranges):
            _check_record(rec[w], refs[w], v1 - v0, (name, "workgroup", w))
        _check_record(grid, ptr.merge_all(refs), nv, (name, "grid"))
        py, info = tsr.decide(x, seq, T, E)
        assert py == (want if want is not None else py)
        if cid != py:
            assert info["margin"] < 1e-4, (name, cid, py, info)  # (rule 5 on float32 sums against float64: only at a near-tie)
            continue
        rid, rlp = ptr.decide(ptr.merge_all(refs), E)
        assert rid == py
        if math.isfinite(rlp):
            assert abs(lp - rlp) <= 1e-4 + 1e-6 * max(abs(float(x64[py])), abs(float(x64[py]) - rlp)), (name, lp, rlp)
        else:
            assert lp == rlp, (name, lp, rlp)


def test_suppress_mask_and_whole_row(driver, tmp_path):
    """A suppress mask (ids in several workgroups' ranges, bit 31 and bit 0 of a word among them) makes its text ids count as -inf; the
    step that fed sot takes the whole row as one set and carries the no-speech logit."""
    nv, P, LD, resident = 51866, 256, 32, 80
    T = nv - tsr.N_TIMESTAMPS
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(nv) * 3.0).astype(np.float32); x[T:] -= np.float32(20.0)
    order = np.argsort(-x[:E])
    sup = sorted(int(i) for i in order[:5]) + [31, 32, 63, 64, ptr.workgroup_ranges(nv, P)[9][0]]
    xs = x.copy(); xs[sup] = -np.inf
    seq = [T, 5]
    ns = T - 2
    xn = x.copy(); xn[ns] = np.nan  # non-finite audio: a NaN <|nospeech|> logit gives NaN, as logit - logsumexp does
    cases = [_step_case(x, seq, T, nv, P, LD, resident, mask_ids=sup), _step_case(x, seq, T, nv, P, LD, resident, mask_ids=[]),
             _step_case(x, [], T, nv, P, LD, resident, whole=True, ns=ns, mask_ids=sup),
             _step_case(xn, [], T, nv, P, LD, resident, whole=True, ns=ns)]
    got = _parse_steps(_run(driver, tmp_path, cases), [P] * 4)
    assert math.isnan(got[3][3]) and math.isnan(float(xn[ns]) - tsr._lse(np.asarray(xn, dtype=np.float64)))
    assert got[0][1] == tsr.decide(xs, seq, T, E)[0] and got[0][1] not in sup
    assert got[1][1] == tsr.decide(x, seq, T, E)[0] == int(order[0])
    ok = ptr.allowed_from_state(ptr.state_of(seq, T), T, E, nv)
    refs = ptr.split_records(np.asarray(xs, dtype=np.float64), ok, E, P, resident)  # (-inf: masked, as the mask makes it)
    for w in range(P):
        _check_record(got[0][0][w], refs[w], nv // P + 1, ("suppress", w))
    rec, cid, val, lp, grid = got[2]
    assert cid == ns and val == x[ns]
    ref = float(x[ns]) - tsr._lse(np.asarray(x, dtype=np.float64))
    assert abs(lp - ref) <= 1e-4 + 1e-6 * max(abs(float(x[ns])), abs(float(x[ns]) - ref)), (lp, ref)
