"""GPU: the weight-row machinery of the persistent launches alone (csrc/decode_persistent_common.hpp: the lane-group reductions,
rows_load / rows_dot / rows_dot_reg, RowSet's prefetch / run / run_ln / publish, RowSetF32, qfold_publish, qfold_unit_query) and the
load-time fold arena (launch_qfold_build), through tests/cpp/persist_rows_driver.cpp: test kernels with the launch's geometry that
spell the calls as decode_persistent.hip does, linked with the shipped decode_persistent objects. Every value is held against the
float64 references of tests/persist_rows_reference.py under bounds derived there (none taken from a GPU result); every granule
buffer comes back whole: the rows of a phase carry the tag, everything else — the guard zones, a workgroup without rows, the other
areas of the fold's granule buffer — is untouched as bits; the (r0, r1) that prefetch computed on the device equal the Python mirror.
Nothing here waits on another workgroup: the fold's consumer launch runs after the producer launch has finished and the driver has
seen the tag in every granule it polls.

One driver process per dtype build and test; after a failed driver run the module's remaining cases are not started."""
import os
import subprocess
import time

import numpy as np
import pytest

import kernel_driver
import persist_rows_reference as PR
from encoder_kernel_reference import U32 as U
from encoder_kernel_reference import from_bits, to_bits
from kernel_driver import DTYPES

pytestmark = pytest.mark.gpu
_session = kernel_driver.Session()
_amp = {}      # (dt, family) -> [median, max] of |mean s| rstd / |result|
_layout = {}   # dt -> the constants the driver printed


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, kernel_driver.driver_exe(request.param, source="persist_rows_driver.cpp", linked=PR.LINKED, also=PR.ALSO)


class Cursor:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert self.at + n <= len(self.raw), "the driver wrote less than its cases ask for"
        v = self.raw[self.at:self.at + n].view(dtype).reshape(shape)
        self.at += n
        return v


def run(driver, cases, tmp_path, refused=False):
    """One driver process over `cases` (bytes each). Returns (the 'ran' lines, Cursor over what it wrote)."""
    dt, exe = driver
    if _session.state["dead"]:
        pytest.fail("not run: an earlier driver run failed (" + _session.state["dead"] + ")")
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            f.write(c)
    try:
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _session.state["dead"] = "timeout"
        raise
    os.remove(fin)
    if refused:
        return r
    if r.returncode != 0 or not r.stdout.rstrip().endswith("done"):
        _session.state["dead"] = f"exit status {r.returncode}"
        pytest.fail(f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    lines = r.stdout.splitlines()
    lay = lines[0].split()
    assert lay[0] == "layout"
    _layout[dt] = {k: int(v) for k, v in zip(lay[1::2], lay[2::2])}
    raw = np.fromfile(fout, dtype=np.uint8)
    os.remove(fout)
    return [ln for ln in lines if ln.startswith("ran ")], Cursor(raw)


def note(dt, what, w):
    _session.worst[dt, what] = max(_session.worst.get((dt, what), 0.0), w)


def test_reductions_and_the_compiled_layout(driver, tmp_path):
    dt, _ = driver
    vs, kinds = PR.reduce_vectors()
    ran, out = run(driver, [np.int32(0).tobytes() + np.int32(len(vs)).tobytes() + vs.tobytes()], tmp_path)
    for k, v in PR.LAY.items():  # the headers as compiled against the headers as read
        assert _layout[dt][k] == v, (k, _layout[dt][k], v)
    got = out.take(np.float32, len(vs), 6, 64)
    for name, w in PR.check_reduce(vs, kinds, got).items():
        note(dt, f"reduce {name}", w)
        print(f"{dt} {name}: worst error / bound {w:.4f}")
    _session.ran[dt].add(("reduce",))


@pytest.mark.parametrize("shape", PR.ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows(driver, tmp_path, shape):
    dt, _ = driver
    LPR, CH = shape
    plan, cases, launches = PR.rows_plan(LPR, CH), [], []
    for gi, (name, N, family, deal_list) in enumerate(plan):
        case = PR.RowsCase(dt, LPR, CH, N, family, PR.rows_seed(LPR, CH, name))
        for di, (P, NS, first) in enumerate(deal_list + (deal_list[:1] if gi == 0 else [])):  # the first launch of a shape runs twice
            cases.append(PR.rows_header(LPR, CH, N, P, NS, first, reuse=int(di > 0)) + (case.payload() if di == 0 else b""))
            launches.append((gi, case, P, NS, first))
        _amp.setdefault((dt, family), []).append((float(np.median(case.amplification)), float(case.amplification.max())))
    ran, out = run(driver, cases, tmp_path)
    assert len(ran) == len(launches)
    tag, guard = _layout[dt]["tag"], _layout[dt]["guard"]
    bits = {}
    for gi, case, P, NS, first in launches:
        own = out.take(np.int32, P, 2)
        gran = out.take(np.uint64, 4, case.N + 2 * guard)
        label = f"{dt} ({LPR}, {CH}) N {case.N} {case.family} P {P} first {first}"
        worst, vals = PR.check_rows(case, P, NS, first, own, gran, tag, guard, label)
        for what, w in worst.items():
            note(dt, f"rows ({LPR}, {CH}) {case.family} {what}", w)
        print(f"{label}: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
        # the same (W, x): the same bits whoever computed the row, in whichever pass, and in a second run
        if gi in bits:
            same = bits[gi][1] == vals.view(np.uint32)
            assert same.all(), f"{label}: bits differ from {bits[gi][0]} at (phase, row) {np.argwhere(~same)[:6].tolist()}"
        else:
            bits[gi] = (label, vals.view(np.uint32).copy())
    assert out.at == len(out.raw)
    _session.ran[dt].add(("rows", shape))


def test_rows_from_registers_give_the_lds_bits(driver, tmp_path):
    dt, _ = driver
    rng = np.random.default_rng(21)
    cases, inputs = [], []
    for LD, CD in PR.REG_SHAPES:
        K, rows = 8 * LD * CD, PR.PL // LD
        W, x = PR.R.weights(rng, rows, K, dt, "benign"), rng.standard_normal(K).astype(np.float32)
        cases.append(np.array([2, LD, CD], np.int32).tobytes() + to_bits(W, dt).tobytes() + x.tobytes())
        inputs.append((LD, CD, W, x))
    ran, out = run(driver, cases, tmp_path)
    for LD, CD, W, x in inputs:
        got = out.take(np.float32, 2, PR.PL)
        lds, reg = got.view(np.uint32)
        assert np.array_equal(lds, reg), f"({LD}, {CD}): rows_dot_reg differs from rows_dot in lanes {np.nonzero(lds != reg)[0][:8]}"
        assert (lds.reshape(-1, LD) == lds.reshape(-1, LD)[:, :1]).all(), f"({LD}, {CD}): the lanes of a row disagree"
        ref, bound = PR.dot_expect(W, x, None, LD, CD)
        ratio = np.abs(got[0].reshape(-1, LD)[:, 0].astype(np.float64) - ref) / bound
        assert ratio.max() <= 1, f"({LD}, {CD}): row {int(np.argmax(ratio))} is {ratio.max():.2f} x its bound"
        note(dt, f"rows_reg ({LD}, {CD})", float(ratio.max()))
        print(f"{dt} rows_reg ({LD}, {CD}): bit-equal to rows_dot; worst error / bound {ratio.max():.4f}")
        _session.ran[dt].add(("rows_reg", (LD, CD)))


def test_the_vocabulary_rows_deal(driver, tmp_path):
    """prefetch's even deal of 51865 / 51866 rows, report only: the vocabulary loop itself is inline in the kernels."""
    dt, _ = driver
    ran, out = run(driver, [PR.rows_header(16, 1, N, P, 0, -1, report=1) for N, P in PR.VOCAB_DEALS], tmp_path)
    for N, P in PR.VOCAB_DEALS:
        own = out.take(np.int32, P, 2)
        assert np.array_equal(own, PR.deals(N, P, -1, 16)), (N, P)
    assert out.at == len(out.raw)
    _session.ran[dt].add(("vocab_deal",))


@pytest.mark.parametrize("what", ["even_too_many_rows", "packed_too_few_workgroups", "no_such_shape"])
def test_driver_refuses_what_a_launch_cannot_take(driver, tmp_path, what):
    """Status 2 before anything is launched: publish stores at most 64 rows and run makes at most two passes."""
    header = {"even_too_many_rows": PR.rows_header(16, 1, 384, 4, 0, -1), "packed_too_few_workgroups": PR.rows_header(32, 3, 2304, 100, 0, 0),
              "no_such_shape": PR.rows_header(16, 2, 256, 16, 0, -1)}[what]
    assert what == "no_such_shape" or not PR.deal_allowed(*{"even_too_many_rows": (384, 4, -1, 16), "packed_too_few_workgroups": (2304, 100, 0, 32)}[what])
    r = run(driver, [header], tmp_path, refused=True)
    assert r.returncode == 2 and "ran " not in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-300:])


def unpack_pairs(words, dt):
    """[n] packed h16 pairs (element 2 t in the low half) -> [2 n] float64."""
    b = np.empty(2 * len(words), np.uint16)
    b[0::2], b[1::2] = words & 0xFFFF, words >> 16
    return from_bits(b, dt)


@pytest.mark.parametrize("d", PR.FOLD_WIDTHS)
def test_query_fold_chain(driver, tmp_path, d):
    dt, _ = driver
    H, dd = d // 64, d * d
    cases = [PR.FoldCase(dt, d, family, kind, 300 + d + ci) for ci, (family, kind) in enumerate(PR.FOLD_CASES)]
    ran, out = run(driver, [c.payload() for c in cases], tmp_path)
    guard = _layout[dt]["guard"]
    for case, line in zip(cases, ran):
        w = line.split()
        info = {k: int(v) for k, v in zip(w[3::2], w[4::2])}
        assert int(w[2]) == d and info["complete"] == 1, line  # a producer that left a granule without its tag: the consumer was not run
        assert info["qfold_stride"] == PR.qfold_stride(d) and info["NP_D"] == PR.producers(d, PR.grid_of(d))[1]["NP_D"]
        qf = out.take(np.float32, info["qfold_stride"])
        gran = out.take(np.uint64, info["NG"] + 2 * guard)
        dbg = out.take(np.float32, 2, d)
        qs = out.take(np.uint32, H, 64)
        label = f"{dt} fold d {d} {case.family} shift {case.shift_kind}"
        G = gran[guard:]
        written = np.zeros(len(gran), bool)
        for base in (info["O_Y1"], info["O_CQ"]):
            written[guard + base:guard + base + d] = True
        for p in range(info["NP_D"]):
            written[guard + info["O_STAT"] + 16 * p:guard + info["O_STAT"] + 16 * p + 2] = True
        tags = (gran >> np.uint64(32)).astype(np.uint32)
        assert (tags[written] == _layout[dt]["tag"]).all(), f"{label}: granules without the tag"
        assert (gran[~written] == PR.SENT64).all(), f"{label}: granules written that belong to nobody: {np.nonzero((gran != PR.SENT64) & ~written)[0][:8] - guard}"
        val = lambda o, n, step=1: (G[o:o + n * step:step] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
        got = dict(M=qf[:dd].reshape(d, d), d=qf[dd:dd + d], s=qf[dd + d:dd + 2 * d], c=qf[dd + 2 * d:dd + 3 * d], y1=val(info["O_Y1"], d), T=val(info["O_CQ"], d),
                   s1=val(info["O_STAT"], info["NP_D"], 16), s2=val(info["O_STAT"] + 1, info["NP_D"], 16), A0=dbg[0], tq=dbg[1],
                   q=np.concatenate([unpack_pairs(qs[h, :32], dt) + unpack_pairs(qs[h, 32:], dt) for h in range(H)]))
        worst, _ = PR.check_fold(case, got, label)
        for what, v in worst.items():
            if "/" not in what:
                note(dt, f"fold d {d} {case.family} {case.shift_kind} {what}", v)
        print(f"{label}: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items() if "/" not in k) + f"; median |mu s| r / |q| {worst['|mu s| / |q|']:.2f}")
    assert out.at == len(out.raw)
    _session.ran[dt].add(("fold", d))


@pytest.mark.parametrize("d", [128, 384])
def test_fold_arena(driver, tmp_path, d):
    dt, _ = driver
    payload, layers = PR.arena_case(dt, d, 2, 40 + d)
    ran, out = run(driver, [payload], tmp_path)
    w = PR.check_arena(layers, d, out.take(np.float32, 2 * PR.qfold_stride(d)), f"{dt} arena d {d}")
    assert out.at == len(out.raw)
    note(dt, f"arena d {d}", w)
    print(f"{dt} arena d {d}, 2 layers: worst error / bound {w:.4f}")
    _session.ran[dt].add(("arena", d))


def test_every_form_ran_every_shape(driver):
    dt, _ = driver
    wanted = ({("reduce",), ("vocab_deal",)} | {("rows", s) for s in PR.ROW_SHAPES} | {("rows_reg", s) for s in PR.REG_SHAPES}
              | {("fold", d) for d in PR.FOLD_WIDTHS} | {("arena", 128), ("arena", 384)})
    assert len(PR.ROW_SHAPES) == 11
    assert wanted <= _session.ran[dt], sorted(wanted - _session.ran[dt], key=str)


def test_zz_report(driver):
    dt, _ = driver
    for (t, what), w in sorted(_session.worst.items()):
        if t == dt:
            print(f"{dt} {what}: worst error / bound {w:.4f}")
    for (t, family), v in sorted(_amp.items()):
        if t == dt:
            print(f"{dt} run_ln {family}: |mean s| rstd / |result| median {np.median([a for a, _ in v]):.2f}, largest {max(b for _, b in v):.1f}")
    print(f"erff budget of the gelu bound: {PR.ERFF_ULPS} ulp (assumed, see persist_rows_reference.py); u = {U:.3e}")
    print(f"wall time so far {time.time() - _session.state['t0']:.0f} s")
