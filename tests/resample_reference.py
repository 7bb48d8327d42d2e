"""Float64 reference of the sample-rate conversion (DESIGN.md §11 "Sample rates"; whisper.axera_amd/csrc/resample.hpp states the
same definition for the engine), the per-element bound its float32 implementations are held to, and the cases of the stand-alone
kernel test (tests/test_gpu_resample_kernel.py). numpy only.

Definition, for an input rate `rate`: g = gcd(rate, 16000), L = 16000 / g, M = rate / g; c = ROLLOFF min(1, L / M), W = Z / c,
K = ceil(W), T = 2 K. h(t) = c sinc(c t) I0(BETA sqrt(1 - (t / W)^2)) / I0(BETA) for |t| < W, else 0. H[r][i] = float32(h((i - K + 1)
- r / L)). Output j < n_out = ceil(n L / M): i0 = floor(j M / L), r = (j M) mod L, y_j = sum over i < T of x[i0 + i - K + 1] H[r][i],
x zero outside [0, n). The float64 operation order of h is the one below (x = c t; sin(pi x) / (pi x); the window); the library
follows it, so the two tables differ only by the two libraries' sin and I0.

Bound per output element: gamma(z + 1) sum |x_k| |H_k| with u = 2^-24, gamma(n) = n u / (1 - n u) and z the number of non-zero
products of that element (the error of a float32 sum of z products in any order, fused or not, plus one rounding) — never a constant;
an element without a non-zero product must be 0.
"""
import math

import numpy as np

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
TARGET = 16000
U = 2.0 ** -24
TILE = 256          # kResampleTile (common.hpp)
SPAN = 9472         # kResampleSpan
LDS_TABLE = 2048    # kResampleLdsTable
GUARD = 4096        # the drivers' guard bytes around every allocation
SENT16 = 0x7FC5
SENT32 = np.uint32(0x7FC57FC5)  # a NaN

RATES = {8000: (2, 1, 68), 11025: (640, 441, 68), 12000: (4, 3, 68), 22050: (320, 441, 94), 24000: (2, 3, 102), 32000: (1, 2, 136),
         44100: (160, 441, 187), 48000: (1, 3, 203), 96000: (1, 6, 406)}

CLIP_DTYPE = np.dtype([("in_off", "<i8"), ("out_off", "<i8"), ("tab_off", "<i8"), ("n_in", "<i4"), ("n_out", "<i4"), ("L", "<i4"),
                       ("M", "<i4"), ("K", "<i4"), ("row", "<i4")])  # ResampleClip (common.hpp)


def gamma(n):
    return n * U / (1.0 - n * U)


def plan(rate):
    g = math.gcd(rate, TARGET)
    L, M = TARGET // g, rate // g
    c = ROLLOFF * min(1.0, L / M)
    W = Z / c
    return L, M, int(math.ceil(W))


def n_out_of(n, rate):
    L, M, _ = plan(rate)
    return -((-n * L) // M)


_tables = {}


def table64(rate):
    """H [L][2 K] in float64, before the one rounding."""
    if rate not in _tables:
        L, M, K = plan(rate)
        c = ROLLOFF * min(1.0, L / M)
        W = Z / c
        tau = (np.arange(2 * K, dtype=np.float64) - K + 1)[None, :] - (np.arange(L, dtype=np.float64) / L)[:, None]
        x = c * tau
        px = np.pi * x
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(x == 0.0, 1.0, np.sin(px) / px)
        inside = np.abs(tau) < W
        u = np.where(inside, tau / W, 0.0)
        h = c * sinc * (np.i0(BETA * np.sqrt(1.0 - u * u)) * (1.0 / np.i0(BETA)))
        _tables[rate] = np.where(inside, h, 0.0)
    return _tables[rate]


def table32(rate):
    return table64(rate).astype(np.float32)


def indices(n, rate, n_out=None):
    L, M, K = plan(rate)
    j = np.arange(n_out_of(n, rate) if n_out is None else n_out, dtype=np.int64)
    return (j * M) // L, (j * M) % L


def windows(x, rate, i0, clamp=False):
    """[n_out][2 K]: x[i0 + i - K + 1], zero outside the clip (clamp: the seeded defect)."""
    _, _, K = plan(rate)
    x = np.asarray(x)
    xp = np.pad(x, (K, K + 2), mode="edge" if clamp else "constant")  # (room on each side: the off-by-one defects stay inside)
    return xp[(i0[:, None] + 1) + np.arange(2 * K)[None, :]]


def reference(x, rate, H32=None):
    """-> (y float64 from the float32 table, per-element bound)."""
    H = (table32(rate) if H32 is None else np.asarray(H32)).astype(np.float64)
    i0, r = indices(len(x), rate)
    xw = windows(np.asarray(x, dtype=np.float64), rate, i0)
    hw = H[r]
    prod = xw * hw
    z = np.count_nonzero(prod, axis=1)
    bound = np.where(z > 0, gamma(z + 1) * np.abs(prod).sum(axis=1), 0.0)
    return prod.sum(axis=1), bound


def emulate32(x, rate, defect=None):
    """The sum in float32 in tap order (each step a fused multiply-add, rounded once), with an optional seeded defect."""
    L, M, K = plan(rate)
    H = table32(rate)
    n = len(x)
    n_out = n_out_of(n, rate)
    if defect == "floor n_out":
        n_out = (n * L) // M
    i0, r = indices(n, rate, n_out)
    if defect == "phase + 1":
        r = (r + 1) % L
    if defect == "i0 + 1":
        i0 = i0 + 1
    if defect == "neighbour row":
        r = np.where(r > 0, r - 1, np.minimum(1, L - 1))
    xw = windows(np.asarray(x, dtype=np.float32), rate, i0, clamp=defect == "clamped padding")
    hw = H[r]
    T = 2 * K - (1 if defect == "last tap dropped" else 0)
    acc = np.zeros(n_out, dtype=np.float32)
    for i in range(T):
        acc = (acc.astype(np.float64) + xw[:, i].astype(np.float64) * hw[:, i].astype(np.float64)).astype(np.float32)
    return acc


DEFECTS = ("phase + 1", "i0 + 1", "last tap dropped", "floor n_out", "neighbour row", "clamped padding")


def check(y, x, rate, what=""):
    """y (float32) against the reference of clip x; returns worst error / bound (0 where every bound is 0). Raises AssertionError."""
    ref, bound = reference(x, rate)
    y = np.asarray(y)
    assert y.shape == ref.shape, f"{what}: {y.shape[0]} outputs, the definition gives {ref.shape[0]}"
    err = np.abs(y.astype(np.float64) - ref)
    assert not np.isnan(err).any(), f"{what}: NaN in the output"
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, f"{what}: {bad.size} elements beyond the bound, first j={bad[0]}: got {y[bad[0]]!r}, reference {ref[bad[0]]!r}, bound {bound[bad[0]]:.3e}"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def impulse_expect(n, p, rate):
    """What a unit impulse at p must come back as: the table values themselves."""
    L, M, K = plan(rate)
    i0, r = indices(n, rate)
    i = p - i0 + K - 1
    ok = (i >= 0) & (i < 2 * K)
    return np.where(ok, table32(rate)[r, np.clip(i, 0, 2 * K - 1)], np.float32(0)).astype(np.float32)


# ------------------------------------------------------------------ input families
FAMILIES = ("noise", "impulse", "dc", "zeros")


def family(name, n, seed):
    if name == "noise":
        return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)
    x = np.zeros(n, dtype=np.float32)
    if name == "impulse":
        x[n // 2] = 1.0
    elif name == "dc":
        x[:] = 1.0
    return x


def n_for_outputs(target, rate):
    """The smallest n with n_out >= target (an up-sampling rate cannot give every count: n_out is then target or the next it can give)."""
    L, M, _ = plan(rate)
    n = max(1, ((target - 1) * M) // L)
    while n_out_of(n, rate) < target:
        n += 1
    return n


def lengths(rate):
    K = plan(rate)[2]
    return [1, 2, K, 2 * K + 1] + [n_for_outputs(t, rate) for t in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]


# ------------------------------------------------------------------ launches of the stand-alone kernel test
def sentinel(count, esz=4):
    return np.full(count * esz // 2, SENT16, dtype=np.uint16)


def launch_group(ident, clips, *, placement="packed", stride=0, rows=None, n_rows=0, gaps=(0, 0, 0), tables_short=0, out_short=0,
                 overflow=True):
    """One launch over clips [(rate, x)]. placement "packed": clip b at out_off = what lies before it + gaps[b]; "rows": clip b in
    staging row rows[b] of n_rows rows of `stride`, tails packed into one overflow buffer in clip order (+ 3 unowned entries)."""
    B = len(clips)
    desc = np.zeros(B, dtype=CLIP_DTYPE)
    tabs, tab_off = [], {}
    for rate, _ in clips:
        if rate not in tab_off:
            tab_off[rate] = sum(t.size for t in tabs)
            tabs.append(device_table(rate).ravel())
    io = oo = 0
    over_off = np.zeros(max(n_rows, 1), dtype=np.int64)
    over_total = 0
    for b, (rate, x) in enumerate(clips):
        L, M, K = plan(rate)
        n_out = n_out_of(len(x), rate)
        oo += gaps[b] if placement == "packed" and b < len(gaps) else 0
        desc[b] = (io, oo if placement == "packed" else 0, tab_off[rate], len(x), n_out, L, M, K, rows[b] if rows else 0)
        io += len(x)
        oo += n_out
        if placement == "rows" and n_out > stride:
            over_off[rows[b]] = over_total
            over_total += n_out - stride
    tables = np.concatenate(tabs)
    bufs = {"in": np.concatenate([np.asarray(x, dtype=np.float32) for _, x in clips]), "tables": tables[: tables.size - tables_short],
            "clips": desc}
    p = dict(batch=B, stride=stride, max_out=int(desc["n_out"].max()), **{"in": "in"}, tables="tables", clips="clips", out="out")
    if placement == "packed":
        bufs["out"] = sentinel(oo + 5 - out_short)
    else:
        bufs["out"] = sentinel(n_rows * stride)
        p["n_rows"] = n_rows
        if over_total and overflow:
            bufs["overflow"] = sentinel(over_total + 3)
            bufs["over_off"] = over_off
            p.update(overflow="overflow", over_off="over_off")
    return bufs, [("resample", ident, p, list(bufs))]


def strip(name, got):
    g = GUARD // 2
    got = np.ascontiguousarray(got).view(np.uint16).ravel()
    assert (got[:g] == SENT16).all() and (got[-g:] == SENT16).all(), f"{name}: store into a guard"
    return got[g:-g]


def device_table(rate):
    """The table as the kernel reads it: [L][2 K], or tap-major [2 K][L] where it has several phases and does not fit the LDS copy
    (resample_table_tap_major, common.hpp)."""
    L, _, K = plan(rate)
    H = table32(rate)
    return np.ascontiguousarray(H.T) if table_path(L, K) == "l2" else H


def table_path(L, K):
    return "uniform" if L == 1 else "lds" if L * 2 * K <= LDS_TABLE else "l2"


def verify(cmd, ident, p, state, got, dt, prev=None):
    """Every buffer the launch names against what it held before: outputs inside the bound (impulses exactly the table values),
    everything else the same bits. Returns {label: worst error / bound}."""
    notes = {}
    after = {k: strip(f"{ident} {k}", v) for k, v in got.items()}
    for k in ("in", "tables", "clips", "over_off"):
        if k in after:
            assert np.array_equal(after[k], np.ascontiguousarray(state[k]).view(np.uint16).ravel()), f"{ident}: {k} changed"
    desc = np.ascontiguousarray(state["clips"]).view(CLIP_DTYPE)
    x_all = np.ascontiguousarray(state["in"]).view(np.float32)
    out = after["out"].view(np.uint32).copy()
    over = after["overflow"].view(np.uint32).copy() if "overflow" in after else None
    over_off = np.ascontiguousarray(state["over_off"]).view(np.int64) if "over_off" in state else None
    stride = p["stride"]
    for b, c in enumerate(desc):
        rate = next(r for r in list(RATES) + [88200] if plan(r) == (c["L"], c["M"], c["K"]))
        x = x_all[c["in_off"]: c["in_off"] + c["n_in"]]
        n_out = int(c["n_out"])
        assert n_out == n_out_of(len(x), rate)
        if stride:
            head = min(n_out, stride)
            lo = int(c["row"]) * stride
            y = out[lo: lo + head].copy()
            out[lo: lo + head] = SENT32
            if n_out > stride:
                o = int(over_off[c["row"]])
                y = np.concatenate([y, over[o: o + n_out - stride]])
                over[o: o + n_out - stride] = SENT32
        else:
            lo = int(c["out_off"])
            y = out[lo: lo + n_out].copy()
            out[lo: lo + n_out] = SENT32
        y = y.view(np.float32)
        label = f"{rate} Hz {table_path(c['L'], c['K'])}"
        notes[label] = max(notes.get(label, 0.0), check(y, x, rate, f"{ident} clip {b}"))
        nzp = np.flatnonzero(x)
        if nzp.size == 1 and x[nzp[0]] == 1.0:  # a unit impulse: the table values, exactly
            want = impulse_expect(len(x), int(nzp[0]), rate)
            assert np.array_equal(y, want), f"{ident} clip {b}: an impulse must come back as the table values"
    assert (out == SENT32).all(), f"{ident}: a store outside the clips' outputs ({np.flatnonzero(out != SENT32)[:5]})"
    if over is not None:
        assert (over == SENT32).all(), f"{ident}: a store into the overflow buffer outside the tails"
    return notes


def form_of(cmd, p, qall=None):
    return cmd, "rows" if p["stride"] else "packed"


def grid_of(cmd, p):
    return (p["max_out"] + TILE - 1) // TILE, p["batch"], 1


WANTED_FORMS = {("resample", "rows"), ("resample", "packed")}
KERNEL_RATES = (8000, 12000, 24000, 48000, 44100, 11025)


def rate_case(rate):
    def make(dt):
        return [launch_group(f"r{rate}.n{n}", [(rate, family(f, n, 1000 * k + i)) for i, f in enumerate(FAMILIES)])
                for k, n in enumerate(lengths(rate))]
    return make


def widest_case(dt):
    n = n_for_outputs(TILE + 1, 96000)
    return [launch_group("r96000", [(96000, family("noise", n, 5)), (96000, family("impulse", n, 6))])]


def mixed_case(dt):
    return [launch_group("mixed", [(44100, family("noise", 1000, 7)), (8000, family("dc", 1, 8)),
                                   (48000, family("noise", n_for_outputs(3 * TILE + 1, 48000), 9))])]


def rows_case(dt):
    """The front-end test's edge: staging rows of 8000 samples, two clips whose tails share one overflow buffer, a clip that ends
    inside its row and a row nobody owns."""
    clips = [(48000, family("noise", n_for_outputs(8001, 48000), 10)), (8000, family("noise", 2500, 11)),
             (44100, family("noise", n_for_outputs(12345, 44100), 12))]
    return [launch_group("rows", clips, placement="rows", stride=8000, rows=[0, 3, 1], n_rows=4)]


def packed_case(dt):
    clips = [(12000, family("noise", 700, 13)), (48000, family("dc", 1000, 14)), (44100, family("impulse", 900, 15))]
    return [launch_group("packed", clips, gaps=(3, 1, 7))]


CASES = {f"rate {r}": rate_case(r) for r in KERNEL_RATES}
CASES.update({"rate 96000, the widest span": widest_case, "mixed batch": mixed_case, "staging rows": rows_case,
              "packed offsets": packed_case})


def host_cases():
    """(label, rate, x) of every clip of CASES: what the checker tests run without a GPU."""
    for name, make in CASES.items():
        for bufs, launches in make("bf16"):
            desc = bufs["clips"]
            for b, c in enumerate(desc):
                rate = next(r for r in list(RATES) + [88200] if plan(r) == (c["L"], c["M"], c["K"]))
                yield f"{launches[0][1]} clip {b}", rate, bufs["in"][c["in_off"]: c["in_off"] + c["n_in"]]
