"""Float64 references, lane maps, input families and DERIVED bounds of the persistent launches' weight-row machinery
(whisper.axera_amd/csrc/decode_persistent_common.hpp: group_sum / wsum / wmax / sum_hi3, rows_load / rows_dot / rows_dot_reg, RowSet,
RowSetF32, qfold_publish, qfold_unit_query) and of the load-time fold arena (decode_persistent.hip: qfold_build_kernel,
qfold_vec_kernel), for tests/test_persist_rows_reference.py (CPU) and tests/test_gpu_persist_rows.py (tests/cpp/persist_rows_driver.cpp).
No tolerance here is taken from a GPU result. u = 2^-24; first-order bounds carry the project's factor 2 for what first order leaves out.

Lane map (rows_load, rows_dot): LPR lanes share a row of K = 8 LPR CH elements; lane j holds chunk i (of CH) as the 8 elements
(j + LPR i) 8 + e. Chain 0 takes the even e, chain 1 the odd e, both in the order i = 0 .. CH - 1, e rising: 4 CH fused
multiply-adds per chain. Then a0 + a1, the log2(LPR) butterfly adds of group_sum<LPR>, and the bias add.

Dot, ref = sum w_i x_i (+ b) in float64 from the exact h16 weights and the fp32 activations: a term passes through at most 4 CH
FMA roundings, one add, log2 LPR tree adds and the bias add, each relative u of a partial sum that sum |w_i x_i| bounds:
    E_dot = 2 (4 CH + 2 + log2 LPR) u sum |w_i x_i| + 2 u |ref|
RowSetF32 (fp32 rows of M) has the same chains: the same bound.

run_ln, res = rstd (W (g . x) - mean s) + c with (g . x), mean, rstd, s, c handed in as fp32:
  (a) against float64 of the same formula on the same fp32 inputs:
      E_a = rstd E_dot + 2 u rstd (|mean s| + |W (g . x) - mean s|) + 2 u |ref|
  (b) against the definition W LN(x) + b with mean, rstd, g . x, s, c in float64 from x, g, beta, W, b. The handed-in values are each
      one fp32 rounding of those: |W| u |g . x| for the products, u |mean| |s| twice (mean and s), u |rstd (..)| for rstd, u |c|:
      E_b = E_a + rstd (u |W| |g . x| + 2 u |mean s|) + u |rstd (W (g . x) - mean s)| + u |c|
      The mean term does not shrink with the result: |mean s| / |ref| is the amplification of this identity, reported per family.

gelu_erf(y) = 0.5 y (1 + erff(y / sqrt 2)) of a value y with bound E_y: |g'| <= 1.13; erff of the ROCm device library within
ERFF_ULPS = 4 ulp (4 u below 1). ASSUMPTION: no accuracy table of the device library is part of this tree; the figure is the one
tests/encoder_kernel_reference.py (EPI_GELU_POS_F32) and tests/gemv_kernel_reference.py already use: the argument carries 2 u, erff
4 u absolute, 1 + erf one rounding, the two products two: under 8 u |y| with the factor 2.   E_g = 1.13 E_y + 8 u |y|

Fold chain (decode_persistent.hip's query fold), every stage against float64 of its own formula on its ACTUAL inputs:
  y1 = W_o a + b_o, A0 = W_cq (g . x0), tq = M a + d (M, d: the fp32 arena as built): E_dot each;  T = tq + A0: one add, 2 u |T|
  tv_i = (x0_i + y1_i) - shift: two roundings, dtv = u |x0 + y1| + u |tv|. Per producer s1 = wsum(tv), s2 = wsum(tv^2), six tree adds:
      ds1 = 2 (sum dtv + 6 u sum |tv|) ; ds2 = 2 (sum (2 |tv| dtv + u tv^2) + 6 u sum tv^2)
  query of a head from the PUBLISHED granules T, s1, s2 and the arena's s, c: t1 = sum s1, t2 = sum s2 (one add + six tree adds),
  dm = t1 / D, var = t2 / D - dm^2, mu = shift + dm, r = (var + 1e-5)^-1/2, q = r (T - mu s) + c:
      ddm = 8 u sum |s1| / D ; dvar = 8 u sum |s2| / D + 2 |dm| ddm + u dm^2 + u |var| ; dr_rel = 0.5 dvar / (var + 1e-5) + 4 u
      dmu = ddm + u |mu| ; E_q = 2 (r (|s| dmu + 2 u |mu s|) + |r (T - mu s)| (dr_rel + 2 u) + u |q|) + pair_err(q)
  pair_err: the h16split2 residual, 2^-16 |q| in bfloat16, 2^-22 |q| (+ 2^-25 below the normal range) in half.
  Against the UNFOLDED definition W_cq LN_cross(x0 + W_o a + b_o) + b_cq in float64 the stage bounds are propagated:
      dT = E_A0 + E_tq + 2 u |T| + |W_cq| u |g . x0| + u (|M| |a| + |d|)      (the rounding of g . x0, of M and d)
      x1 = x0 + y1 with dy = E_y1 per element: dmu' = mean dy ; dvar' = 2 mean(|x1 - mu| (dy + dmu')) + mean((dy + dmu')^2)
      dq = r (dT + (dmu + dmu') |s| + |mu| u |s|) + |r (T - mu s)| (dr_rel + 0.5 dvar' / (var + 1e-5)) + u |c|, on top of E_q.

Arena: every element against float64; the kernels accumulate D terms in double and round once: u |ref| + D 2^-52 sum |terms|.
"""
import os
import re

import numpy as np
import torch

import decode_kernel_reference as R
from encoder_kernel_reference import U32 as U
from encoder_kernel_reference import from_bits, gelu64, round16, to_bits
from gemv_kernel_reference import outlier0_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")
ERFF_ULPS = 4
GELU_SLOPE = 1.13
LN_EPS = 1e-5
SENT64 = np.uint64(0x7FC57FC57FC57FC5)
FAMILIES = ("benign", "realistic", "outlier0")

# persist_dispatch: d_model -> (LD, CD, LF, CF)
SHAPES = {128: (16, 1, 32, 2), 256: (32, 1, 64, 2), 384: (16, 3, 64, 3), 512: (32, 2, 64, 4), 768: (32, 3, 64, 6), 1280: (32, 5, 64, 10)}
ROW_SHAPES_D = tuple((v[0], v[1]) for v in SHAPES.values())
ROW_SHAPES_F = tuple((v[2], v[3]) for v in SHAPES.values() if (v[2], v[3]) not in ROW_SHAPES_D)
ROW_SHAPES = ROW_SHAPES_D + ROW_SHAPES_F  # the 11 distinct (LPR, CH)
REG_SHAPES = tuple(s for s in ROW_SHAPES_D if s[1] <= 3)
FOLD_WIDTHS = (128, 256, 384, 512, 768)
FORMS = ("reduce", "rows", "rows_reg", "fold", "arena")
LINKED = ("decode_persistent", "decode_persistent2")  # the objects the driver links: launch_qfold_build, qfold_floats
ALSO = ("common.hpp", "decode_layout.hpp", "decode_persistent_common.hpp")


def _ints(text, names=None):
    found = {k: int(v) for k, v in re.findall(r"\b([A-Z][A-Z0-9_]*) = (\d+)\b", text)}
    return found if names is None else {k: found[k] for k in names}


def source_layout():
    """The constants of the headers as the SOURCE states them (the driver prints the ones it was compiled with; the GPU test holds
    the two against each other): PT, PL, CT, NCW, DecArena's units, the QF_* vector offsets."""
    common = open(os.path.join(CSRC, "common.hpp")).read()
    pers = open(os.path.join(CSRC, "decode_persistent_common.hpp")).read()
    lay = _ints(common[common.index("struct DecArena {"):].split("static constexpr")[0])
    lay.update(_ints(pers, ("PT", "NPW", "NCW", "QF_SQKV", "QF_CQKV", "QF_SFC1", "QF_CFC1")))
    lay["PL"], lay["CT"] = 64 * lay.pop("NPW"), 64 * lay["NCW"]
    return lay


LAY = source_layout()
CT, PL = LAY["CT"], LAY["PL"]


def qfold_stride(d):
    """M [d][d], then the vectors up to c_fc1 [4 d]."""
    return d * d + (LAY["QF_CFC1"] + 4) * d


# ------------------------------------------------------------------------------------------ reductions
def lane_perms(G):
    """The butterfly partners of group_sum<G>, in its order: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror, then the
    row swaps."""
    l = np.arange(64)
    p = [l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15))]
    if G >= 32:
        p.append(l ^ 16)
    if G >= 64:
        p.append(l ^ 32)
    return p


def emu_group_sum(v, G):
    """float32 [..., 64] -> the sums over aligned groups of G lanes in the butterfly's association order, in every lane."""
    v = np.asarray(v, dtype=np.float32)
    for p in lane_perms(G):
        v = v + v[..., p]
    return v


def emu_sum_hi3(v):
    l = np.arange(64)
    v = np.asarray(v, dtype=np.float32)
    for p in ((l & ~15) | ((l + 8) & 15), l ^ 16, l ^ 32):
        v = v + v[..., p]
    return v


REDUCTIONS = (("group_sum16", 16), ("group_sum32", 32), ("group_sum64", 64), ("wsum", 64), ("wmax", 64), ("sum_hi3", 8))


def reduce_groups(name):
    """lane -> group id of a reduction (sum_hi3: the lanes that share lane & 7)."""
    l = np.arange(64)
    return l & 7 if name == "sum_hi3" else l // dict(REDUCTIONS)[name]


def reduce_vectors(seed=5):
    """(vectors [n][64] float32, kinds): small integers (exact sums), one fp32 pattern, and for wmax a single maximum in each of the
    64 lane positions among lanes at -inf or below it."""
    rng = np.random.default_rng(seed)
    vs, kinds = [], []
    for _ in range(3):
        vs.append(rng.integers(-40, 41, 64).astype(np.float32))
        kinds.append("int")
    vs.append(np.arange(64, dtype=np.float32) * 3 - 70)  # a lane-dependent pattern: a missing butterfly step changes every group
    kinds.append("int")
    vs.append((rng.standard_normal(64) * np.exp(rng.uniform(-6, 6, 64))).astype(np.float32))
    kinds.append("f32")
    for pos in range(64):
        v = np.where(rng.random(64) < 0.5, -np.inf, rng.uniform(-5, 5, 64)).astype(np.float32)
        v[pos] = 7.5
        vs.append(v)
        kinds.append("max")
    return np.stack(vs), kinds


def check_reduce(vs, kinds, got):
    """got [n][6][64]. Returns {name: worst error / bound}."""
    worst = {}
    for vi, (v, kind) in enumerate(zip(vs, kinds)):
        v64 = v.astype(np.float64)
        for ri, (name, G) in enumerate(REDUCTIONS):
            g, grp = got[vi, ri], reduce_groups(name)
            if name == "wmax":
                assert np.array_equal(g, np.full(64, v.max(), np.float32)), (vi, name, g, v.max())
                continue
            if kind == "max":
                continue  # -inf lanes: sums of -inf, only wmax is asked
            for gid in np.unique(grp):
                m = grp == gid
                ref = v64[m].sum()
                assert (g[m].view(np.uint32) == g[m].view(np.uint32)[0]).all(), f"vector {vi} {name} group {gid}: its lanes disagree: {g[m]}"
                if kind == "int":
                    assert g[m][0] == ref, f"vector {vi} {name} group {gid}: {g[m][0]} against {ref}"
                else:
                    bound = np.log2(m.sum()) * U * np.abs(v64[m]).sum()
                    r = abs(float(g[m][0]) - ref) / bound
                    assert r <= 1, f"vector {vi} {name} group {gid}: {g[m][0]} against {ref}: {r:.2f} x its bound"
                    worst[name] = max(worst.get(name, 0.0), r)
    return worst


def emu_reduce(vs):
    out = np.empty((len(vs), 6, 64), np.float32)
    with np.errstate(invalid="ignore"):
        for ri, (name, G) in enumerate(REDUCTIONS):
            if name == "wmax":
                out[:, ri] = vs.max(axis=1, keepdims=True)
            elif name == "sum_hi3":
                out[:, ri] = emu_sum_hi3(vs)
            else:
                out[:, ri] = emu_group_sum(vs, G)
    return out


# ------------------------------------------------------------------------------------------ the dot product
def lane_view(v, LPR, CH):
    """[..., K] -> [..., CH (i), LPR (j), 8 (e)]: element (j + LPR i) 8 + e."""
    return v.reshape(v.shape[:-1] + (CH, LPR, 8))


def emu_rows_dot(W, x, LPR, CH):
    """rows_dot / rows_dot_reg / RowSetF32::run (without the bias) in the kernel's association order: W [R][K] float32 (the exact
    weight values), x [K] float32. fmaf as float32(w x + acc) with the product and sum in float64 (a 35-bit product is exact there)."""
    w, xx = lane_view(W.astype(np.float64), LPR, CH), lane_view(x.astype(np.float64), LPR, CH)
    acc = np.zeros((W.shape[0], LPR, 2), np.float32)
    for i in range(CH):
        for e in range(8):
            acc[:, :, e & 1] = (w[:, i, :, e] * xx[i, :, e] + acc[:, :, e & 1].astype(np.float64)).astype(np.float32)
    v = acc[:, :, 0] + acc[:, :, 1]
    full = np.zeros((W.shape[0], 64), np.float32)
    full[:, :LPR] = v
    return emu_group_sum(full, LPR)[:, 0]


def dot_terms(LPR, CH):
    return 4 * CH + 2 + int(np.log2(LPR))


def dot_expect(W, x, b, LPR, CH):
    """(ref, bound) of W x (+ b): float64."""
    W64, x64 = W.astype(np.float64), x.astype(np.float64)
    ref = W64 @ x64 + (0.0 if b is None else b.astype(np.float64))
    return ref, 2 * dot_terms(LPR, CH) * U * (np.abs(W64) @ np.abs(x64)) + 2 * U * np.abs(ref) + 1e-300


def gelu_expect(y, ey):
    return gelu64(y), GELU_SLOPE * ey + 2 * ERFF_ULPS * U * np.abs(y) + 1e-300


def emu_gelu(y):
    """gelu_erf in float32 with this machine's erff (torch's): the EMULATION's erff, not the device library's."""
    t = torch.from_numpy(np.asarray(y, dtype=np.float32))
    return (np.float32(0.5) * t * (1 + torch.erf(t * np.float32(0.70710678118654752440)))).numpy()


def erff_ulps(n=200001):
    """This machine's float32 erf against float64 on [-4, 4], in units of u (= 1 ulp below 1): what the emulation's erff is worth."""
    x = np.linspace(-4, 4, n).astype(np.float32)
    e32 = torch.erf(torch.from_numpy(x)).numpy().astype(np.float64)
    e64 = torch.erf(torch.from_numpy(x.astype(np.float64))).numpy()
    return float(np.abs(e32 - e64).max() / U)


# ------------------------------------------------------------------------------------------ row dealing
def deal(wg, N, P, first, LPR, NS=0):
    """RowSet::prefetch's (r0, r1) of workgroup wg, which the kernels hand the rotated index rwg = (wg - NS + P) % P."""
    rwg, slots = (wg - NS + P) % P, CT // LPR
    if first < 0:
        return rwg * N // P, (rwg + 1) * N // P
    pidx = rwg - first
    if pidx < 0:
        pidx += P
    if pidx * slots >= N:
        return 0, 0
    return pidx * slots, min(pidx * slots + slots, N)


def deals(N, P, first, LPR, NS=0):
    return np.array([deal(wg, N, P, first, LPR, NS) for wg in range(P)], dtype=np.int64)


def deal_allowed(N, P, first, LPR, NS=0):
    n = np.diff(deals(N, P, first, LPR, NS), axis=1).ravel()
    return bool((n <= 2 * (CT // LPR)).all() and (n <= 64).all() and (first < 0 or (first < P and P * (CT // LPR) >= N)))


def producers(d, P):
    """decode_persistent.hip's packed deals on P workgroups: {name: (N, LPR, first)} of the K = d phases and the K = 4 d phase, and the
    producer counts NP_D, NP_Q, NP_F, NP_F2."""
    LD, CD, LF, CF = SHAPES[d]
    SLD = CT // LD
    NP_D, NP_Q, NP_F, NP_F2 = -(-d // SLD), -(-3 * d // SLD), -(-4 * d // SLD), -(-d // (CT // LF))
    pk_qkv = P - NP_Q if NP_Q <= P else -1
    pk_f = NP_D if (NP_D + NP_F <= P and NP_Q <= P and NP_D + NP_F + NP_Q >= P) else (0 if (NP_F <= P and NP_Q <= P and NP_F + NP_Q >= P) else -1)
    return {"d": (d, LD, 0), "qkv": (3 * d, LD, pk_qkv), "fc1": (4 * d, LD, pk_f), "fc2": (d, LF, 0)}, dict(NP_D=NP_D, NP_Q=NP_Q, NP_F=NP_F, NP_F2=NP_F2)


def grid_of(d):
    return 128 if d == 128 else 256


def even_grids(N, LPR):
    """Grids P <= 256 of the even deal on which some workgroup owns exactly SLOTS, SLOTS + 1 (or, where N has no such grid, the
    smallest count above SLOTS that one has) and 2 SLOTS rows and none more: at most three, preferring grids that do not divide N."""
    slots = CT // LPR
    counts = {P: set(np.diff(deals(N, P, -1, LPR), axis=1).ravel().tolist()) for P in range(1, 257)}
    ok = {P: c for P, c in counts.items() if max(c) <= min(2 * slots, 64)}
    between = sorted({n for c in ok.values() for n in c if slots < n < 2 * slots})
    have = {n for c in ok.values() for n in c}  # (3 d rows on at most 256 workgroups: wide shapes cannot come down to SLOTS rows each)
    want = [slots if slots in have else None, between[0] if between else None, 2 * slots if 2 * slots in have else None]
    grids = []
    for t in want:
        if t is None or any(t in ok[P] for P in grids):
            continue
        cand = sorted((P for P, c in ok.items() if t in c), key=lambda P: (N % P == 0, -len(ok[P] & set(w for w in want if w)), P))
        if cand:
            grids.append(cand[0])
    return grids, want


# ------------------------------------------------------------------------------------------ rows: cases, references, checks
class RowsCase:
    """One set of inputs of the rows form: W [N][K] (h16 values as float32), b, and per phase an activation vector; for run_ln the raw
    x, g, beta and the handed-in fp32 (g . x, mean, rstd, s, c). ref[p], bound[p]: float64 per row; ref_b / bound_b: run_ln against
    the definition."""

    def __init__(self, dt, LPR, CH, N, family, seed):
        self.dt, self.LPR, self.CH, self.N, self.family, self.K = dt, LPR, CH, N, family, 8 * LPR * CH
        K = self.K
        rng = np.random.default_rng(seed)
        if family == "benign":
            x = rng.standard_normal((4, K)).astype(np.float32)
            g, be = rng.uniform(0.5, 1.5, K).astype(np.float32), rng.uniform(-1, 1, K).astype(np.float32)
            W = R.weights(rng, N, K, dt, "benign")
        elif family == "realistic":
            x, g, be, oc = R.realistic_stream(rng, 4, K)
            W = R.weights(rng, N, K, dt, "realistic", oc)
        else:
            x, g, be, oc, swap = outlier0_stream(rng, 4, K)
            W = R.weights(rng, N, K, dt, "realistic", (oc[0], swap))
            W[:, [0, swap]] = W[:, [swap, 0]]
        far = int(np.argmax(np.abs(x.astype(np.float64).mean(axis=1))))  # run_ln gets the draw whose mean is farthest from 0: a mean that
        x[[2, far]] = x[[far, 2]]                                        # happens to vanish would let a lost mean . s pass (discrimination)
        # the bias changes sign from one pass of SLOTS rows to the next: a second pass that took the first pass's bias is off by >= 1
        sign = np.where((np.arange(N) // (CT // LPR)) % 2 == 0, 1.0, -1.0)
        self.W, self.b = W, (sign * rng.uniform(0.5, 1, N)).astype(np.float32)
        self.x, self.g, self.be = x, g, be
        W64, x64 = W.astype(np.float64), x[2].astype(np.float64)
        mean64 = x64.mean()
        rstd64 = 1.0 / np.sqrt(((x64 - mean64) ** 2).mean() + LN_EPS)
        s64, c64 = W64 @ g.astype(np.float64), W64 @ be.astype(np.float64) + self.b.astype(np.float64)
        self.mean, self.rstd = np.float32(mean64), np.float32(rstd64)
        self.s, self.c = s64.astype(np.float32), c64.astype(np.float32)
        self.gx = g * x[2]  # one fp32 rounding per element, as the pollers form it
        self.acts = np.stack([x[0], x[1], self.gx, x[3]])
        # ---- references
        self.ref, self.bound = [None] * 4, [None] * 4
        self.ref[0], self.bound[0] = dot_expect(W, x[0], self.b, LPR, CH)
        self.ref[1], self.bound[1] = dot_expect(W, x[1], None, LPR, CH)
        dot, edot = dot_expect(W, self.gx, None, LPR, CH)
        m, r, s, c = float(self.mean), float(self.rstd), self.s.astype(np.float64), self.c.astype(np.float64)
        core = dot - m * s
        self.ref[2] = r * core + c
        self.bound[2] = r * edot + 2 * U * r * (np.abs(m * s) + np.abs(core)) + 2 * U * np.abs(self.ref[2])
        absdot = np.abs(W64) @ np.abs(self.gx.astype(np.float64))
        self.ref_b = rstd64 * (W64 @ (g.astype(np.float64) * x64) - mean64 * s64) + c64
        self.bound_b = self.bound[2] + r * (U * absdot + 2 * U * np.abs(m * s)) + U * np.abs(r * core) + U * np.abs(c)
        self.amplification = np.abs(m * s) * r / np.maximum(np.abs(self.ref[2]), 1e-300)
        y, ey = dot_expect(W, x[3], self.b, LPR, CH)
        self.pre3 = y
        self.ref[3], self.bound[3] = gelu_expect(y, ey)

    def payload(self):
        return b"".join([to_bits(self.W, self.dt).tobytes(), self.b.tobytes(), self.s.tobytes(), self.c.tobytes(), self.acts.astype(np.float32).tobytes(),
                         np.float32(self.mean).tobytes(), np.float32(self.rstd).tobytes()])

    def emulate(self):
        """[4][N] float32 in the kernel's association order."""
        d = [emu_rows_dot(self.W, self.acts[p], self.LPR, self.CH) for p in range(4)]
        ln = self.rstd * (d[2] - self.mean * self.s) + self.c
        return np.stack([d[0] + self.b, d[1], ln.astype(np.float32), emu_gelu(d[3] + self.b)])

    def perturbed(self, what, P, first, NS=0):
        """{phase: reference under a defect}: what the discrimination test moves."""
        W64, LPR, CH, slots = self.W.astype(np.float64), self.LPR, self.CH, CT // self.LPR
        a64 = self.acts.astype(np.float64)
        m, r, s, c = float(self.mean), float(self.rstd), self.s.astype(np.float64), self.c.astype(np.float64)
        if what == "drop_mean_s":
            return {2: r * (W64 @ a64[2]) + c}
        if what == "bias_of_first_pass":
            b2, s2, c2 = self.b.astype(np.float64).copy(), s.copy(), c.copy()
            for r0, r1 in deals(self.N, P, first, LPR, NS):
                for row1 in range(r0 + slots, r1):
                    b2[row1], s2[row1], c2[row1] = self.b[row1 - slots], s[row1 - slots], c[row1 - slots]
            return {0: W64 @ a64[0] + b2, 2: r * (W64 @ a64[2] - m * s2) + c2}
        if what == "swap_chunks":
            a2 = a64.copy()
            a2[:, 0:8], a2[:, 8:16] = a64[:, 8:16], a64[:, 0:8]
        elif what == "drop_last_lane":
            a2 = lane_view(a64.copy(), LPR, CH)
            a2[:, :, LPR - 1, :] = 0
            a2 = a2.reshape(4, -1)
        else:
            raise KeyError(what)
        return {0: W64 @ a2[0] + self.b, 1: W64 @ a2[1], 2: r * (W64 @ a2[2] - m * s) + c}


def rows_header(LPR, CH, N, P, NS, first, report=0, reuse=0):
    return np.array([1, LPR, CH, N, P, NS, first, report, reuse], dtype=np.int32).tobytes()


def check_rows(case, P, NS, first, own, gran, tag, guard, label=""):
    """own [P][2] int32 and gran [4][guard + N + guard] uint64 of one launch. Tags, guards, ownership, values. Returns
    ({what: worst error / bound}, values [4][N] float32)."""
    N = case.N
    want = deals(N, P, first, case.LPR, NS)
    assert np.array_equal(own, want), f"{label}: prefetch's (r0, r1) differ from the mirror at workgroups {np.nonzero((own != want).any(axis=1))[0][:8]}"
    vals = np.empty((4, N), np.float32)
    worst = {}
    for p in range(4):
        g = gran[p]
        for side, z in (("front", g[:guard]), ("back", g[guard + N:])):
            assert (z == SENT64).all(), f"{label} phase {p}: {side} guard granules written at {np.nonzero(z != SENT64)[0][:8]}"
        body = g[guard:guard + N]
        tags = (body >> np.uint64(32)).astype(np.uint32)
        assert (tags == tag).all(), f"{label} phase {p}: rows without the tag: {np.nonzero(tags != tag)[0][:8]} ({(tags != tag).sum()} of {N})"
        vals[p] = (body & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    return check_rows_values(case, vals, label), vals


PHASES = ("run+bias", "run", "run_ln", "run+gelu")


def check_rows_values(case, vals, label=""):
    """vals [4][N] float32 against the references of the four phases (run_ln against both). Returns {what: worst error / bound}."""
    worst = {}
    for p in range(4):
        refs = [("", case.ref[p], case.bound[p])] + ([(" definition", case.ref_b, case.bound_b)] if p == 2 else [])
        for suffix, ref, bound in refs:
            assert np.isfinite(vals[p]).all(), f"{label} phase {p}: non-finite values"
            ratio = np.abs(vals[p].astype(np.float64) - ref) / bound
            i = int(np.argmax(ratio))
            assert ratio[i] <= 1, (f"{label} phase {PHASES[p]}{suffix}: row {i} {vals[p][i]} against {ref[i]}: error {abs(vals[p][i] - ref[i]):.3e} = "
                                   f"{ratio[i]:.2f} x its bound {bound[i]:.3e}")
            worst[PHASES[p] + suffix] = float(ratio[i])
    return worst


def rows_plan(LPR, CH):
    """What the GPU test launches for a shape: [(name, N, family, [(P, NS, first)])]. K = d shapes: the packed deals of a 2-layer
    model's d, 3 d and 4 d rows on the launch's grid, and 3 d dealt evenly on even_grids; K = 4 d shapes: the packed d rows and the
    even 3 d. Every deal of a group runs on the same inputs."""
    K = 8 * LPR * CH
    if (LPR, CH) in ROW_SHAPES_D:
        d = K
        P = grid_of(d)
        NS = P - 2 * (d // 64)
        pk, _ = producers(d, P)
        even = [(Pe, 0, -1) for Pe in even_grids(3 * d, LPR)[0]]
        return [("d", d, "benign", [(P, NS, pk["d"][2])]), ("3d", 3 * d, "realistic", [(P, NS, pk["qkv"][2])] + even),
                ("4d", 4 * d, "outlier0", [(P, NS, pk["fc1"][2])])]
    d = K // 4
    P = grid_of(d)
    NS = P - 2 * (d // 64)
    pk, _ = producers(d, P)
    assert pk["fc2"][1] == LPR
    return [("d", d, "realistic", [(P, NS, pk["fc2"][2])]), ("3d", 3 * d, "outlier0", [(Pe, 0, -1) for Pe in even_grids(3 * d, LPR)[0]])]


def rows_seed(LPR, CH, name):
    return 1000 * LPR + 10 * CH + len(name)


VOCAB_DEALS = ((51865, 128), (51865, 256), (51866, 128), (51866, 256))  # (N, P) of the report-only deal, (LPR, CH) = (16, 1)
FOLD_CASES = (("benign", "mean"), ("realistic", "mean"), ("outlier0", "mean"), ("realistic", "off"))


def fold_perturbed(case, what=None):
    """The folded identity r (A0 + M a + d - mu s) + c in float64 (what = None: equals the definition), or under a defect of the
    discrimination test."""
    M, dv, s, c = case.arena64(g_role="F_ATTN_LN_W" if what == "attn_g_in_M" else "F_CROSS_LN_W", with_d=what != "drop_d")
    _, _, mu, _, r = case.definition()
    T = case.w_cq.astype(np.float64) @ (case.g.astype(np.float64) * case.x0.astype(np.float64)) + M @ case.a.astype(np.float64) + dv
    return r * (T - (0.0 if what == "drop_mean_s" else mu) * s) + c


# ------------------------------------------------------------------------------------------ the fold
class FoldCase:
    """Inputs of one layer's query fold at width d: W_o, W_cq (h16 values), one layer of DecArena's floats with the LayerNorm vectors of
    the three roles and the biases drawn independently, the layer input x0, the attention vector a, the statistics' shift."""

    def __init__(self, dt, d, family, shift_kind, seed):
        self.dt, self.d, self.family, self.shift_kind = dt, d, family, shift_kind
        self.LD, self.CD = SHAPES[d][:2]
        rng = np.random.default_rng(seed)
        F = LAY
        fl = np.zeros((F["F_UNITS"], d), np.float32)
        if family == "benign":
            x0 = rng.standard_normal(d).astype(np.float32)
            oc = ()
            for k in ("F_ATTN_LN_W", "F_CROSS_LN_W", "F_MLP_LN_W"):
                fl[F[k]] = rng.uniform(0.5, 1.5, d)
            for k in ("F_ATTN_LN_B", "F_CROSS_LN_B", "F_MLP_LN_B"):
                fl[F[k]] = rng.uniform(-1, 1, d)
        else:
            gen = (lambda: R.realistic_stream(rng, 1, d)) if family == "realistic" else (lambda: outlier0_stream(rng, 1, d)[:4])
            x, g, be, oc = gen()
            x0, fl[F["F_CROSS_LN_W"]], fl[F["F_CROSS_LN_B"]] = x[0], g, be
            for kw, kb in (("F_ATTN_LN_W", "F_ATTN_LN_B"), ("F_MLP_LN_W", "F_MLP_LN_B")):
                _, g2, b2, _ = R.realistic_stream(rng, 1, d)
                fl[F[kw]], fl[F[kb]] = g2, b2
        for k, n in (("F_B_QKV", 3), ("F_B_O", 1), ("F_B_CQ", 1), ("F_B_CO", 1), ("F_B_FC1", 4), ("F_B_FC2", 1)):
            fl[F[k]:F[k] + n] = rng.uniform(-1, 1, (n, d))
        wfam = "benign" if family == "benign" else "realistic"
        self.w_o = R.weights(rng, d, d, dt, wfam)
        self.w_cq = R.weights(rng, d, d, dt, wfam, oc)
        self.fl, self.x0 = fl, x0
        self.a = rng.standard_normal(d).astype(np.float32)
        self.g = fl[F["F_CROSS_LN_W"]]
        self.xg = self.g * x0
        m, sd = float(x0.astype(np.float64).mean()), float(x0.astype(np.float64).std())
        self.shift = np.float32(m if shift_kind == "mean" else m + sd)

    def payload(self):
        return b"".join([np.int32(3).tobytes(), np.int32(self.d).tobytes(), to_bits(self.w_o, self.dt).tobytes(), to_bits(self.w_cq, self.dt).tobytes(),
                         self.fl.tobytes(), self.a.tobytes(), self.xg.tobytes(), self.x0.tobytes(), np.float32(self.shift).tobytes()])

    def arena64(self, g_role="F_CROSS_LN_W", with_d=True):
        """float64 M, d, s, c of the layer (g_role: which LayerNorm's gain enters M — the defect of the discrimination test)."""
        F, fl = LAY, self.fl.astype(np.float64)
        wq, wo = self.w_cq.astype(np.float64), self.w_o.astype(np.float64)
        g, be = fl[F["F_CROSS_LN_W"]], fl[F["F_CROSS_LN_B"]]
        M = (wq * fl[F[g_role]]) @ wo
        dv = (wq * g) @ fl[F["F_B_O"]] if with_d else np.zeros(self.d)
        return M, dv, wq @ g, wq @ be + fl[F["F_B_CQ"]]

    def definition(self):
        """q = W_cq LN_cross(x0 + W_o a + b_o) + b_cq in float64, and the pieces the propagated bound needs."""
        F, fl = LAY, self.fl.astype(np.float64)
        y1 = self.w_o.astype(np.float64) @ self.a.astype(np.float64) + fl[F["F_B_O"]]
        x1 = self.x0.astype(np.float64) + y1
        mu, var = x1.mean(), x1.var()
        r = 1.0 / np.sqrt(var + LN_EPS)
        ln = (x1 - mu) * r * fl[F["F_CROSS_LN_W"]] + fl[F["F_CROSS_LN_B"]]
        return self.w_cq.astype(np.float64) @ ln + fl[F["F_B_CQ"]], x1, mu, var, r

    def emulate(self):
        """The chain in float32 in the kernels' association order, from an arena that is the float64 one rounded once. Returns the
        dict check_fold takes."""
        d, LD, CD, slots = self.d, self.LD, self.CD, CT // self.LD
        M, dv, s, c = (v.astype(np.float32) for v in self.arena64())
        b_o = self.fl[LAY["F_B_O"]]
        y1 = emu_rows_dot(self.w_o, self.a, LD, CD) + b_o
        A0 = emu_rows_dot(self.w_cq, self.xg, LD, CD)
        tq = emu_rows_dot(M, self.a, LD, CD) + dv
        T = tq + A0
        tv = (self.x0 + y1) - self.shift
        npd = d // slots
        full = np.zeros((npd, 64), np.float32)
        full[:, :slots] = tv.reshape(npd, slots)
        s1, s2 = emu_group_sum(full, 64)[:, 0], emu_group_sum(full * full, 64)[:, 0]
        q = emu_query(T, s1, s2, s, c, self.shift, d)
        hi, lo = R.pair_split(q, self.dt)
        return dict(M=M, d=dv, s=s, c=c, y1=y1, A0=A0, tq=tq, T=T, s1=s1, s2=s2, q=hi.astype(np.float64) + lo.astype(np.float64))


def emu_query(T, s1, s2, s, c, shift, d):
    """qfold_unit_query's arithmetic in float32 (the statistics summed pairwise, then in a tree)."""
    f = np.float32
    n = len(s1)
    sl = (n + 1) // 2
    lanes1, lanes2 = np.zeros(64, f), np.zeros(64, f)
    for t in range(sl):
        lanes1[32 + t] = s1[t] + (s1[t + sl] if t + sl < n else f(0))
        lanes2[32 + t] = s2[t] + (s2[t + sl] if t + sl < n else f(0))
    t1, t2 = emu_group_sum(lanes1, 64)[0], emu_group_sum(lanes2, 64)[0]
    dm = t1 / f(d)
    var = max(t2 / f(d) - dm * dm, f(0))
    mu, r = f(shift) + dm, f(1.0 / np.sqrt(np.float64(var + f(LN_EPS))))
    return (r * (T - mu * s) + c).astype(f)


def check_fold(case, got, label=""):
    """got: M [d][d], d, s, c (the arena as built), y1, A0, tq, T [d], s1, s2 [NP_D], q [d] (hi + lo, float64). Every stage against
    float64 of its own formula on its actual inputs, the query also against the unfolded definition. Returns {what: worst ratio}."""
    d, LD, CD, dt = case.d, case.LD, case.CD, case.dt
    slots = CT // LD
    npd = d // slots
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    worst = {}

    def hold(what, val, ref, bound):
        assert np.isfinite(f64(val)).all(), f"{label} {what}: non-finite"
        ratio = np.abs(f64(val) - ref) / (bound + 1e-300)
        i = int(np.argmax(ratio))
        assert ratio.flat[i] <= 1, f"{label} {what}: element {i} {f64(val).flat[i]} against {ref.flat[i]}: {ratio.flat[i]:.2f} x its bound {bound.flat[i]:.3e}"
        worst[what] = float(ratio.flat[i])

    b_o = case.fl[LAY["F_B_O"]]
    ry1, ey1 = dot_expect(case.w_o, case.a, b_o, LD, CD)
    hold("y1", got["y1"], ry1, ey1)
    rA0, eA0 = dot_expect(case.w_cq, case.xg, None, LD, CD)
    hold("A0", got["A0"], rA0, eA0)
    rtq, etq = dot_expect(got["M"], case.a, got["d"], LD, CD)
    hold("M a + d", got["tq"], rtq, etq)
    rT = f64(got["tq"]) + f64(got["A0"])
    hold("T", got["T"], rT, 2 * U * np.abs(rT))
    # the statistics, from the y1 that was published
    x1g = f64(case.x0) + f64(got["y1"])
    tv = (x1g - float(case.shift)).reshape(npd, slots)
    dtv = (U * np.abs(x1g)).reshape(npd, slots) + U * np.abs(tv)
    hold("sum(x1 - shift)", got["s1"], tv.sum(1), 2 * (dtv.sum(1) + 6 * U * np.abs(tv).sum(1)))
    hold("sum(x1 - shift)^2", got["s2"], (tv * tv).sum(1), 2 * ((2 * np.abs(tv) * dtv + U * tv * tv).sum(1) + 6 * U * (tv * tv).sum(1)))
    # the query from the published granules
    T, s1, s2, s, c = f64(got["T"]), f64(got["s1"]), f64(got["s2"]), f64(got["s"]), f64(got["c"])
    dm = s1.sum() / d
    var = max(s2.sum() / d - dm * dm, 0.0)
    mu, r = float(case.shift) + dm, 1.0 / np.sqrt(var + LN_EPS)
    core = T - mu * s
    q = r * core + c
    ddm = 8 * U * np.abs(s1).sum() / d
    dvar = 8 * U * np.abs(s2).sum() / d + 2 * abs(dm) * ddm + U * dm * dm + U * abs(var)
    dr_rel = 0.5 * dvar / (var + LN_EPS) + 4 * U
    dmu = ddm + U * abs(mu)
    eq = 2 * (r * (np.abs(s) * dmu + 2 * U * np.abs(mu * s)) + np.abs(r * core) * (dr_rel + 2 * U) + U * np.abs(q)) + R.pair_err(q, dt)
    hold("q from the granules", got["q"], q, eq)
    # the query against the unfolded definition
    qd, x1, mu_d, var_d, r_d = case.definition()
    M64, d64, s64, c64 = case.arena64()
    absWq = np.abs(f64(case.w_cq))
    dT = eA0 + etq + 2 * U * np.abs(rT) + absWq @ (U * np.abs(f64(case.xg))) + U * (np.abs(M64) @ np.abs(f64(case.a)) + np.abs(d64))
    dmu2 = ey1.mean()
    dx = ey1 + dmu2
    dvar2 = 2 * (np.abs(x1 - mu_d) * dx).mean() + (dx * dx).mean()
    eqd = eq + r * (dT + (dmu + dmu2) * np.abs(s64) + abs(mu) * U * np.abs(s64)) + np.abs(r * core) * (dr_rel + 0.5 * dvar2 / (var_d + LN_EPS)) + U * np.abs(c64)
    hold("q against the definition", got["q"], qd, eqd)
    worst["|mu s| / |q|"] = float(np.median(np.abs(mu * s) * r / np.maximum(np.abs(q), 1e-300)))
    return worst, dict(q=q, eq=eq, qd=qd, eqd=eqd, mu=mu, r=r)


def arena_layer_expect(wl, fl, d):
    """One layer of the arena in float64 from the layer's weights wl {unit: [n][d] float32 values} and floats fl [F_UNITS][d]: flat
    (ref, bound) of qfold_stride(d) elements."""
    F, f = LAY, fl.astype(np.float64)
    wq, wo, wqkv, wfc1 = (wl[k].astype(np.float64) for k in ("W_CQ", "W_O", "W_QKV", "W_FC1"))
    g, be = f[F["F_CROSS_LN_W"]], f[F["F_CROSS_LN_B"]]
    eps = d * 2.0 ** -52
    ref, ab = [], []

    def put(r, a):
        ref.append(np.ravel(r))
        ab.append(np.ravel(a))

    put((wq * g) @ wo, (np.abs(wq) * np.abs(g)) @ np.abs(wo))
    put((wq * g) @ f[F["F_B_O"]], (np.abs(wq) * np.abs(g)) @ np.abs(f[F["F_B_O"]]))
    put(wq @ g, np.abs(wq) @ np.abs(g))
    put(wq @ be + f[F["F_B_CQ"]], np.abs(wq) @ np.abs(be) + np.abs(f[F["F_B_CQ"]]))
    ga, ba, gm, bm = f[F["F_ATTN_LN_W"]], f[F["F_ATTN_LN_B"]], f[F["F_MLP_LN_W"]], f[F["F_MLP_LN_B"]]
    bq, b1 = f[F["F_B_QKV"]:F["F_B_QKV"] + 3].ravel(), f[F["F_B_FC1"]:F["F_B_FC1"] + 4].ravel()
    put(wqkv @ ga, np.abs(wqkv) @ np.abs(ga))
    put(wqkv @ ba + bq, np.abs(wqkv) @ np.abs(ba) + np.abs(bq))
    put(wfc1 @ gm, np.abs(wfc1) @ np.abs(gm))
    put(wfc1 @ bm + b1, np.abs(wfc1) @ np.abs(bm) + np.abs(b1))
    ref, ab = np.concatenate(ref), np.concatenate(ab)
    assert len(ref) == qfold_stride(d)
    return ref, U * np.abs(ref) + eps * ab + 1e-300


def arena_case(dt, d, L, seed):
    """(payload, [(wl, fl)] per layer): random weights in every unit, the LayerNorm vectors of the three roles drawn independently."""
    rng = np.random.default_rng(seed)
    F = LAY
    units = {"W_QKV": 3, "W_O": 1, "W_CQ": 1, "W_CO": 1, "W_FC1": 4, "W_FC2": 4}
    layers, wbits, fls = [], [], []
    for _ in range(L):
        arena = np.zeros((F["W_UNITS"] * d, d), np.float32)
        wl = {}
        for k, n in units.items():
            wl[k] = R.weights(rng, n * d, d, dt, "benign")
            arena[F[k] * d:(F[k] + n) * d] = wl[k]
        fl = rng.uniform(-1, 1, (F["F_UNITS"], d)).astype(np.float32)
        for k in ("F_ATTN_LN_W", "F_CROSS_LN_W", "F_MLP_LN_W"):
            fl[F[k]] = rng.uniform(0.5, 1.5, d) * rng.choice([1.0, 3.0])
        layers.append((wl, fl))
        wbits.append(to_bits(arena, dt).tobytes())
        fls.append(fl.tobytes())
    return b"".join([np.int32(4).tobytes(), np.array([d, L], np.int32).tobytes()] + wbits + fls), layers


def check_arena(layers, d, got, label=""):
    worst = 0.0
    for l, (wl, fl) in enumerate(layers):
        ref, bound = arena_layer_expect(wl, fl, d)
        g = got[l * qfold_stride(d):(l + 1) * qfold_stride(d)].astype(np.float64)
        assert np.isfinite(g).all(), f"{label} layer {l}: elements nobody wrote: {np.nonzero(~np.isfinite(g))[0][:8]}"
        ratio = np.abs(g - ref) / bound
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1, f"{label} layer {l}: element {i} {g[i]} against {ref[i]}: {ratio[i]:.2f} x its bound {bound[i]:.3e}"
        worst = max(worst, float(ratio[i]))
    return worst
