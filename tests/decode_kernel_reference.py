"""Float64 references of the batched decoder step's kernels (whisper.axera_amd/csrc/decode_gemm.hip and decode_attention_kernel
in decoder.hip), the numpy index maps of their layouts, and per-element bounds derived from the arithmetic (no free constants).
tests/encoder_kernel_reference.py supplies the 16-bit conversions, `Expect` and the checker; the notation is the same:
u = 2^-24, u16 = 2^-8 (bfloat16) / 2^-11 (half), hulp(x) = half an ulp of the 16-bit type at |x|. Every bound is first order,
worst case, for a kernel that does the stated arithmetic in fp32 in ANY order.

Pair split (split_bf16): hi = rn16(x), r = x - hi is exact in fp32 (|r| <= u16 |x| and r is a multiple of x's fp32 ulp),
lo = rn16(r): |x - (hi + lo)| <= u16 |r| <= u16^2 |x|, i.e. 16 significant bits in bfloat16 and 22 in half. Half only: below
2^-14 the type is subnormal with spacing 2^-24, so both roundings are absolute, 2^-25 at most; above 65504 it has no values
(inputs stay below; the headroom is reported).            pair_err(x) = u16^2 |x| (+ 2^-25 in half)
A stored pair must also be consistent: |lo| <= hulp(hi) (lo is the remainder of hi's rounding).

Linear layers, y[b][n] = sum_k W[n][k] a[b][k] + bias[n]: W is h16, exact. The input is either a stored pair (then a = hi + lo
exactly and the reference uses exactly that) or the kernel's own LayerNorm output y' with error E_a followed by the split:
ea = E_a + pair_err(|a| + E_a). Products of two 16-bit values are exact in fp32; T terms (2 K: hi and lo; 4 K on the fold rows of
the o launch, whose weights are a pair too), the eight waves' partial sums and the bias are added in fp32 in some order:
    E_y = (|W| ea) + (T + 9) u (|W| (|a| + ea) + |bias|)
  GEPI_STORE, q of GEPI_QKV_CACHE, fold rows A0   E_y
  GEPI_PARTIAL (slice s of ksplit, no bias)       (2 K / ksplit + 9) u |W_s| |a_s|
  GEPI_RESID  out += y                            E_y + u |old| + u |ref|
  GEPI_QKV_CACHE K / V rows (stored as h16)       E_y + hulp(|ref| + E_y), at row off[b] of the clip's own cache
  GEPI_GELU   g(y) = 0.5 y (1 + erf(y / sqrt 2)), |g'| <= 1.13, erff of the device library within 4 ulp (the derivation in
              encoder_kernel_reference.py, EPI_GELU_POS_F32): E_g = 1.13 E_y + 8 u |y|, stored as a pair: + pair_err(|g| + E_g)
  GEPI_LOGITS the dumped logits: E_y. The argmax partial of a workgroup is exact GIVEN the logits the GPU dumped: the maximum of its
              rows and the LOWEST index that holds it.
  stat_part (o launch): s1 = sum of the 16 new residual values xn of a block, q2 = sum (xn - s1 / 16)^2, from values with error E:
              ds1 = sum E + 5 u sum |xn| ; ddm_i = E_i + ds1 / 16 + u |s1 / 16| + u |dm_i| ; dq2 = sum (2 |dm| ddm + ddm^2) + 6 u q2

LayerNorm of a row of K values, y = (x - mean) r g + b, r = (var + 1e-5)^-1/2, S1 = mean |x|, ex2 = mean x^2:
  two passes (act_prep_kernel): the bound of encoder_kernel_reference.py (mean: K u S1; a = x - mean; var = mean a^2).
  ONE pass (the clip-block prologue, the fused cross-attention query): var = ex2 - mean^2. ex2: K squares rounded and summed,
  (K + 2) u ex2; mean^2: 2 |mean| dmean + u mean^2 with dmean = K u S1; the subtraction u var. With |mean| S1 <= ex2 (Cauchy-
  Schwarz) and mean^2 <= ex2:       dvar = ((3 K + 4) kappa + 1) u var,  kappa = ex2 / var  (computed as ((3 K + 4) ex2 + var) u)
  — the cancellation is explicit: the relative error of the variance grows linearly with kappa, a benign row has kappa ~ 1, a row
  with outlier channels < 4 (decode_gemm.hip asserts it), a row shifted by c standard deviations 1 + c^2. Then
  dr_rel = 0.5 dvar / (var + 1e-5) + 4 u,  E = |g| (da r + |a| r dr_rel) + 3 u (|a r g| + |y|),  da = dmean + u |a|.
  Fold rows of the QKV launch: a = ln_w2 x (no statistics): u |a|.

Fused query (decode_attention_kernel<1>): q = Wq LN(x) + bq by fp32 FMA over d terms in four chains and two lane steps:
    dq = |Wq| E_ln + (d + 8) u (|Wq| (|y| + E_ln) + |bq|)
Folded query (<2>), from tq, the block statistics sp[i] = (s1, q2), fold_s, fold_c, all taken as given: mean = sum s1 / d,
m2 = sum (q2 + 16 (s1 / 16 - mean)^2), r = (m2 / d + 1e-5)^-1/2, q = r (tq - mean s) + c:
    dmean = 64 u sum |s1| / d ; ddm = u |s1 / 16| + dmean + u |dm| ; dm2 = sum (32 |dm| ddm + 16 ddm^2 + 3 u t_i) + 64 u sum t_i
    dr_rel = 0.5 dm2 / (m2 + d 1e-5) + 4 u ; dq = r (u |tq| + |s| dmean + 2 u |mean s|) + |r (tq - mean s)| (dr_rel + 2 u) + u |q|

Attention of one (clip, head): s_j = 0.125 q.k_j over keys j < n_keys, p = softmax(s), o = sum_j p_j v_j (K, V h16, exact):
  score: ds_j = 0.125 (sum_d |dq_d| |k_jd| + 65 u sum_d (|q_d| + |dq_d|) |k_jd|) + u |s_j|
  exponentials: __expf(x) = exp2(x log2 e) with v_exp_f32 (1 ulp): the rounding of the product is worth u |x| in the result, the
  instruction 2 u. A term's weight passes through one __expf of its own and the rescaling factors alpha of the block loop, the
  wave merge and the split fold: their arguments add up to at most s_max - s_j, and there are at most C = ceil(cap_blocks / 4) +
  n_split + 2 of them, each with one multiplication:   eps_j = ds_j + u (3 C + 2 (s_max - s_j))
  carried through numerator and denominator:            sum_j p_j eps_j (|v_j| + |o|)
  fp32 sums of n_keys terms in any order, the merges, the division: (n_keys + C + 3) u PV,  PV = sum_j p_j |v_j|
  The first-order terms carry a factor 2 for what first order leaves out. Pair output: + pair_err(|o| + E). Partial output
  (m, l, o[64] per split): m is the maximum of the split's computed scores: |m - s_max| <= max_j ds_j; o / l is the split's own
  attention under the same bound; a split without a key records m = -inf, l = 0, o = 0 exactly.
"""
import numpy as np
import torch

from encoder_kernel_reference import (GUARD, SENT16, U32, Expect, check, check_values, from_bits, gelu64, hulp, mm64, round16, sentinel,
                                      to_bits, u16)

GEPI_STORE, GEPI_GELU, GEPI_RESID, GEPI_QKV_CACHE, GEPI_LOGITS, GEPI_PARTIAL = range(6)
LN_EPS = 1e-5
PART = 66  # floats of a split record: m, l, o[64]


# ------------------------------------------------------------------------------------------ layouts
def frag_index(row, k, nbs):
    """activation pair: element of a[clip = row][k] in the fragment-major layout with nbs allocated clip blocks."""
    row, k = np.asarray(row), np.asarray(k)
    tile = (k >> 5) * nbs + (row >> 4)
    return (tile * 64 + ((k >> 3) & 3) * 16 + (row & 15)) * 8 + (k & 7)


def wfrag_index(row, k, KS):
    """packed weights: element of W[row][k], KS = K / 32 k-steps per row block."""
    row, k = np.asarray(row), np.asarray(k)
    tile = (row >> 4) * KS + (k >> 5)
    return (tile * 64 + ((k >> 3) & 3) * 16 + (row & 15)) * 8 + (k & 7)


def pack_weight(w, fill=0):
    """[N][K] array -> fragment-major [ceil(N / 16) * 16 * K], rows >= N filled (the packing kernels write zeros)."""
    N, K = w.shape
    out = np.full((N + 15) // 16 * 16 * K, fill, dtype=w.dtype)
    out[wfrag_index(np.arange(N)[:, None], np.arange(K)[None, :], K // 32)] = w
    return out


def unpack_weight(wp, N, K):
    return wp[wfrag_index(np.arange(N)[:, None], np.arange(K)[None, :], K // 32)]


def kcache_index(step, dd, variant=None):
    """blocked self-/cross-K of one (clip, head): key `step`, dimension dd."""
    step, dd = np.asarray(step), np.asarray(dd)
    if variant == "swap":  # seeded defect 7
        return (step & 63) * 4096 + (dd >> 3) * 512 + (step >> 6) * 8 + (dd & 7)
    return (step >> 6) * 4096 + (dd >> 3) * 512 + (step & 63) * 8 + (dd & 7)


def vcache_index(step, dd):
    return np.asarray(step) * 64 + np.asarray(dd)


def ksplit_for(K):
    """Engine::enqueue_decode_step_batched's choice of K slices for a residual GEMM."""
    KS = K // 32
    for k in (4, 3, 2):
        if KS % k == 0 and KS // k >= 8:
            return k
    return 1


def logits_resident_ok(K, batch):
    ch, nb = (K // 32 + 7) // 8, (min(batch, 64) + 15) // 16
    return K % 128 == 0 and ch <= 5 and ch * nb <= 15


def dgemm_grid(N, rt):
    return min((N + 15) // 16, 256) if rt == 0 else (N + 16 * rt - 1) // (16 * rt)


# ------------------------------------------------------------------------------------------ the pair
def pair_split(x, dt):
    """float32 array -> (hi, lo) float32, as split_bf16 does it."""
    x = np.asarray(x, dtype=np.float32)
    hi = round16(x, dt)
    return hi, round16(x - hi, dt)


def pair_err(ax, dt):
    return u16(dt) ** 2 * np.abs(ax) + (2.0 ** -25 if dt == "f16" else 0.0)


def pair_bits(x, dt):
    hi, lo = pair_split(x, dt)
    return to_bits(hi, dt), to_bits(lo, dt)


def frag_pair(x, nbs, dt, fill=SENT16):
    """fp32 [batch][K] -> the two fragment-major uint16 arrays ([K / 32][nbs][512]); clips >= batch hold `fill`."""
    B, K = x.shape
    hi, lo = pair_bits(x, dt)
    idx = frag_index(np.arange(B)[:, None], np.arange(K)[None, :], nbs)
    out = []
    for a in (hi, lo):
        f = np.full((K + 31) // 32 * nbs * 512, fill, dtype=np.uint16)
        f[idx] = a
        out.append(f)
    return out


def unfrag_pair(hi_bits, lo_bits, B, K, nbs, dt):
    """float64 [batch][K] value hi + lo of a stored pair."""
    idx = frag_index(np.arange(B)[:, None], np.arange(K)[None, :], nbs)
    return from_bits(hi_bits[idx], dt) + from_bits(lo_bits[idx], dt)


class PairExpect:
    """A fragment-major pair output: ref / bound of hi + lo at the written elements, the initial bits of both arrays elsewhere."""

    def __init__(self, n):
        self.ref, self.bound, self.written = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)

    def put(self, idx, ref, bound):
        idx = np.asarray(idx).ravel()
        assert not self.written[idx].any() and np.unique(idx).size == idx.size, "the reference writes an element twice"
        self.ref[idx], self.bound[idx], self.written[idx] = np.asarray(ref).ravel(), np.asarray(bound).ravel(), True


def check_pair(name, hi_bits, lo_bits, init_hi, init_lo, exp, dt):
    """hi_bits / lo_bits: uint16 dumps with guards. Returns the worst error / bound of hi + lo."""
    g = GUARD // 2
    vals = []
    for what, got, init in (("hi", hi_bits, init_hi), ("lo", lo_bits, init_lo)):
        got = np.ascontiguousarray(got).view(np.uint16).ravel()
        assert (got[:g] == SENT16).all() and (got[-g:] == SENT16).all(), f"{name} {what}: store into a guard"
        got = got[g:-g]
        init = np.ascontiguousarray(init).view(np.uint16).ravel()
        assert got.size == init.size == exp.written.size, (name, got.size, init.size, exp.written.size)
        bad = np.nonzero((got != init) & ~exp.written)[0]
        assert bad.size == 0, f"{name} {what}: {bad.size} elements outside the valid output changed, first at element {bad[0]}"
        vals.append(from_bits(got, dt))
    w = exp.written
    if not w.any():  # every clip of the launch was finished
        return 0.0
    hi, lo = vals[0][w], vals[1][w]
    assert np.isfinite(hi).all() and np.isfinite(lo).all(), f"{name}: a non-finite pair element"
    assert (np.abs(lo) <= hulp(hi, dt) * (1 + 2.0 ** -20)).all(), f"{name}: lo is not the remainder of hi's rounding"
    assert (exp.bound[w] > 0).all(), f"{name}: a zero bound"
    return check_values(name, hi + lo, exp.ref[w], exp.bound[w])


# ------------------------------------------------------------------------------------------ LayerNorm
def ln_expect(x64, g, b, onepass, dx=None):
    """x64 float64 [rows][K] (dx: its error). Returns (y, E_y, kappa) — unrounded fp32 result, its bound, ex2 / var per row."""
    K = x64.shape[1]
    dx = np.zeros_like(x64) if dx is None else dx
    g64, b64 = g.astype(np.float64), b.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    a = x64 - mean
    var = (a * a).mean(1, keepdims=True)
    ex2 = (x64 * x64).mean(1, keepdims=True)
    r = 1.0 / np.sqrt(var + LN_EPS)
    y = a * r * g64 + b64
    dmean = K * U32 * np.abs(x64).mean(1, keepdims=True) + dx.mean(1, keepdims=True)
    da = dmean + U32 * np.abs(a) + dx
    if onepass:
        dvar = ((3 * K + 4) * ex2 + var) * U32 + 2 * (np.abs(x64) * dx).mean(1, keepdims=True)
    else:
        dvar = 2 * (np.abs(a) * da).mean(1, keepdims=True) + (da * da).mean(1, keepdims=True) + (K + 4) * U32 * var
    dr_rel = 0.5 * dvar / (var + LN_EPS) + 4 * U32
    e = np.abs(g64) * (da * r + np.abs(a) * r * dr_rel) + 3 * U32 * (np.abs(a * r * g64) + np.abs(y))
    return y, e, (ex2 / np.maximum(var, 1e-300)).ravel()


LN_FAMILIES = ("benign", "outlier", "shift4", "shift100", "small")


def ln_rows(rng, B, K, families=LN_FAMILIES):
    """fp32 [B][K], clip b of family families[b % len]: N(0, 1); three outlier channels at |x| 150-500 (kappa < 4); shifted by
    sqrt(3) / sqrt(99) standard deviations (kappa = 4: the asserted ceiling, and 100); 0.01 N(0, 1) (eps matters)."""
    x = rng.standard_normal((B, K))
    ch = rng.choice(K, 3, replace=False)
    big = rng.uniform(150, 500, 3) * rng.choice([-1, 1], 3)
    for b in range(B):
        f = families[b % len(families)]
        if f == "outlier":
            x[b, ch] += big
        elif f == "shift4":
            x[b] = (x[b] - x[b].mean()) / x[b].std() + np.sqrt(3.0)
        elif f == "shift100":
            x[b] = (x[b] - x[b].mean()) / x[b].std() + np.sqrt(99.0)
        elif f == "small":
            x[b] *= 0.01
    return x.astype(np.float32)


def realistic_stream(rng, B, K):
    """The residual stream, LayerNorm gains and bias as modelgen's kind='realistic' has them (tools/modelgen.py,
    realistic_weights): an outlier channel at 0.75 * 14 sqrt(d) (1 +- 0.2), log-normal gains centred at 4 with hot channels at
    12-30 and 0.02-0.1 on the outlier channels, biases N(0, 0.02) with a few at +-2; the non-outlier part has spread 3."""
    x = rng.standard_normal((B, K)) * 3.0
    oc = rng.choice(np.arange(1, K), 2, replace=False)
    x[:, oc[0]] += 0.75 * 14.0 * np.sqrt(K) * (1.0 + 0.2 * np.sin(np.arange(B) / 7.0))
    x[:, oc[1]] -= 14.0 * np.sqrt(K)
    g = 4.0 * np.exp(rng.standard_normal(K) * 0.6)
    hot = rng.choice(K, max(1, K // 96), replace=False)
    g[hot] = rng.uniform(12.0, 30.0, len(hot))
    g = np.clip(g, 0.05, 30.0)
    g[oc] = rng.uniform(0.02, 0.1, 2)
    b = rng.standard_normal(K) * 0.02
    hb = rng.choice(K, max(1, K // 128), replace=False)
    b[hb] = rng.uniform(-2.0, 2.0, len(hb))
    return x.astype(np.float32), g.astype(np.float32), b.astype(np.float32), oc


def weights(rng, N, K, dt, family="benign", small_cols=()):
    """h16 weight values [N][K] (float32, representable): 0.05 U(-1, 1), or N(0, 0.02) with small columns on the outlier channels."""
    w = rng.uniform(-1, 1, (N, K)) * 0.05 if family == "benign" else rng.standard_normal((N, K)) * 0.02
    for c in small_cols:
        w[:, c] *= 0.05
    return round16(w, dt)


# ------------------------------------------------------------------------------------------ linear layers
def _linear(a, ea, W, bias, terms):
    ref = mm64(a, W) + bias
    bound = mm64(ea, np.abs(W)) + (terms + 9) * U32 * (mm64(np.abs(a) + ea, np.abs(W)) + np.abs(bias))
    return ref, bound


def _inputs(p, bufs, dt):
    """(a, ea, a2, kappa) of a cgemm / dgemm launch: the activations the MFMAs see, their error, and for the LayerNorm-prologue
    launch with fold rows the second input ln_w2 . x."""
    B, K = p["batch"], p["K"]
    if p.get("ln_w"):
        x = bufs[p["x"]].astype(np.float64).reshape(-1, K)[:B]
        y, e, kappa = ln_expect(x, bufs[p["ln_w"]], bufs[p["ln_b"]], onepass=True)
        a2 = None
        if p.get("ln_w2"):
            y2 = x * bufs[p["ln_w2"]].astype(np.float64)
            e2 = U32 * np.abs(y2)
            a2 = (y2, e2 + pair_err(np.abs(y2) + e2, dt))
        return y, e + pair_err(np.abs(y) + e, dt), a2, kappa
    a = unfrag_pair(bufs[p["a_hi"]], bufs[p["a_lo"]], B, K, p["nbs"], dt)
    return a, np.zeros_like(a), None, None


def _cache_put(out, p, bufs, dt, ref, bound):
    """K / V rows of GEPI_QKV_CACHE: ref / bound [B][2 d] (K columns, then V columns)."""
    B, d, bs, Tc = p["batch"], p["d_model"], p["kv_batch_stride"], p["n_ctx_pad"]
    off = bufs[p["off"]].astype(np.int64)[:B, None]
    c = np.arange(d)[None, :]
    head, dd = c >> 6, c & 63
    base = np.arange(B)[:, None] * bs + head * Tc * 64
    bound = bound + hulp(np.abs(ref) + bound, dt)
    out[p["k_cache"]].put(base + kcache_index(off, dd), ref[:, :d], bound[:, :d])
    out[p["v_cache"]].put(base + vcache_index(off, dd), ref[:, d:], bound[:, d:])


def _stat_expect(xn, e):
    """(s1, q2) per 16-row block of new residual rows xn [B][n] with error e, and their bounds."""
    B, n = xn.shape
    xb, eb = xn.reshape(B, n // 16, 16), e.reshape(B, n // 16, 16)
    s1 = xb.sum(2)
    ds1 = eb.sum(2) + 5 * U32 * np.abs(xb).sum(2)
    dm = xb - s1[..., None] / 16
    ddm = eb + (ds1 / 16 + U32 * np.abs(s1) / 16)[..., None] + U32 * np.abs(dm)
    q2 = (dm * dm).sum(2)
    dq2 = (2 * np.abs(dm) * ddm + ddm * ddm).sum(2) + 6 * U32 * q2
    return np.stack([s1, q2], 2), np.stack([ds1, dq2], 2)


def gemm_expect(p, bufs, dt):
    """A cgemm or dgemm launch: p holds the driver's keys (scalars, and buffer names for pointer fields), bufs the initial content
    of every buffer (uint16 bits for h16, float32, int32). Returns ({buffer name: Expect}, {(hi name, lo name): PairExpect}, info)."""
    N, K, B, nbs, epi = p["N"], p["K"], p["batch"], p["nbs"], p["epilogue"]
    bufs = typed(p, bufs)
    fr0 = p.get("fold_row0", 0)
    W = from_bits(unpack_weight(bufs[p["W"]], N, K), dt)
    bias = bufs[p["bias"]].astype(np.float64) if p.get("bias") else np.zeros(N)
    a, ea, a2, kappa = _inputs(p, bufs, dt)
    out, pairs = {}, {}
    for key, size in (("out", 4), ("out2", 4), ("stat_part", 4), ("k_cache", 2), ("v_cache", 2), ("logits_dump", 4)):
        if p.get(key):
            out[p[key]] = Expect(np.ascontiguousarray(bufs[p[key]]).view(np.uint16).ravel(), size)
    bi, ni = np.arange(B)[:, None], np.arange(N)[None, :]
    if epi == GEPI_PARTIAL:
        ks, pb = p["ksplit"], p["part_batch"]
        for s in range(ks):
            sl = slice(s * K // ks, (s + 1) * K // ks)
            ref, bound = _linear(a[:, sl], ea[:, sl], W[:, sl], np.zeros(N), 2 * K // ks)
            out[p["out"]].put((s * pb + bi) * N + ni, ref, bound)
        return out, pairs, dict(kappa=kappa)
    nx = fr0 if fr0 else N
    ref, bound = _linear(a, ea, W[:nx], bias[:nx], 2 * K)
    ref2 = None
    if fr0 and a2 is not None:    # QKV launch: fold rows against ln_w2 . x
        ref2, bound2 = _linear(a2[0], a2[1], W[fr0:], bias[fr0:], 2 * K)
    elif fr0:                     # o launch: fold rows with the (hi, lo) weight pair
        Wl = from_bits(unpack_weight(bufs[p["W_lo"]], N - fr0, K), dt)
        ref2, bound2 = _linear(a, ea, W[fr0:] + Wl, bias[fr0:], 4 * K)
    if epi == GEPI_STORE:
        out[p["out"]].put(bi * N + ni, ref, bound)
    elif epi == GEPI_RESID:
        old = bufs[p["out"]].astype(np.float64).reshape(-1)[:B * nx].reshape(B, nx)
        xn = old + ref
        exn = bound + U32 * np.abs(old) + U32 * np.abs(xn)
        out[p["out"]].put(bi * nx + np.arange(nx)[None, :], xn, exn)
        if fr0:
            old2 = bufs[p["out2"]].astype(np.float64).reshape(-1)[:B * (N - fr0)].reshape(B, N - fr0)
            out[p["out2"]].put(bi * (N - fr0) + np.arange(N - fr0)[None, :], old2 + ref2, bound2 + U32 * np.abs(old2) + U32 * np.abs(old2 + ref2))
        if p.get("stat_part"):
            st, dst = _stat_expect(xn, exn)
            out[p["stat_part"]].put(np.arange(st.size), st, dst + 1e-300)
    elif epi == GEPI_GELU:
        g = gelu64(ref)
        eg = 1.13 * bound + 8 * U32 * np.abs(ref)
        pe = PairExpect(bufs[p["out_hi"]].size)
        pe.put(frag_index(bi, ni, nbs), g, eg + pair_err(np.abs(g) + eg, dt))
        pairs[p["out_hi"], p["out_lo"]] = pe
    elif epi == GEPI_QKV_CACHE:
        d = p["d_model"]
        out[p["out"]].put(bi * d + np.arange(d)[None, :], ref[:, :d], bound[:, :d])
        _cache_put(out, p, bufs, dt, ref[:, d:3 * d], bound[:, d:3 * d])
        if fr0:
            out[p["out2"]].put(bi * d + np.arange(d)[None, :], ref2, bound2)
    elif epi == GEPI_LOGITS:
        wrote = (bufs[p["off"]][:B] >= p["skip_before_step"]).any()
        if p.get("logits_dump") and wrote:
            out[p["logits_dump"]].put(bi * p["logits_dump_stride"] + ni, ref, bound)
        return out, pairs, dict(kappa=kappa, wrote=bool(wrote), logits=ref, bound=bound)
    else:
        raise ValueError(epi)
    return out, pairs, dict(kappa=kappa, fold_in=None if a2 is None else np.abs(a2[0]).max())


def argmax_expect(logits, N, rt, grid, last=False):
    """Per workgroup (max, lowest index holding it) of fp32 logits [B][N] as the GPU dumped them. rt >= 1: workgroup w owns rows
    [16 rt w, 16 rt (w + 1)); rt == 0: the 16-row blocks w, w + grid, ..."""
    B = logits.shape[0]
    val, idx = np.full((B, grid), -np.inf, np.float32), np.full((B, grid), 0x7FFFFFFF, np.int32)
    n = np.arange(N)
    owner = (n // 16) % grid if rt == 0 else n // (16 * rt)
    for w in range(grid):
        rows = n[owner == w]
        if rows.size == 0:
            continue
        sub = logits[:, rows]
        val[:, w] = sub.max(1)
        hit = sub == val[:, w:w + 1]
        idx[:, w] = rows[(hit.shape[1] - 1 - np.argmax(hit[:, ::-1], 1)) if last else np.argmax(hit, 1)]
    return val, idx


def actprep_expect(p, bufs, dt):
    """launch_act_prep: ({x buffer: Expect}, {(hi, lo): PairExpect})."""
    B, K, nbs, n_part, pb, do_ln = p["batch"], p["K"], p["nbs"], p["n_part"], p.get("part_batch", 0), p["do_ln"]
    bufs = typed(p, bufs)
    x = bufs[p["x"]].astype(np.float64).reshape(-1, K)[:B]
    ex = Expect(np.ascontiguousarray(bufs[p["x"]]).view(np.uint16).ravel(), 4)
    dx = np.zeros_like(x)
    if n_part:
        part = bufs[p["part"]].astype(np.float64)
        parts = np.stack([part[(s * pb) * K:(s * pb + B) * K].reshape(B, K) for s in range(n_part)])
        pbias = bufs[p["part_bias"]].astype(np.float64)
        mag = np.abs(x) + np.abs(pbias) + np.abs(parts).sum(0)
        x = x + pbias + parts.sum(0)
        dx = (n_part + 1) * U32 * mag
        ex.put(np.arange(B * K), x, dx + U32 * np.abs(x))
    if do_ln:
        y, e, _ = ln_expect(x, bufs[p["g"]], bufs[p["be"]], onepass=False, dx=dx)
    else:
        y, e = x, dx
    pe = PairExpect(bufs[p["hi"]].size)
    pe.put(frag_index(np.arange(B)[:, None], np.arange(K)[None, :], nbs), y, e + pair_err(np.abs(y) + e, dt))
    return {p["x"]: ex}, {(p["hi"], p["lo"]): pe}


# ------------------------------------------------------------------------------------------ attention
def kv_natural(bits, B, H, cap, stride, dt, blocked):
    """[B][H][cap * 64 keys][64] float64 of a blocked K or row-major V buffer."""
    key, dd = np.arange(cap * 64)[:, None], np.arange(64)[None, :]
    idx = kcache_index(key, dd) if blocked else vcache_index(key, dd)
    base = np.arange(B)[:, None, None, None] * stride + np.arange(H)[None, :, None, None] * cap * 4096
    return from_bits(bits[base + idx[None, None]], dt)


def kv_store(nat, stride, dt, blocked, fill):
    """the inverse: natural [B][H][keys][64] float -> bits of a buffer of B * stride elements (`fill` elsewhere)."""
    B, H, T, _ = nat.shape
    key, dd = np.arange(T)[:, None], np.arange(64)[None, :]
    idx = kcache_index(key, dd) if blocked else vcache_index(key, dd)
    base = np.arange(B)[:, None, None, None] * stride + np.arange(H)[None, :, None, None] * T * 64
    out = np.full(B * stride, fill, dtype=np.uint16)
    out[base + idx[None, None]] = to_bits(nat, dt).reshape(nat.shape)
    return out


def query_expect(p, bufs, dt):
    """(q, dq) float64 [B][d] of an attention launch, by its query mode."""
    B, d = p["batch"], p["d_model"]
    if p.get("tq"):
        tq = bufs[p["tq"]].astype(np.float64).reshape(-1)[:B * d].reshape(B, d)
        sp = bufs[p["stat_part"]].astype(np.float64).reshape(-1)[:B * (d // 16) * 2].reshape(B, d // 16, 2)
        s, c = bufs[p["fold_s"]].astype(np.float64), bufs[p["fold_c"]].astype(np.float64)
        s1, q2 = sp[..., 0], sp[..., 1]
        mean = s1.sum(1, keepdims=True) / d
        dmean = 64 * U32 * np.abs(s1).sum(1, keepdims=True) / d
        dm = s1 / 16 - mean
        ddm = U32 * np.abs(s1) / 16 + dmean + U32 * np.abs(dm)
        t = q2 + 16 * dm * dm
        m2 = t.sum(1, keepdims=True)
        dm2 = (32 * np.abs(dm) * ddm + 16 * ddm * ddm + 3 * U32 * np.abs(t)).sum(1, keepdims=True) + 64 * U32 * np.abs(t).sum(1, keepdims=True)
        r = 1.0 / np.sqrt(m2 / d + LN_EPS)
        dr_rel = 0.5 * dm2 / (m2 + d * LN_EPS) + 4 * U32
        core = tq - mean * s
        q = r * core + c
        dq = r * (U32 * np.abs(tq) + np.abs(s) * dmean + 2 * U32 * np.abs(mean * s)) + np.abs(r * core) * (dr_rel + 2 * U32) + U32 * np.abs(q)
        return q, dq
    if p.get("wq"):
        x = bufs[p["x"]].astype(np.float64).reshape(-1)[:B * d].reshape(B, d)
        y, e, _ = ln_expect(x, bufs[p["ln_w"]], bufs[p["ln_b"]], onepass=True)
        Wq = from_bits(bufs[p["wq"]], dt).reshape(d, d)
        bq = bufs[p["bq"]].astype(np.float64)
        q = mm64(y, Wq) + bq
        return q, mm64(e, np.abs(Wq)) + (d + 8) * U32 * (mm64(np.abs(y) + e, np.abs(Wq)) + np.abs(bq))
    q = bufs[p["q"]].astype(np.float64).reshape(-1)[:B * d].reshape(B, d)
    return q, np.zeros_like(q)


def softmax_expect(q, dq, k, v, chain):
    """One (clip, head), one key range: q, dq [64]; k, v [n][64] float64. Returns (o, E_o, s_max, max ds) — E_o without the
    output's own rounding."""
    n = k.shape[0]
    s = 0.125 * (k @ q)
    ak = np.abs(k)
    ds = 0.125 * (ak @ dq + 65 * U32 * (ak @ (np.abs(q) + dq))) + U32 * np.abs(s)
    smax = s.max()
    w = np.exp(s - smax)
    pr = w / w.sum()
    o = pr @ v
    av = np.abs(v)
    pv = pr @ av
    eps = ds + U32 * (3 * chain + 2 * (smax - s))
    pe = pr * eps
    first = pe @ av + pe.sum() * np.abs(o) + (n + chain + 3) * U32 * pv
    return o, 2 * first + 1e-300, smax, ds.max()


def attn_expect(p, bufs, dt):
    """launch_decode_attention. Returns dict: pair (PairExpect or None), part ([B][H][n_split] records: None for an empty split,
    else (o, E, smax, dsmax)), active [B], n_keys [B]."""
    B, H, d, cap, ns = p["batch"], p["n_head"], p["d_model"], p["cap_blocks"], p.get("n_split", 1)
    bufs = typed(p, bufs)
    done = bufs[p["done"]][:B] != 0
    n_keys = np.full(B, p["n_keys"]) if p["n_keys"] >= 0 else bufs[p["off"]][:B].astype(np.int64) + 1
    q, dq = query_expect(p, bufs, dt)
    k = kv_natural(bufs[p["k"]], B, H, cap, p["kv_batch_stride"], dt, True)
    v = kv_natural(bufs[p["v"]], B, H, cap, p["kv_batch_stride"], dt, False)
    chain = (cap + 3) // 4 + ns + 2
    res = dict(pair=None, part=None, active=~done, n_keys=n_keys)
    if p.get("out_hi"):
        pe = PairExpect(bufs[p["out_hi"]].size)
        for b in np.nonzero(~done)[0]:
            for h in range(H):
                o, e, _, _ = softmax_expect(q[b, h * 64:h * 64 + 64], dq[b, h * 64:h * 64 + 64], k[b, h, :n_keys[b]], v[b, h, :n_keys[b]], chain)
                pe.put(frag_index(b, h * 64 + np.arange(64), p["nbs"]), o, e + pair_err(np.abs(o) + e, dt))
        res["pair"] = pe
    else:
        bps = (cap + ns - 1) // ns
        part = {}
        for b in np.nonzero(~done)[0]:
            for h in range(H):
                for s in range(ns):
                    lo_k, hi_k = min(s * bps * 64, n_keys[b]), min(min(cap, (s + 1) * bps) * 64, n_keys[b])
                    part[b, h, s] = None if hi_k <= lo_k else softmax_expect(q[b, h * 64:h * 64 + 64], dq[b, h * 64:h * 64 + 64],
                                                                             k[b, h, lo_k:hi_k], v[b, h, lo_k:hi_k], chain)
        res["part"] = part
    return res


def check_attn_part(name, got_bits, init_bits, p, res):
    """The partial-record output [B][H][n_split][66] of a launch against attn_expect's result. Returns the worst error / bound."""
    g = GUARD // 2
    got_bits = np.ascontiguousarray(got_bits).view(np.uint16).ravel()
    assert (got_bits[:g] == SENT16).all() and (got_bits[-g:] == SENT16).all(), f"{name}: store into a guard"
    got = got_bits[g:-g].view(np.float32)
    init = np.ascontiguousarray(init_bits).view(np.uint16).ravel().view(np.float32)
    B, H, ns = p["batch"], p["n_head"], p.get("n_split", 1)
    worst = 0.0
    keep = np.ones(got.size, dtype=bool)
    for (b, h, s), r in res["part"].items():
        at = ((b * H + h) * ns + s) * PART
        keep[at:at + PART] = False
        m, l, o = got[at], got[at + 1], got[at + 2:at + PART].astype(np.float64)
        if r is None:
            assert m == -np.inf and l == 0 and not o.any(), f"{name} clip {b} head {h} split {s}: a split without keys recorded m {m} l {l}"
            continue
        ref, e, smax, dsmax = r
        assert abs(float(m) - smax) <= dsmax, f"{name} clip {b} head {h} split {s}: m {m} against {smax} +- {dsmax}"
        assert l > 0, f"{name} clip {b} head {h} split {s}: l = {l}"
        worst = max(worst, check_values(f"{name} clip {b} head {h} split {s}", o / float(l), ref, e))
    assert np.array_equal(got.view(np.uint32)[keep], init.view(np.uint32)[keep]), f"{name}: a record of a finished clip (or beyond the launch) changed"
    return worst


SCORE_FAMILIES = ("flat", "dominant", "rising", "falling", "huge")


def attn_qkv(rng, n, dt, family):
    """q [64] fp32, k, v [n][64] (h16 values) of one (clip, head): |s| ~ 1; one key 40 above the rest (the output is that key's V
    row exactly); scores rising / falling by 3 per key (clipped at 600 keys' worth); |s| in the hundreds."""
    q, k, v = rng.standard_normal(64), rng.standard_normal((n, 64)), rng.standard_normal((n, 64))
    if family == "dominant":
        q[0], k[:, 0] = 8.0, 0.0
        k[rng.integers(n), 0] = 40.0 + 100.0  # 0.125 * 8 * 140 = 140 above the rest: every other weight underflows to 0
    elif family in ("rising", "falling"):
        q[0] = 4.0
        k[:, 0] = (3.0 if family == "rising" else -3.0) * np.minimum(np.arange(n), 600) / (0.125 * 4.0)
        q[1:] *= 0.5
    elif family == "huge":
        sg = rng.choice([-1.0, 1.0], 64)
        q = 6.0 * sg + 0.25 * q
        k = 6.0 * sg * rng.choice([-1.0, 1.0], (n, 1)) + 0.25 * k
    return q.astype(np.float32), round16(k, dt), round16(v, dt)


# ------------------------------------------------------------------------------------------ launches (shared by the CPU proof and the GPU test)
# A launch is (cmd, id, p, outs): the driver's command, a label, its keys (scalars; a pointer field names a buffer) and the
# buffers to look at afterwards. A group is (bufs, [launches]): the launches run in order on one set of buffers, and each one is
# checked against the content its predecessors really left (the hand-offs of the step).
POINTER_KEYS = ("W", "bias", "x", "ln_w", "ln_b", "a_hi", "a_lo", "out", "out_hi", "out_lo", "k_cache", "v_cache", "off", "ln_w2", "W_lo",
                "out2", "stat_part", "amax_val", "amax_idx", "logits_dump", "g", "be", "hi", "lo", "part", "part_bias", "q", "k", "v", "done",
                "mpart", "mcnt", "wq", "bq", "tq", "fold_s", "fold_c", "w", "wp")
WRITABLE = {"cgemm": ("out", "out2", "stat_part", "k_cache", "v_cache", "out_hi", "out_lo"),
            "dgemm": ("out", "k_cache", "v_cache", "out_hi", "out_lo", "amax_val", "amax_idx", "logits_dump"),
            "actprep": ("x", "hi", "lo"), "attn": ("part", "out_hi", "out_lo", "mpart", "mcnt"), "packw": ("wp",), "packw_split": ("hi", "lo")}


H16_KEYS = ("W", "a_hi", "a_lo", "out_hi", "out_lo", "k_cache", "v_cache", "W_lo", "hi", "lo", "k", "v", "wq", "wp")
I32_KEYS = ("off", "done", "amax_idx", "mcnt")


def typed(p, bufs, cmd=None):
    """bufs with every buffer the launch names viewed as the type its field has (a dump comes back as uint16)."""
    out = dict(bufs)
    for k in POINTER_KEYS:
        if p.get(k):
            t = np.uint16 if (k in H16_KEYS or (k == "w" and cmd == "packw")) else np.int32 if k in I32_KEYS else np.float32
            out[p[k]] = np.ascontiguousarray(bufs[p[k]]).ravel().view(t)
    return out


def launch(cmd, ident, **p):
    return cmd, ident, p, [p[k] for k in WRITABLE[cmd] if p.get(k)]


def f32_slack(vals, slack):
    """float32 content followed by `slack` sentinel elements."""
    return np.concatenate([np.asarray(vals, dtype=np.float32).ravel().view(np.uint16), sentinel(slack, 4)]).view(np.float32)


def hidden_rows(rng, B, K, family):
    """what a pair input holds: N(0, 1) (an attention output), or an FFN hidden row of a trained model (post-GELU, sparse, a few
    entries up to modelgen's hidden_peak of 6000)."""
    a = rng.standard_normal((B, K))
    if family == "realistic":
        a = np.maximum(a, 0) * 2
        a[:, rng.choice(K, max(2, K // 256), replace=False)] = rng.uniform(2000, 6000, (B, max(2, K // 256)))
    return a.astype(np.float32)


def linear_group(dt, seed, cmd, *, K, N, batch, nbs, epi, rt=1, ln=False, family="benign", d_model=0, offs=None, ksplit=1, n_ctx_pad=448):
    """One cgemm / dgemm launch (not LOGITS) with everything around its outputs holding the sentinel."""
    rng = np.random.default_rng(seed)
    B = batch
    b, p = {}, dict(N=N, K=K, batch=B, nbs=nbs, epilogue=epi, rt=rt)
    oc = ()
    if ln:
        if family == "realistic":
            x, g, be, oc = realistic_stream(rng, B, K)
        else:
            x, g, be = ln_rows(rng, B, K), rng.uniform(0.5, 1.5, K).astype(np.float32), rng.uniform(-1, 1, K).astype(np.float32)
        b.update(x=f32_slack(x, K), ln_w=g, ln_b=be)
        p.update(x="x", ln_w="ln_w", ln_b="ln_b")
    else:
        b["a_hi"], b["a_lo"] = frag_pair(hidden_rows(rng, B, K, family), nbs, dt)
        p.update(a_hi="a_hi", a_lo="a_lo")
    b["W"] = to_bits(pack_weight(weights(rng, N, K, dt, family, oc)), dt)
    p["W"] = "W"
    if epi != GEPI_PARTIAL:
        b["bias"], p["bias"] = rng.uniform(-1, 1, N).astype(np.float32), "bias"
    if epi == GEPI_STORE:
        b["out"] = sentinel((B + 1) * N, 4)
    elif epi == GEPI_RESID:
        b["out"] = f32_slack(rng.standard_normal(B * N) * (3.0 if family == "realistic" else 1.0), N)
    elif epi == GEPI_GELU:
        b["out_hi"], b["out_lo"] = (sentinel((N + 31) // 32 * nbs * 512, 2) for _ in range(2))
        p.update(out_hi="out_hi", out_lo="out_lo")
    elif epi == GEPI_QKV_CACHE:
        bs = d_model * n_ctx_pad + 4096 + 64  # slack between the clips' caches
        b.update(out=sentinel((B + 1) * d_model, 4), k_cache=sentinel(B * bs, 2), v_cache=sentinel(B * bs, 2), off=np.asarray(offs, dtype=np.int32))
        p.update(k_cache="k_cache", v_cache="v_cache", off="off", d_model=d_model, n_ctx_pad=n_ctx_pad, kv_batch_stride=bs)
    elif epi == GEPI_PARTIAL:
        pb = B + 3
        b["out"] = sentinel((ksplit * pb + 1) * N, 4)  # the engine's part_batch is its capacity, not this launch's clips
        p.update(ksplit=ksplit, part_batch=pb)
    if "out" in b:
        p["out"] = "out"
    return b, [launch(cmd, f"{cmd}.K{K}.N{N}.b{B}.e{epi}.rt{rt}.{'ln' if ln else 'pair'}.{family}", **p)]


def actprep_launch(rng, b, *, K, batch, nbs, n_part, do_ln, part_batch, part="part", x="x", ident=None):
    """launch_act_prep on buffers b (x, part present or made here)."""
    if x not in b:
        b[x] = f32_slack(ln_rows(rng, batch, K), K)
    if n_part and part not in b:
        b[part] = f32_slack(rng.standard_normal(((n_part - 1) * part_batch + batch) * K), K)
    b.update(g=rng.uniform(0.5, 1.5, K).astype(np.float32), be=rng.uniform(-1, 1, K).astype(np.float32),
             part_bias=rng.uniform(-1, 1, K).astype(np.float32), hi=sentinel(K // 32 * nbs * 512, 2), lo=sentinel(K // 32 * nbs * 512, 2))
    p = dict(K=K, batch=batch, nbs=nbs, n_part=n_part, do_ln=int(do_ln), part_batch=part_batch, x=x, hi="hi", lo="lo")
    if do_ln:
        p.update(g="g", be="be")
    if n_part:
        p.update(part=part, part_bias="part_bias")
    return launch("actprep", ident or f"actprep.K{K}.b{batch}.p{n_part}.ln{int(do_ln)}", **p)


def partial_group(dt, seed, *, K, d, batch, nbs):
    """The split-K residual GEMM with the slice count the engine picks, and the act_prep launch that folds its partials."""
    ks = ksplit_for(K)
    b, ls = linear_group(dt, seed, "dgemm", K=K, N=d, batch=batch, nbs=nbs, epi=GEPI_PARTIAL, ksplit=ks)
    b["part"] = b.pop("out")
    ls[0][2].update(out="part")
    ls[0] = launch("dgemm", ls[0][1] + f".ks{ks}", **ls[0][2])
    ls.append(actprep_launch(np.random.default_rng(seed + 1), b, K=d, batch=batch, nbs=nbs, n_part=ks, do_ln=True, part_batch=batch + 3))
    return b, ls


def logits_group(dt, seed, *, K, N, batch, nbs, rt, offs=None, skip=0, dump=True, ties=True, family="benign"):
    """The vocabulary projection. ties: the rows of the largest logit of clip 0 are duplicated — into the same 16-row tile, the
    next row lane, another workgroup, and (rt 0) a later iteration of the same workgroup — so the lowest index has to win."""
    rng = np.random.default_rng(seed)
    B = batch
    a = rng.standard_normal((B, K)).astype(np.float32)
    w = weights(rng, N, K, dt, family)
    grid = dgemm_grid(N, rt)
    if ties and N >= 4:
        hi, lo = pair_split(a, dt)
        top = int(np.argmax(mm64(hi[:1].astype(np.float64) + lo[:1], w)[0]))
        span = 16 * max(rt, 1)
        dup = {((top // 16) * 16 + (top + 5) % 16) % N, (top + span) % N, (top + 16 * grid) % N, (top + 32 * grid + 3) % N, N - 1}
        for r in dup:
            w[r] = w[top]
    b = dict(W=to_bits(pack_weight(w), dt), off=np.asarray(offs if offs is not None else np.arange(B) + 3, dtype=np.int32),
             amax_val=sentinel(B * (grid + 2), 4), amax_idx=sentinel(B * (grid + 2), 4))
    b["a_hi"], b["a_lo"] = frag_pair(a, nbs, dt)
    p = dict(N=N, K=K, batch=B, nbs=nbs, epilogue=GEPI_LOGITS, rt=rt, W="W", a_hi="a_hi", a_lo="a_lo", off="off", amax_val="amax_val",
             amax_idx="amax_idx", amax_stride=grid + 2, skip_before_step=skip)
    if dump:
        b["logits_dump"] = sentinel(B * (N + 7), 4)
        p.update(logits_dump="logits_dump", logits_dump_stride=N + 7)
    return b, [launch("dgemm", f"logits.K{K}.N{N}.b{B}.rt{rt}.skip{skip}", **p)]


def fold_group(dt, seed, *, d, batch, nbs, n_split, n_keys=1500, family="realistic"):
    """The query fold's hand-off: the QKV launch with rows [3d, 4d) against ln_w2 . x -> A0; the o launch with the (hi, lo) product
    matrix adding onto A0 and leaving the block statistics; decode_attention_kernel<2> consuming both."""
    rng = np.random.default_rng(seed)
    B, H, cap = batch, d // 64, (n_keys + 63) // 64
    if family == "realistic":
        x, g, be, oc = realistic_stream(rng, B, d)
        g2 = realistic_stream(rng, 1, d)[1]
        g2[oc] = rng.uniform(0.02, 0.1, 2)
    else:
        x, g, be, oc = ln_rows(rng, B, d), rng.uniform(0.5, 1.5, d).astype(np.float32), rng.uniform(-1, 1, d).astype(np.float32), ()
        g2 = rng.uniform(0.5, 1.5, d).astype(np.float32)
    bs = d * 448 + 4096
    offs = rng.permutation(448)[:B]
    b = dict(x=f32_slack(x, d), ln_w=g, ln_b=be, ln_w2=g2, W=to_bits(pack_weight(weights(rng, 4 * d, d, dt, family, oc)), dt),
             bias=rng.uniform(-1, 1, 4 * d).astype(np.float32), q=sentinel((B + 1) * d, 4), a0=sentinel((B + 1) * d, 4),
             k_cache=sentinel(B * bs, 2), v_cache=sentinel(B * bs, 2), off=offs.astype(np.int32))
    ls = [launch("cgemm", f"fold.qkv.d{d}.b{B}.{family}", N=4 * d, K=d, batch=B, nbs=nbs, epilogue=GEPI_QKV_CACHE, rt=2 if (4 * d // 16) * ((B + 15) // 16) > 512 else 1,
                 x="x", ln_w="ln_w", ln_b="ln_b", ln_w2="ln_w2", W="W", bias="bias", out="q", out2="a0", k_cache="k_cache", v_cache="v_cache",
                 off="off", d_model=d, n_ctx_pad=448, kv_batch_stride=bs, fold_row0=3 * d)]
    # o launch: W_o rows [0, d), M_hi rows [d, 2d) in one array, M_lo apart; the attention vector as a pair
    m = rng.standard_normal((d, d)) * (0.02 * 4.0)
    mh, ml = pair_split(m, dt)
    wo = np.concatenate([weights(rng, d, d, dt, family), mh])
    b["Wo"], b["Wlo"] = to_bits(pack_weight(wo), dt), to_bits(pack_weight(ml), dt)
    b["att_hi"], b["att_lo"] = frag_pair(hidden_rows(rng, B, d, "benign"), nbs, dt)
    b["bias_o"] = rng.uniform(-1, 1, 2 * d).astype(np.float32)
    b["stat"] = sentinel((B + 1) * (d // 16) * 2, 4)
    ls.append(launch("cgemm", f"fold.o.d{d}.b{B}.{family}", N=2 * d, K=d, batch=B, nbs=nbs, epilogue=GEPI_RESID, rt=1, a_hi="att_hi", a_lo="att_lo",
                     W="Wo", W_lo="Wlo", bias="bias_o", out="x", out2="a0", stat_part="stat", fold_row0=d))
    kv = attn_kv(rng, dt, B, H, cap, n_keys, 0, b)
    b.update(fold_s=rng.standard_normal(d).astype(np.float32), fold_c=rng.standard_normal(d).astype(np.float32), done=np.zeros(B, np.int32),
             o_hi=sentinel(d // 32 * nbs * 512, 2), o_lo=sentinel(d // 32 * nbs * 512, 2), mpart=sentinel(B * H * n_split * PART, 4),
             mcnt=np.zeros(B * H + 2, np.int32))
    ls.append(launch("attn", f"fold.attn.d{d}.b{B}.s{n_split}.{family}", batch=B, n_head=H, d_model=d, n_keys=n_keys, cap_blocks=cap, n_split=n_split,
                     nbs=nbs, done_late=1, tq="a0", stat_part="stat", fold_s="fold_s", fold_c="fold_c", done="done", out_hi="o_hi", out_lo="o_lo",
                     **({"mpart": "mpart", "mcnt": "mcnt"} if n_split > 1 else {}), **kv))
    return b, ls


def attn_kv(rng, dt, B, H, cap, n_keys, slack, b, names=("k", "v"), garbage=False, kv=None):
    """K / V buffers of cap blocks per (clip, head): standard-normal (or the given natural [B][H][cap * 64][64]) rows; rows at or
    beyond the keys in use hold zeros as the engine's caches do, or finite garbage."""
    stride = H * cap * 4096 + slack
    nk = np.broadcast_to(np.asarray(n_keys), (B,))
    out = {}
    for i, nm in enumerate(names):
        nat = rng.standard_normal((B, H, cap * 64, 64)) if kv is None else kv[i].copy()
        for c in range(B):
            nat[c, :, nk[c]:] = rng.uniform(-300, 300, nat[c, :, nk[c]:].shape) if garbage else 0.0
        b[nm] = kv_store(nat, stride, dt, i == 0, 0)
        out["kv"[i]] = nm
    out["kv_batch_stride"] = stride
    return out


def attn_group(dt, seed, *, H=3, batch=3, cap, n_keys=None, offs=None, n_split=1, mode="q", out="pair", nbs=None, done=None, done_late=0,
               families=SCORE_FAMILIES, garbage_too=True, relaunch=False):
    """One attention launch (and a second one on finite garbage beyond the keys; relaunch: a third without resetting anything).
    mode: "q" | "fused" (LayerNorm + projection in the kernel). Score families are dealt over the (clip, head) pairs."""
    rng = np.random.default_rng(seed)
    B, d = batch, H * 64
    nbs = nbs or (B + 15) // 16 + 1
    nk = np.full(B, n_keys) if n_keys is not None else np.asarray(offs) + 1
    b = dict(done=np.asarray(done if done is not None else np.zeros(B), dtype=np.int32))
    p = dict(batch=B, n_head=H, d_model=d, n_keys=n_keys if n_keys is not None else -1, cap_blocks=cap, n_split=n_split, nbs=nbs,
             done_late=done_late, done="done")
    if offs is not None:
        b["off"], p["off"] = np.asarray(offs, dtype=np.int32), "off"
    kn, vn = np.zeros((B, H, cap * 64, 64)), np.zeros((B, H, cap * 64, 64))
    q = np.zeros((B, d), np.float32)
    for c in range(B):
        for h in range(H):
            fam = families[(c * H + h + seed) % len(families)] if mode == "q" else "flat"
            q[c, h * 64:h * 64 + 64], kn[c, h, :nk[c]], vn[c, h, :nk[c]] = attn_qkv(rng, nk[c], dt, fam)
    if mode == "q":
        b["q"], p["q"] = f32_slack(q, d), "q"
    else:
        x, g, be, _ = realistic_stream(rng, B, d) if seed % 2 else (ln_rows(rng, B, d), rng.uniform(0.5, 1.5, d).astype(np.float32), rng.uniform(-1, 1, d).astype(np.float32), ())
        b.update(x=f32_slack(x, d), ln_w=g, ln_b=be, wq=to_bits(weights(rng, d, d, dt, "realistic"), dt), bq=rng.uniform(-1, 1, d).astype(np.float32))
        p.update(x="x", ln_w="ln_w", ln_b="ln_b", wq="wq", bq="bq")
    p.update(attn_kv(rng, dt, B, H, cap, nk, 128, b, kv=(kn, vn)))
    if out == "pair":
        b.update(out_hi=sentinel(d // 32 * nbs * 512, 2), out_lo=sentinel(d // 32 * nbs * 512, 2))
        p.update(out_hi="out_hi", out_lo="out_lo")
        if n_split > 1:
            b.update(mpart=sentinel(B * H * n_split * PART, 4), mcnt=np.zeros(B * H + 2, np.int32))
            p.update(mpart="mpart", mcnt="mcnt")
    else:
        b["part"], p["part"] = sentinel((B * H * n_split + 1) * PART, 4), "part"
    ident = f"attn.{mode}.H{H}.b{B}.cap{cap}.keys{n_keys if n_keys is not None else 'off'}.s{n_split}.{out}.late{done_late}"
    ls = [launch("attn", ident, **p)]
    if garbage_too:
        g2 = dict(p)
        g2.update(attn_kv(rng, dt, B, H, cap, nk, 128, b, names=("kg", "vg"), garbage=True, kv=(kn, vn)))
        ls.append(launch("attn", ident + ".garbage", **g2))
    if relaunch:
        ls.append(launch("attn", ident + ".again", **p))
    return b, ls


def pack_groups(dt, seed, N, K):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((N, K)).astype(np.float32)
    n = (N + 15) // 16 * 16 * K
    return [(dict(w=to_bits(w, dt), wp=sentinel(n, 2)), [launch("packw", f"packw.N{N}.K{K}", N=N, K=K, w="w", wp="wp")]),
            (dict(w=w, hi=sentinel(n, 2), lo=sentinel(n, 2)), [launch("packw_split", f"packw_split.N{N}.K{K}", N=N, K=K, w="w", hi="hi", lo="lo")])]


# ------------------------------------------------------------------------------------------ the check of one launch
def strip(name, got):
    g = GUARD // 2
    got = np.ascontiguousarray(got).view(np.uint16).ravel()
    assert (got[:g] == SENT16).all() and (got[-g:] == SENT16).all(), f"{name}: store into a guard"
    return got[g:-g]


def verify(cmd, ident, p, state, got, dt, prev=None):
    """state: buffer name -> content before the launch; got: buffer name -> uint16 dump (guards included) after it; prev: the
    dumps of the launch before (an attention launch labelled ".again" or ".garbage" must reproduce them bit for bit). Returns {label: worst error / bound}."""
    notes = {}
    state = typed(p, state, cmd)
    if cmd in ("cgemm", "dgemm"):
        exp, pairs, info = gemm_expect(p, state, dt)
        epi = p["epilogue"]
        form = "ln" if p.get("ln_w") else "pair"
        for name, e in exp.items():
            key = [k for k in ("out", "out2", "stat_part", "k_cache", "v_cache", "logits_dump") if p.get(k) == name][0]
            notes[f"{cmd} epilogue {epi} {form} {key}"] = check(f"{ident} {name}", got[name], e, dt)
        for (hn, ln_), pe in pairs.items():
            notes[f"{cmd} epilogue {epi} {form} pair"] = check_pair(f"{ident} pair", got[hn], got[ln_], state[hn], state[ln_], pe, dt)
        if epi == GEPI_LOGITS:
            grid, B, st = dgemm_grid(p["N"], p["rt"]), p["batch"], p["amax_stride"]
            av, ai = strip(ident, got[p["amax_val"]]), strip(ident, got[p["amax_idx"]])
            if not info["wrote"]:
                assert np.array_equal(av, state[p["amax_val"]].view(np.uint16)) and np.array_equal(ai, state[p["amax_idx"]].view(np.uint16)), f"{ident}: written below skip_before_step"
                return notes
            want_v, want_i = np.ascontiguousarray(state[p["amax_val"]]).view(np.float32).copy(), np.ascontiguousarray(state[p["amax_idx"]]).view(np.int32).copy()
            if p.get("logits_dump"):
                lg = strip(ident, got[p["logits_dump"]]).view(np.float32)
                lg = np.stack([lg[c * p["logits_dump_stride"]:c * p["logits_dump_stride"] + p["N"]] for c in range(B)])
            else:
                lg = None
            rv, ri = argmax_expect(lg if lg is not None else info["logits"].astype(np.float32), p["N"], p["rt"], grid)
            for c in range(B):
                want_v[c * st:c * st + grid], want_i[c * st:c * st + grid] = rv[c], ri[c]
            gv, gi = av.view(np.float32), ai.view(np.int32)
            if lg is not None:
                assert np.array_equal(gv.view(np.uint32), want_v.view(np.uint32)), f"{ident}: an argmax partial is not the maximum of its rows"
                bad = np.nonzero(gi != want_i)[0]
                assert bad.size == 0, f"{ident}: argmax index {gi[bad[0]]} where the lowest row with the maximum is {want_i[bad[0]]}"
            else:  # no dump: the maximum within the logits' bound, everything else untouched
                mask = np.zeros(gv.size, dtype=bool)
                for c in range(B):
                    mask[c * st:c * st + grid] = True
                assert np.array_equal(gv.view(np.uint32)[~mask], want_v.view(np.uint32)[~mask]) and np.array_equal(gi[~mask], want_i[~mask])
                bmax = np.stack([info["bound"][:, (np.arange(p["N"]) // 16) % grid == w].max(1) if p["rt"] == 0 else
                                 info["bound"][:, w * 16 * p["rt"]:(w + 1) * 16 * p["rt"]].max(1) for w in range(grid)], 1)
                refv = argmax_expect(info["logits"], p["N"], p["rt"], grid)[0]
                for c in range(B):
                    notes[f"dgemm logits rt{p['rt']} max"] = max(notes.get(f"dgemm logits rt{p['rt']} max", 0), check_values(ident, gv[c * st:c * st + grid], refv[c], bmax[c]))
        return notes
    if cmd == "actprep":
        exp, pairs = actprep_expect(p, state, dt)
        for name, e in exp.items():
            if p["n_part"]:
                notes["actprep x"] = check(f"{ident} x", got[name], e, dt)
            else:
                assert np.array_equal(strip(ident, got[name]), np.ascontiguousarray(state[name]).view(np.uint16)), f"{ident}: x written without partials"
        for (hn, ln_), pe in pairs.items():
            notes[f"actprep pair ln{p['do_ln']}"] = check_pair(f"{ident} pair", got[hn], got[ln_], state[hn], state[ln_], pe, dt)
        return notes
    if cmd == "attn":
        if prev is not None and ident.endswith((".again", ".garbage")):
            for name in got:
                if name != p.get("mpart"):
                    assert np.array_equal(got[name], prev[name]), f"{ident}: {name} differs from the launch before"
        res = attn_expect(p, state, dt)
        mode = "fold" if p.get("tq") else "fused" if p.get("wq") else "q"
        if res["pair"] is not None:
            notes[f"attn {mode} pair splits {p.get('n_split', 1)}"] = check_pair(f"{ident}", got[p["out_hi"]], got[p["out_lo"]], state[p["out_hi"]], state[p["out_lo"]], res["pair"], dt)
            if p.get("mcnt"):
                strip(ident, got[p["mpart"]])
                assert not strip(ident, got[p["mcnt"]]).any(), f"{ident}: mcnt is not zero after the launch"
        else:
            notes[f"attn {mode} part splits {p.get('n_split', 1)}"] = check_attn_part(ident, got[p["part"]], state[p["part"]], p, res)
        return notes
    if cmd == "packw":
        w = state[p["w"]].reshape(p["N"], p["K"])
        assert np.array_equal(strip(ident, got[p["wp"]]), pack_weight(w)), f"{ident}: the packed weights differ from the index map"
        return {"packw": 0.0}
    if cmd == "packw_split":
        hi, lo = pair_bits(state[p["w"]].reshape(p["N"], p["K"]), dt)
        assert np.array_equal(strip(ident, got[p["hi"]]), pack_weight(hi)), f"{ident}: hi != h16(w)"
        assert np.array_equal(strip(ident, got[p["lo"]]), pack_weight(lo)), f"{ident}: lo != h16(w - hi)"
        return {"packw_split": 0.0}
    raise ValueError(cmd)
