"""Float64 references of the encoder's kernels (whisper.axera_amd/csrc/gemm.hip, encoder_attn.hip) on the same 16-bit input
values, and the checker that compares EVERY output element under a bound computed from the reference (never a constant), and
every element a launch must not write bit for bit with what was there before.

Notation: u = 2^-24 (unit roundoff of fp32), u16 = 2^-8 (bfloat16) / 2^-11 (IEEE half), hulp(x) = half an ulp of the build's
16-bit type at |x| (fp16 subnormals: 2^-25, absolute). Every bound below is "first order, worst case": |error| <= bound for a
kernel that does the stated arithmetic in fp32 in ANY order.

GEMM, acc = sum_k A[m,k] W[n,k] (+ bias): products of two 16-bit values are exact in fp32, so only the K - 1 additions and
the bias addition round:  E_acc = K u (|A| |W|^T + |bias|)[m,n]  from a second float64 product of absolute values.
  EPI_BIAS_BF16, EPI_QKV, EPI_CROSS_KV  E = E_acc + hulp(|ref| + E_acc)   (the kernel rounds ITS value, which may sit E_acc away)
  EPI_PARTIAL_F32                       E = (K / ksplit) u (|A| |W|^T) over the slice's k range
  EPI_RESID_F32   C += acc + bias       E = E_acc + u |C| (the addition acc + bias + C may associate either way: u (|acc+bias| +
                                        |C|) is inside E_acc + u |C|) + u |ref| for the last addition
  GELU epilogues, x = acc + bias, g(x) = 0.5 x (1 + erf(x / sqrt 2)), |g'| <= 1.13:
    pre-activation error carried through: 1.13 E_acc
    EPI_GELU_POS_F32 (erff of the device library, at most 4 ulp = 4 u below 1): the argument x / sqrt 2 carries 2 u relative,
      worth at most 2 u * max z erf'(z) < 1 u; erf: 4 u; 1 + erf: 1 u at most 2 u below the binade edge -> (1 + erf) within
      7 u, times 0.5 |x| = 3.5 u |x|; the two multiplications u |g| <= u |x| each -> 6 u |x|, taken as 8 u |x|; the addition
      of the position adds u |ref|.                                   E = 1.13 E_acc + 8 u |x| + u |ref|
    EPI_BIAS_GELU_BF16 (gelu_erf_fast2: erf by Abramowitz-Stegun 7.1.26, published |erf error| <= 1.5e-7 -> 0.5 |x| 1.5e-7):
      t = rcp(1 + p|x|/sqrt 2): multiply-add 2 u + hardware reciprocal 1 ulp (2 u) = 4 u relative; the degree-5 polynomial
      0.5 poly(t) moves by |t poly'(t)| 4 u <= 0.5 (0.25 + 2*0.28 + 3*1.42 + 4*1.45 + 5*1.06) 4 u = 32 u, its five Horner steps
      add <= 2 u each on partial sums below 1.3 -> 45 u; exp2(-w^2), w = c |x|: w^2 carries 5 u relative, worth
      5 u ln2 y 2^-y <= 2 u at any y, plus v_exp's 1 ulp (2 u) -> 4 u; e = 0.5 - poly exp2: 45 u + 0.5 * 4 u + 2 u <= 49 u;
      the result |x| e + 0.5 x: 49 u |x| + 2 u |x| -> taken as 56 u |x| (absolute: in the negative tail, where g(x) is far below
      |x|, this — not the output's ulp — is what the kernel's cancellation really leaves).
                                             E' = 1.13 E_acc + (0.75e-7 + 56 u) |x|,  E = E' + hulp(|ref| + E')

LayerNorm (one wave per row, fp32; d values): S1 = mean |x|, a = x - mean, var = mean a^2, r = (var + 1e-5)^-1/2
  mean: d u S1 (any order) ; a: that + u |a| ; var: 2 mean(|a| da) + mean(da^2) + (d + 4) u var ; r: relative
  0.5 dvar / (var + eps) + 4 u (addition, division, rsqrtf within 1 ulp) ; y = a r g + b: |g| (da r + |a| r dr_rel) + 3 u (|a r g| + |y|),
  then hulp(|ref| + E). With a partial fold x' = x + bias + part[0] + ... (fixed order, n + 1 additions) the written-back x' is
  within (n + 1) u (|x| + |bias| + sum |part|) and that error enters a (and, through a, the variance) as an input perturbation.

Attention, o = sum_j p_j v_j, p = softmax(q.k / 8) over keys < T, PV = sum_j p_j |v_j| (all reference quantities):
  P is narrowed to h16 while l is summed unrounded:       u16 PV
  score error ds_j = 64 u sum_d |q_d| |k_jd| (raw units), carried through exp (x 0.125 p_j) in numerator and denominator:
                                                            sum_j p_j 0.125 ds_j (|v_j| + |o|)
  exponent arithmetic: exp2(fma(s, c, -fl(m c))): the rounding of m c (u |m| c log2 units = 0.125 u |m| relative in p, at
  most twice: before and after a rescale), of the fma result (0.125 u |s_j - m| 8 ... taken as 0.125 u |s_j - s_max|) and
  v_exp's 1 ulp twice (p and alpha) = 4 u:                  sum_j p_j eps_j (|v_j| + |o|), eps_j = u (4 + 0.25 max|s| + 0.125 |s_j - s_max|)
  fp32 sums: P.V over T keys in any order T u PV; l: a lane adds 32 terms per tile, the tiles, the other half: (33 + tiles) u;
  1 / l and the final product 3 u:                          (T + 36 + tiles) u PV
  fp16 only: a probability below 2^-14 is a subnormal, absolute error 2^-25 in units where l >= 1:   2^-25 sum_j |v_j|
  The first-order terms carry a factor 2 for what first order leaves out (products of two relative errors, and p evaluated
  at the reference's scores instead of the kernel's); then hulp(|ref| + E).
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
SENT16 = 0x7FC5  # a NaN in bfloat16, in half and (twice) in fp32: nothing a kernel computes from finite inputs
GUARD = 4096     # bytes before and after every allocation of the driver, filled with the sentinel

EPI_BIAS, EPI_GELU, EPI_GELU_POS, EPI_RESID, EPI_QKV, EPI_CROSS_KV, EPI_PARTIAL = range(7)


# ------------------------------------------------------------------------------------------ the 16-bit types
def tdtype(dt):
    return torch.float16 if dt == "f16" else torch.bfloat16


def u16(dt):
    return 2.0 ** -11 if dt == "f16" else 2.0 ** -8


def to_bits(x, dt):
    """float array -> uint16 bit patterns of the build's type (round to nearest even)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdtype(dt))
    return t.view(torch.int16).numpy().view(np.uint16)


def from_bits(b, dt):
    """uint16 bit patterns -> float64 values."""
    t = torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).view(tdtype(dt))
    return t.to(torch.float64).numpy()


def round16(x, dt):
    """float32 values rounded to the build's 16-bit type (the kernels' narrowing points)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdtype(dt)).to(torch.float32).numpy()


def hulp(x, dt):
    """Half an ulp of the 16-bit type at |x| (float64 array)."""
    ax = np.abs(x)
    e = np.floor(np.log2(np.maximum(ax, 1e-300)))
    if dt == "f16":
        e = np.maximum(e, -14.0)  # subnormals: absolute 2^-25
        return np.exp2(e - 11.0)
    return np.exp2(np.maximum(e, -126.0) - 8.0)


def sentinel(n_elems, itemsize):
    return np.full(n_elems * itemsize // 2, SENT16, dtype=np.uint16)


def mm64(a, b):
    """float64 a @ b^T through torch (threaded)."""
    return (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) @ torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).T).numpy()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x) * (0.5 ** 0.5)).numpy())


def vt_perm(m):
    """position of frame m inside V^T: the frames of a 16-group are stored in the order [0-3, 8-11, 4-7, 12-15]."""
    m = np.asarray(m)
    return (m & ~15) | ((m & 4) << 1) | ((m & 8) >> 1) | (m & 3)


# ------------------------------------------------------------------------------------------ GEMM
class Expect:
    """What one output buffer must hold after a launch: `ref` / `bound` (float64, flat) where `written`, the initial bits
    elsewhere."""

    def __init__(self, init_bits, itemsize):
        self.init = init_bits  # uint16 view of the initial content
        self.itemsize = itemsize
        n = init_bits.size * 2 // itemsize
        self.ref = np.zeros(n)
        self.bound = np.zeros(n)
        self.written = np.zeros(n, dtype=bool)

    def put(self, idx, ref, bound):
        idx = np.asarray(idx).ravel()
        before = int(self.written.sum())
        self.ref[idx] = np.asarray(ref).ravel()
        self.bound[idx] = np.asarray(bound).ravel()
        self.written[idx] = True
        assert int(self.written.sum()) == before + idx.size, "the reference writes an element twice"


def gather_rows(a_vals, off, lda, M, K):
    """A rows as the kernel addresses them: row m = K values from off + m * lda (rows may overlap)."""
    return np.lib.stride_tricks.as_strided(a_vals[off:], shape=(M, K), strides=(lda * a_vals.itemsize, a_vals.itemsize))


def gemm_expect(p, bufs, dt):
    """p: the launch as GemmParams sees it (element offsets into named buffers), bufs: name -> initial content (uint16 bit
    view for h16 buffers, float32 for fp32 ones, int32 for the slot map). Returns {buffer name: Expect}."""
    epi, M, N, K, B, d = p["epi"], p["M"], p["N"], p["K"], p["batch"], p["d"]
    A = from_bits(bufs[p["A"]], dt)
    W = from_bits(bufs[p["W"]], dt).reshape(N, K)
    bias = bufs[p["bias"]].astype(np.float64) if p.get("bias") else np.zeros(N)
    part = p.get("qkv_part", 0)
    out = {}

    def expect(name, itemsize):
        if name not in out:
            out[name] = Expect(np.ascontiguousarray(bufs[name]).view(np.uint16).ravel(), itemsize)
        return out[name]

    for key, size in (("C", 4 if epi in (EPI_GELU_POS, EPI_RESID) else 2), ("C2", 2), ("C3", 2), ("part", 4)):
        if p.get(key):  # every output buffer of the launch is checked, also the ones this launch must leave alone
            expect(p[key], size)
    n_idx = np.arange(N)
    m_idx = np.arange(M)[:, None]
    for b in range(B):
        a = gather_rows(A, p.get("A_off", 0) + b * p["a_bs"], p["lda"], M, K)
        if epi == EPI_PARTIAL:
            ks = p["ksplit"]
            e = expect(p["part"], 4)
            for q in range(ks):
                sl = slice(q * K // ks, (q + 1) * K // ks)
                acc, ab = mm64(a[:, sl], W[:, sl]), mm64(np.abs(a[:, sl]), np.abs(W[:, sl]))
                e.put(q * p["part_stride"] + b * M * N + m_idx * N + n_idx, acc, (K // ks) * U32 * ab)
            continue
        acc = mm64(a, W) + bias
        eacc = K * U32 * (mm64(np.abs(a), np.abs(W)) + np.abs(bias))
        if epi == EPI_BIAS:
            expect(p["C"], 2).put(p.get("C_off", 0) + b * p["c_bs"] + m_idx * p["ldc"] + n_idx, acc, eacc + hulp(np.abs(acc) + eacc, dt))
        elif epi == EPI_GELU:
            g = gelu64(acc)
            e1 = 1.13 * eacc + (0.75e-7 + 56 * U32) * np.abs(acc)
            expect(p["C"], 2).put(p.get("C_off", 0) + b * p["c_bs"] + m_idx * p["ldc"] + n_idx, g, e1 + hulp(np.abs(g) + e1, dt))
        elif epi == EPI_GELU_POS:
            pos = bufs[p["aux"]].astype(np.float64).reshape(M, N)
            ref = gelu64(acc) + pos
            expect(p["C"], 4).put(p.get("C_off", 0) + b * p["c_bs"] + m_idx * p["ldc"] + n_idx, ref, 1.13 * eacc + 8 * U32 * np.abs(acc) + U32 * np.abs(ref))
        elif epi == EPI_RESID:
            e = expect(p["C"], 4)
            idx = p.get("C_off", 0) + b * p["c_bs"] + m_idx * p["ldc"] + n_idx
            cur = bufs[p["C"]].ravel()[idx].astype(np.float64)
            ref = acc + cur
            e.put(idx, ref, eacc + U32 * np.abs(cur) + U32 * np.abs(ref))
        elif epi == EPI_QKV:
            bound = eacc + hulp(np.abs(acc) + eacc, dt)
            if part != 2:
                expect(p["C"], 2).put(b * p["c_bs"] + m_idx * d + np.arange(d), acc[:, :d], bound[:, :d])
                expect(p["C2"], 2).put(b * p["c2_bs"] + m_idx * d + np.arange(d), acc[:, d:2 * d], bound[:, d:2 * d])
            if part != 1:
                expect(p["C3"], 2).put(b * p["c3_bs"] + np.arange(d) * p["t_pad"] + vt_perm(m_idx), acc[:, 2 * d:], bound[:, 2 * d:])
        elif epi == EPI_CROSS_KV:
            bound = eacc + hulp(np.abs(acc) + eacc, dt)
            L, tp, nbt = p["n_layer"], p["t_pad"], p["nbt"]
            slot = int(bufs[p["slot_map"]][b]) if p.get("slot_map") else b
            n = np.arange(L * d)
            l, c = n // d, n % d
            head, dd = c >> 6, c & 63
            base = ((l * nbt + slot) * (d >> 6) + head) * tp * 64
            expect(p["C"], 2).put(base + (m_idx >> 6) * 4096 + (dd >> 3) * 512 + (m_idx & 63) * 8 + (dd & 7), acc[:, :L * d], bound[:, :L * d])
            expect(p["C2"], 2).put((base // 64 + m_idx) * 64 + dd, acc[:, L * d:], bound[:, L * d:])
        else:
            raise ValueError(epi)
    return out


def check(name, got_bits, exp, dt, guard=True):
    """got_bits: uint16 view of the dumped allocation (with its guards). Asserts every written element within its bound and
    everything else bit-identical to what was there; returns the worst error / bound."""
    g = GUARD // 2
    got_bits = np.ascontiguousarray(got_bits).view(np.uint16).ravel()
    if guard:
        assert (got_bits[:g] == SENT16).all(), f"{name}: store into the guard in front of the buffer"
        assert (got_bits[-g:] == SENT16).all(), f"{name}: store into the guard behind the buffer"
        got_bits = got_bits[g:-g]
    assert got_bits.size == exp.init.size, (name, got_bits.size, exp.init.size)
    w = torch.from_numpy(exp.written)
    k = exp.itemsize // 2
    changed = torch.from_numpy((got_bits != exp.init).reshape(-1, k)).any(1)  # per element (torch: threaded, these buffers are large)
    bad = torch.nonzero(changed & ~w)
    assert bad.numel() == 0, f"{name}: {bad.numel()} elements outside the valid output changed, first at element {int(bad[0])}"
    if not exp.written.any():  # a buffer this launch leaves alone altogether (the other half of a split Q,K / V launch)
        return 0.0
    if exp.itemsize == 4:
        got = torch.from_numpy(got_bits.view(np.float32)).to(torch.float64)
    else:
        got = torch.from_numpy(got_bits.view(np.int16)).view(tdtype(dt)).to(torch.float64)
    bound = torch.from_numpy(exp.bound)
    assert bool((bound[w] > 0).all()), f"{name}: a zero bound"
    ratio = (got - torch.from_numpy(exp.ref)).abs() / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))  # a NaN or inf output is beyond any bound
    ratio = torch.where(w, ratio, torch.zeros_like(ratio))
    el = int(torch.argmax(ratio))
    worst = float(ratio[el])
    assert worst <= 1.0, (f"{name}: element {el}: got {float(got[el])!r} want {exp.ref[el]!r} = {worst:.2f} x its bound {exp.bound[el]:.3e}; "
                          f"{int((ratio > 1).sum())} of {int(w.sum())} beyond")
    return worst


# ------------------------------------------------------------------------------------------ LayerNorm
def layernorm_expect(x, g, b, dt, part=None, part_bias=None):
    """x float32 [rows][d]; part float32 [n][rows][d] or None. Returns (x' ref, x' bound or None, y ref, y bound)."""
    x64 = x.astype(np.float64)
    d = x.shape[1]
    dx = np.zeros_like(x64)
    if part is not None:
        mag = np.abs(x64) + np.abs(part_bias.astype(np.float64)) + np.abs(part.astype(np.float64)).sum(0)
        x64 = x64 + part_bias.astype(np.float64) + part.astype(np.float64).sum(0)
        dx = (part.shape[0] + 1) * U32 * mag
    g64, b64 = g.astype(np.float64), b.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    a = x64 - mean
    var = (a * a).mean(1, keepdims=True)
    r = 1.0 / np.sqrt(var + 1e-5)
    y = a * r * g64 + b64
    dmean = d * U32 * np.abs(x64).mean(1, keepdims=True) + dx.mean(1, keepdims=True)
    da = dmean + U32 * np.abs(a) + dx
    dvar = 2 * (np.abs(a) * da).mean(1, keepdims=True) + (da * da).mean(1, keepdims=True) + (d + 4) * U32 * var
    dr_rel = 0.5 * dvar / (var + 1e-5) + 4 * U32
    e = np.abs(g64) * (da * r + np.abs(a) * r * dr_rel) + 3 * U32 * (np.abs(a * r * g64) + np.abs(y))
    return x64, (dx + U32 * np.abs(x64) if part is not None else None), y, e + hulp(np.abs(y) + e, dt)


# ------------------------------------------------------------------------------------------ attention
def attention_expect(q, k, v, dt, t_pad):
    """q, k, v float64 [T][64] of one (clip, head), v in natural frame order. Returns (o ref [T][64], bound)."""
    T = q.shape[0]
    nkt = t_pad // 64
    s = q @ k.T  # raw scores
    ds = 64 * U32 * (np.abs(q) @ np.abs(k).T)
    smax = s.max(1, keepdims=True)
    w = np.exp((s - smax) * 0.125)
    p = w / w.sum(1, keepdims=True)
    o = p @ v
    av = np.abs(v)
    pv = p @ av
    eps = U32 * (4 + 0.25 * np.abs(s).max(1, keepdims=True) + 0.125 * np.abs(s - smax)) + 0.125 * ds
    pe = p * eps
    first = u16(dt) * pv + pe @ av + pe.sum(1, keepdims=True) * np.abs(o) + (T + 36 + nkt) * U32 * pv
    e = 2 * first
    if dt == "f16":
        e = e + 2.0 ** -25 * av.sum(0, keepdims=True)
    return o, e + hulp(np.abs(o) + e, dt)


def check_values(name, got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    err[~np.isfinite(err)] = np.inf
    ratio = err / bound
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[i])
    assert worst <= 1.0, f"{name}: element {i}: got {np.asarray(got)[i]!r} want {ref[i]!r}, error {err[i]:.3e} = {worst:.2f} x its bound {bound[i]:.3e}; {int((ratio > 1).sum())} of {ratio.size} beyond"
    return worst


# ------------------------------------------------------------------------------------------ input families
def gemm_inputs(rng, shape_a, shape_w, n_bias, dt, family, k_hidden=False):
    """(A bits, W bits, bias f32). "uniform": A in [-1, 1), W in 0.05 [-1, 1), bias in [-1, 1) (profiles/microbench/
    gemm_shapes.cpp). "realistic": trained-model statistics — unit activations with a few channels at |x| 150-500 (k_hidden:
    an FFN hidden row, post-GELU, a few entries up to ~5000... scaled so that nothing overflows half) and N(0, 0.02) weights
    whose columns on the outlier channels are small, as trained models have them."""
    if family == "uniform":
        a = rng.uniform(-1, 1, shape_a)
        w = rng.uniform(-1, 1, shape_w) * 0.05
    else:
        K = shape_a[-1]
        a = rng.standard_normal(shape_a)
        w = rng.standard_normal(shape_w) * 0.02
        ch = rng.choice(K, size=max(2, K // 128), replace=False)
        if k_hidden:
            a = np.maximum(a, 0) * 2  # post-GELU: non-negative, sparse-ish
            a[..., ch] = rng.uniform(2000, 5000, (len(ch),))
        else:
            a[..., ch] = a[..., ch] * 20 + rng.uniform(150, 500, (len(ch),)) * rng.choice([-1, 1], (len(ch),))
        w[..., ch] *= 0.05
    return to_bits(a, dt), to_bits(w, dt), rng.uniform(-1, 1, n_bias).astype(np.float32)


ATTN_FAMILIES = ("flat", "dom0", "domlast", "domtail", "rise6", "rise10", "fall", "huge")


def attention_inputs(rng, T, dt, family):
    """q, k, v float32 [T][64] (already representable in the 16-bit type) of one (clip, head). Scores are s = q.k (raw), the
    softmax sees s / 8; in log2 units s * 0.18.
      flat      N(0,1) q and k: |s / 8| ~ 1
      dom0 / domlast / domtail  one key (0, T - 1, the first key of the last 64-key tile) ~40 nats above the rest
      rise6 / rise10 / fall     the row maximum rises by ~6 / ~10 log2 units per 64-key tile (straddling thresholds 0.5, 8
                16: rescales on every tile, every second, every third), or falls by 10 (late tiles underflow to 0)
      huge      |s / 8| in the hundreds: q = 6 sgn, k = +-6 sgn + noise"""
    q = rng.standard_normal((T, 64))
    k = rng.standard_normal((T, 64))
    v = rng.standard_normal((T, 64))
    tile = np.arange(T) // 64
    if family in ("dom0", "domlast", "domtail"):
        j = {"dom0": 0, "domlast": T - 1, "domtail": (T - 1) // 64 * 64}[family]
        q[:, 0] = 8.0
        k[:, 0] = 0.0
        k[j, 0] = 40.0  # 8 * 40 / 8 = 40 nats
    elif family in ("rise6", "rise10", "fall"):
        step = {"rise6": 6.0, "rise10": 10.0, "fall": -10.0}[family]
        q[:, 0] = 4.0
        k[:, 0] = step * tile / (0.125 * 1.4426950408889634 * 4.0)
        q[:, 1:] *= 0.5
    elif family == "huge":
        sg = rng.choice([-1.0, 1.0], 64)
        q = 6.0 * sg + 0.25 * q
        k = 6.0 * sg * rng.choice([-1.0, 1.0], (T, 1)) + 0.25 * k
    r = lambda x: round16(x, dt)
    return r(q), r(k), r(v)


def split_k_rule(d, K, batch, T=1500):
    """The engine's choice of K slices for a residual GEMM (csrc/engine.cpp, run_encoder::resid); 1 = no split."""
    tiles, nk = (d // 128) * ((T + 127) // 128) * batch, K // 64
    if d % 128 == 0 and batch <= 2 and tiles * 2 <= 256:
        for sp in (4, 3, 2):
            if nk % sp == 0 and nk // sp >= 4 and tiles * sp <= 512:
                return sp
    return 1


def expected_kernel(force, M, n_cols, K, batch, a_elems, w_elems):
    """The kernel launch_one starts (csrc/gemm.hip): 1 = 128x128, 2 = 256x128 ring, 5 = 256x256 stream per CU."""
    mt256 = (M + 255) // 256
    if n_cols % 256 == 0:
        tiles_sq = n_cols // 256 * mt256 * batch
        fill = lambda t: t / ((t + 255) // 256 * 256)
        sq_pays = tiles_sq >= 256 and 1.15 * fill(tiles_sq) >= fill(2 * tiles_sq)
        nk = K // 64
        if (force == 5 or (force == 0 and sq_pays)) and nk >= 4 and nk % 2 == 0 and a_elems * 2 < 2 ** 32 and w_elems * 2 < 2 ** 32:
            return 5
    tiles256 = n_cols // 128 * mt256 * batch
    if force == 2 or (force == 0 and tiles256 >= 256 and K >= 128):
        return 2
    return 1


# ------------------------------------------------------------------------------------------ the launches of run_encoder
GEMM_KINDS = ("conv1", "conv2", "qkv", "qk", "v", "oproj_resid", "ffn2_resid", "oproj_part", "ffn2_part", "ffn1", "cross", "bias")


def gemm_case(kind, d, clips, dt, family, seed, T=1500, n_layer=4, ksplit=0):
    """One launch of Engine::run_encoder (csrc/engine.cpp) with its strides and offsets: (params, buffers). Buffers hold the
    initial content of every allocation; whatever the launch must not write holds the sentinel."""
    rng = np.random.default_rng(seed)
    frames, t_pad = 2 * T, (T + 63) // 64 * 64
    mel_rows, h1_rows = frames + 4, frames + 2
    nm = 80 if d <= 1024 else 128
    tail = 2048  # the engine's activations have 4096 bytes of slack: conv rows read a little past the last frame
    p = dict(kind=kind, d=d, batch=clips, M=T, t_pad=t_pad)
    b = {}

    def inputs(rows, cols, N, K, hidden=False, extra=0):
        a, w, bias = gemm_inputs(rng, (rows, cols), (N, K), N, dt, family, k_hidden=hidden)
        b["A"] = np.concatenate([a.ravel(), np.zeros(extra, np.uint16)])
        b["W"], b["bias"] = w.ravel(), bias
        p.update(A="A", W="W", bias="bias", N=N, K=K)

    if kind == "conv1":
        K = (3 * nm + 63) // 64 * 64
        inputs(clips * mel_rows, nm, d, K, extra=tail)
        b["h1"] = sentinel(clips * h1_rows * d, 2)
        p.update(epi=EPI_GELU, lda=nm, a_bs=mel_rows * nm, C="h1", C_off=d, ldc=d, c_bs=h1_rows * d, M=frames)
    elif kind == "conv2":
        inputs(clips * h1_rows, d, d, 3 * d, extra=tail)
        b["pos"] = rng.uniform(-1, 1, T * d).astype(np.float32)
        b["x"] = sentinel(clips * T * d, 4)
        p.update(epi=EPI_GELU_POS, lda=2 * d, a_bs=h1_rows * d, aux="pos", C="x", ldc=d, c_bs=T * d)
    elif kind in ("qkv", "qk", "v"):
        inputs(clips * T, d, 3 * d, d)
        b["q"], b["k"], b["vt"] = sentinel(clips * T * d, 2), sentinel(clips * T * d, 2), sentinel(clips * d * t_pad, 2)
        p.update(epi=EPI_QKV, lda=d, a_bs=T * d, C="q", c_bs=T * d, C2="k", c2_bs=T * d, C3="vt", c3_bs=d * t_pad, ldc=0,
                 qkv_part={"qkv": 0, "qk": 1, "v": 2}[kind])
    elif kind in ("oproj_resid", "ffn2_resid", "oproj_part", "ffn2_part"):
        K = d if kind.startswith("oproj") else 4 * d
        inputs(clips * T, K, d, K, hidden=K != d)
        p.update(lda=K, a_bs=T * K, ldc=d, c_bs=T * d)
        if kind.endswith("resid"):
            b["x"] = rng.standard_normal(clips * T * d).astype(np.float32)
            p.update(epi=EPI_RESID, C="x")
        else:
            b["part"] = sentinel((ksplit + 1) * (clips + 1) * T * d, 4)  # one slab and one clip more than the launch writes
            p.update(epi=EPI_PARTIAL, ksplit=ksplit, part="part", part_stride=(clips + 1) * T * d)
    elif kind in ("ffn1", "bias"):  # "bias": EPI_BIAS_BF16 at mlp.0's shape (no launch of the encoder uses it; the kernels have it)
        inputs(clips * T, d, 4 * d, d)
        b["ffn"] = sentinel(clips * T * 4 * d, 2)
        p.update(epi=EPI_GELU if kind == "ffn1" else EPI_BIAS, lda=d, a_bs=T * d, C="ffn", ldc=4 * d, c_bs=T * 4 * d)
    elif kind == "cross":
        nbt = clips + 2
        inputs(clips * T, d, 2 * n_layer * d, d)
        b["slots"] = np.array([nbt - 1 - 2 * i if nbt - 1 - 2 * i >= 0 else 2 * (clips - 1 - i) + (nbt % 2) for i in range(clips)], dtype=np.int32)
        assert len(set(b["slots"].tolist())) == clips and b["slots"].max() < nbt and list(b["slots"]) != list(range(clips))
        n = n_layer * nbt * d * t_pad
        b["ck"], b["cv"] = sentinel(n, 2), sentinel(n, 2)
        p.update(epi=EPI_CROSS_KV, lda=d, a_bs=T * d, C="ck", C2="cv", ldc=0, c_bs=0, n_layer=n_layer, nbt=nbt, slot_map="slots")
    else:
        raise ValueError(kind)
    return p, b


def launches(p):
    """[(first column, column count)] of the launch_one calls of this launch_gemm."""
    d = p["d"]
    if p["epi"] == EPI_QKV:
        return ([(0, 2 * d)] if p["qkv_part"] != 2 else []) + ([(2 * d, d)] if p["qkv_part"] != 1 else [])
    if p["epi"] == EPI_CROSS_KV:
        return [(0, p["n_layer"] * d), (p["n_layer"] * d, p["n_layer"] * d)]
    return [(0, p["N"])]
