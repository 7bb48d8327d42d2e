"""Float64 reference of the persistent launches' 64-key attention block (attn_block / attn_block_regs in
whisper.axera_amd/csrc/decode_persistent_common.hpp), the operand index maps of its matrix-pipe form stated independently of
csrc/decode_layout.hpp, and a per-element bound derived from the arithmetic in the notation of tests/decode_kernel_reference.py:
u = 2^-24, u16 = 2^-8 (bfloat16) / 2^-11 (half). First order, worst case, for a block that does the stated arithmetic in fp32 in
ANY order; the first-order terms carry a factor 2 for what first order leaves out.

The block: one wave, 64 keys, 64 dims. Inputs: the query as a stored pair (q = hi + lo EXACTLY, so the reference uses exactly
that), K and V in the 16-bit type (exact), a valid flag per key.
  scores   s_j = 0.125 sum_d (hi_d + lo_d) k_jd: 128 products of two 16-bit values, exact in fp32, added in fp32 in some order (the
           matrix instruction's accumulation included) and the two halves joined by one more addition:
               ds_j = 0.125 * 129 u sum_d (|hi_d| + |lo_d|) |k_jd| + u |s_j|
  m        the maximum of the computed scores of the valid keys: |m - s_max| <= dm = max_j ds_j
  p_j      __expf(s_j - m) = exp2((s_j - m) log2 e) with v_exp_f32: the subtraction and the product are worth u |s_j - m| each in
           the result, the instruction 2 u; against exp(s_j - s_max) of the reference the computed m adds dm:
               eps_j = ds_j + dm + u (3 + 2 (s_max - s_j))                    (relative)
  l        64 terms added in fp32:            E_l = sum_j p_j eps_j + 64 u l
  o_d      p_j is stored as a pair of the 16-bit type: pair_err(p) = u16^2 p (+ 2^-25 in half, where a small p is subnormal); then
           128 exact products added in fp32 and the halves joined:
               E_o = sum_j (p_j eps_j + pair_err(p_j)) |v_jd| + 129 u sum_j p_j |v_jd|
  A block without a valid key records m = -inf, l = 0, o = 0 exactly. A masked key's K row never reaches the result (it may hold
  NaN); a masked key's V row is multiplied by p = 0 and has to be finite.

Operand maps of v_mfma_f32_16x16x32 (lane l: A[row l % 16][k = 8 (l / 16) + j], B[k = 8 (l / 16) + j][col l % 16], result register
r of lane l: D[row 4 (l / 16) + r][col l % 16]), as this block uses them:
  A (both products)   even rows the hi half of the pair, odd rows the lo half: lane l reads the 16 bytes at dword
                      32 (l % 2) + 16 ks + 4 (l / 16) of the packed pairs ([32] hi dwords, then [32] lo), 2 values per dword
  B, scores           block kb, k-step ks: lane l holds dims 32 ks + 8 (l / 16) + j of key 16 kb + l % 16: one 16-byte piece of the
                      blocked K [dim / 8][key][8]
  B, output, VT       block nb, k-step ks: keys 32 ks + 8 (l / 16) + j of dim 16 nb + l % 16: one piece of the transposed V
                      [key / 8][dim][8 keys]
  B, output, rows     the same elements out of row-major V [key][64] by two ds_read_b64_tr_b16: in each group of 16 lanes, lane
                      4 q + p supplies the address of 4 elements (row q, columns 4 p .. 4 p + 3 of a 4 x 16 block) and lane i
                      receives column i of the four rows
  result              lane l takes register 0 + register 1 of accumulator l / 16: the score of key l, then o[l]
"""
import numpy as np

from encoder_kernel_reference import U32, from_bits, round16, to_bits, u16

VALID_COUNTS = (0, 1, 9, 17, 28, 33, 63, 64)  # 28: the last block of 1500 audio keys; 0: the all-masked block
FORMS = {"rows": 0, "vt": 1, "regs": 2}       # V home: row-major cross tile, transposed self cache (LDS), transposed (registers)
LANES = np.arange(64)


# ------------------------------------------------------------------------------------------ layouts, restated
def k_offset(key, dim):
    """blocked K of one 64-key block: [dim / 8][key][8]"""
    return ((np.asarray(dim) >> 3) * 64 + np.asarray(key)) * 8 + (np.asarray(dim) & 7)


def vt_offset(key, dim):
    """transposed V of one block: [key / 8][dim][8 keys]"""
    return ((np.asarray(key) >> 3) * 64 + np.asarray(dim)) * 8 + (np.asarray(key) & 7)


def v_offset(key, dim):
    """row-major V of one block: [key][64]"""
    return np.asarray(key) * 64 + np.asarray(dim)


# ------------------------------------------------------------------------------------------ operand maps
def a_words(ks):
    """[64 lanes][4]: dword index into the packed pairs ([32] hi, [32] lo) of lane l's A fragment of k-step ks."""
    return (32 * (LANES % 2) + 16 * ks + 4 * (LANES // 16))[:, None] + np.arange(4)[None, :]


def a_fragment(packed, ks):
    """[64 lanes][8] uint16: the A fragment out of 64 packed dwords (low half-word = the even element)."""
    w = np.asarray(packed, dtype=np.uint32)[a_words(ks)]
    return np.stack([w & 0xFFFF, w >> 16], axis=-1).reshape(64, 8).astype(np.uint16)


def b_piece(blk, ks):
    """(row [64][8], k [64][8]) of a B fragment read as ONE 16-byte piece: row = 16 blk + l % 16 (key of the scores, dim of the
    output), k = 32 ks + 8 (l / 16) + j (dim of the scores, key of the output); and the piece's element offset [64]."""
    row = np.broadcast_to((16 * blk + LANES % 16)[:, None], (64, 8))
    k = (32 * ks + 8 * (LANES // 16))[:, None] + np.arange(8)[None, :]
    return row, k, ((4 * ks + LANES // 16) * 64 + 16 * blk + LANES % 16) * 8


def tr_read(addr):
    """ds_read_b64_tr_b16: addr [64] element offsets supplied by the lanes -> [64][4] element offsets each lane receives."""
    out = np.empty((64, 4), dtype=np.int64)
    for g in range(4):
        for i in range(16):
            for q in range(4):
                out[16 * g + i, q] = addr[16 * g + 4 * q + i // 4] + i % 4
    return out


def b_rows_addresses(nb, ks):
    """the two address vectors [64] a wave supplies for B (nb, ks) of the output out of row-major V."""
    g, q, p = LANES // 16, (LANES // 4) % 4, LANES % 4
    a = v_offset(32 * ks + 8 * g + q, 16 * nb + 4 * p)
    return a, a + 4 * 64


def b_rows(nb, ks):
    """[64][8] element offsets into row-major V that lane l ends up with in fragment element j."""
    a0, a1 = b_rows_addresses(nb, ks)
    return np.concatenate([tr_read(a0), tr_read(a1)], axis=1)


def pick(acc):
    """acc [4 blocks][16 rows][16 cols] -> [64]: lane l takes D[4 (l / 16)][l % 16] + D[4 (l / 16) + 1][l % 16] of accumulator l / 16."""
    g, c = LANES // 16, LANES % 16
    return acc[g, 4 * g, c] + acc[g, 4 * g + 1, c]


def mfma(a_bits, b_bits, dt):
    """one v_mfma_f32_16x16x32 on fragments [64][8] (bit patterns): D [16][16], exact operands, float64 accumulation."""
    a, b = from_bits(a_bits, dt).reshape(4, 16, 8), from_bits(b_bits, dt).reshape(4, 16, 8)  # [k / 8][row or col][k % 8]
    return np.einsum("grj,gcj->rc", a, b)


def emulate(form, q_packed, k_bits, v_bits, nvalid, dt):
    """The matrix-pipe block through the maps above on one block's LDS images (k_bits blocked K; v_bits row-major for form "rows",
    transposed else): fp32 at the kernel's rounding points (scores, probabilities, the pair), float64 inside a product."""
    acc = np.zeros((4, 16, 16))
    for kb in range(4):
        for ks in range(2):
            acc[kb] += mfma(a_fragment(q_packed, ks), k_bits[b_piece(kb, ks)[2][:, None] + np.arange(8)], dt)
    with np.errstate(over="ignore", invalid="ignore"):  # a masked column may hold anything
        s = (pick(acc).astype(np.float32) * np.float32(0.125)).astype(np.float64)
    s[LANES >= nvalid] = -np.inf
    m = s.max()
    if m == -np.inf:
        return -np.inf, 0.0, np.zeros(64)
    p = np.exp(s - m).astype(np.float32)
    hi = round16(p, dt)
    lo = round16(p - hi, dt)
    pp = np.concatenate([to_bits(hi, dt).view(np.uint16).reshape(32, 2), to_bits(lo, dt).view(np.uint16).reshape(32, 2)])
    packed = pp[:, 0].astype(np.uint32) | (pp[:, 1].astype(np.uint32) << 16)
    oc = np.zeros((4, 16, 16))
    for nb in range(4):
        for ks in range(2):
            at = b_rows(nb, ks) if form == "rows" else b_piece(nb, ks)[2][:, None] + np.arange(8)
            oc[nb] += mfma(a_fragment(packed, ks), v_bits[at], dt)
    return m, float(p.astype(np.float64).sum()), pick(oc)


# ------------------------------------------------------------------------------------------ reference and bound
def pair_err(ax, dt):
    return u16(dt) ** 2 * np.abs(ax) + (2.0 ** -25 if dt == "f16" else 0.0)


def block_expect(q_hi, q_lo, k, v, nvalid):
    """q_hi, q_lo [64], k, v [64 keys][64] float64 (rows >= nvalid ignored). Returns None for a block without a valid key, else
    dict(m, dm, l, El, o, Eo)."""
    if nvalid == 0:
        return None
    k, v = k[:nvalid], v[:nvalid]
    s = 0.125 * (k @ (q_hi + q_lo))
    ds = 0.125 * 129 * U32 * (np.abs(k) @ (np.abs(q_hi) + np.abs(q_lo))) + U32 * np.abs(s)
    m, dm = s.max(), ds.max()
    p = np.exp(s - m)
    eps = ds + dm + U32 * (3 + 2 * (m - s))
    l = p.sum()
    av = np.abs(v)
    return dict(m=m, dm=dm, l=l, El=2 * ((p * eps).sum() + 64 * U32 * l) + 1e-300, o=p @ v, p=p, eps=eps, av=av)


def output_bound(r, dt):
    return 2 * ((r["p"] * r["eps"] + pair_err(r["p"], dt)) @ r["av"] + 129 * U32 * (r["p"] @ r["av"])) + 1e-300


def check_record(name, rec, r, dt):
    """One partial record (m, l, o[64]) of a block against block_expect's result. Returns the worst error / bound."""
    m, l, o = float(rec[0]), float(rec[1]), np.asarray(rec[2:66], dtype=np.float64)
    if r is None:
        assert m == -np.inf and l == 0.0 and not o.any() and np.isfinite(o).all(), f"{name}: a block without keys recorded m {m} l {l} o {o}"
        return 0.0
    assert np.isfinite(m) and np.isfinite(l) and np.isfinite(o).all(), f"{name}: m {m} l {l}, finite o: {np.isfinite(o).all()}"
    wm, wl = abs(m - r["m"]) / r["dm"], abs(l - r["l"]) / r["El"]
    assert wm <= 1, f"{name}: m {m} against {r['m']} +- {r['dm']}"
    assert wl <= 1, f"{name}: l {l} against {r['l']} +- {r['El']}"
    eo = output_bound(r, dt)
    ratio = np.abs(o - r["o"]) / eo
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1, f"{name}: o[{i}] {o[i]} against {r['o'][i]}, error {abs(o[i] - r['o'][i]):.3e} = {ratio[i]:.2f} x its bound {eo[i]:.3e}"
    return float(max(wm, wl, ratio[i]))


# ------------------------------------------------------------------------------------------ the cases
def finite_max(dt):
    return 65504.0 if dt == "f16" else 3e38  # the "+-3e38" of a masked K row; half has no such value: its largest


def make_case(dt, seed, counts, garbage):
    """Eight blocks of one workgroup: wave w has counts[w] valid keys. Returns dict(q_packed [64] uint32, q_hi, q_lo [64] float64,
    k, v [8][64][64] float64 natural (key, dim) order, k_bits, v_bits [8][64][64] uint16 natural order, counts).
    The query holds one dim at 30 x the rest; K rows of masked keys hold `garbage`: "huge" (+- the type's largest value) or "nan"
    (quiet and signalling NaN bit patterns, both signs); V rows of masked keys stay finite."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(64).astype(np.float32)
    q[int(rng.integers(64))] *= 30.0
    hi = round16(q, dt)
    lo = round16(q - hi, dt)
    hb, lb = to_bits(hi, dt).astype(np.uint32), to_bits(lo, dt).astype(np.uint32)
    packed = np.concatenate([hb[0::2] | (hb[1::2] << 16), lb[0::2] | (lb[1::2] << 16)]).astype(np.uint32)
    k_bits = to_bits(rng.standard_normal((8, 64, 64)).astype(np.float32), dt).copy()
    v_bits = to_bits((rng.standard_normal((8, 64, 64)) * 2.0).astype(np.float32), dt).copy()
    for w, n in enumerate(counts):
        if garbage == "huge":
            g = to_bits(np.where(rng.random((64 - n, 64)) < 0.5, -1.0, 1.0).astype(np.float32) * np.float32(finite_max(dt)), dt)
        else:
            pats = np.array([0x7FC5, 0xFFC1, 0x7F81 if dt == "bf16" else 0x7D01, 0xFFFF], dtype=np.uint16)
            g = pats[rng.integers(4, size=(64 - n, 64))]
        k_bits[w, n:] = g
    return dict(q_packed=packed, q_hi=hi.astype(np.float64), q_lo=lo.astype(np.float64), k=from_bits(k_bits, dt), v=from_bits(v_bits, dt),
                k_bits=k_bits, v_bits=v_bits, counts=tuple(counts))


def lds_images(case, form):
    """(K [8][4096], V [8][4096]) uint16 as the block finds them: blocked K; V row-major ("rows") or transposed."""
    key, dim = np.arange(64)[:, None], np.arange(64)[None, :]
    K = np.empty((8, 4096), dtype=np.uint16)
    V = np.empty((8, 4096), dtype=np.uint16)
    K[:, k_offset(key, dim)] = case["k_bits"]
    V[:, v_offset(key, dim) if form == "rows" else vt_offset(key, dim)] = case["v_bits"]
    return K, V
