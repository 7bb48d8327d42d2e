"""Float64 restatement of the FP8 cross K/V format (csrc/decode_layout.hpp "FP8 cross K/V", csrc/cross_kv_fp8.hip): the e4m3fn code
table, the power-of-two scale rule, the quantiser, the device index maps, and the attention reference with its derived bound.
Nothing here reads the engine's code; tests/test_cross_fp8_reference.py compares the index maps with a host printer built from the
header, and the GPU tests compare the kernels with these functions.

Codes: OCP e4m3fn, sign | 4-bit exponent (bias 7) | 3-bit mantissa; exponent 0 is subnormal (m / 8 * 2^-6), 0x7f / 0xff are NaN, the
largest finite value is 0x7e = 448. Scale of a channel (one head dimension of a (layer, slot, head, K or V) over the clip's valid
keys): 2^e with the smallest integer e such that amax * 2^-e <= 448, kept in [-126, 120]; e = 0 for an all-zero channel. x * 2^-e is
exact in fp32 for the 16-bit inputs, so a code is ONE round-to-nearest-even of an exact value: the comparison with the kernel is
bit for bit."""
import math

import numpy as np

E_MIN, E_MAX = -126, 120
FP8_MAX = 448.0
KV_DIM, BLOCK_KEYS = 64, 64
U32 = 2.0 ** -24


def code_table():
    """float64 [256]: the value of every code (NaN for 0x7f and 0xff)."""
    t = np.empty(256)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = math.nan
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t


TABLE = code_table()


def scale_exponent(amax):
    """The exponent e of a channel whose largest magnitude is amax (float, >= 0)."""
    amax = float(amax)
    if amax == 0.0:
        return 0
    f, k = math.frexp(amax)  # amax = f 2^k, f in [0.5, 1); 448 = 0.875 * 2^9
    e = k - 9 if f <= 0.875 else k - 8
    return min(max(e, E_MIN), E_MAX)


def encode(y):
    """Codes of the exact values y (float64, |y| <= 448), round to nearest even; the sign of y (of -0.0 too) is kept."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    assert (a <= FP8_MAX).all()
    _, k = np.frexp(a)
    E = np.where(a < 2.0 ** -6, -6, k - 1)  # the binade's exponent; everything below 2^-6 (zero too) has the subnormal spacing 2^-9
    q = np.rint(a / np.exp2((E - 3).astype(np.float64))).astype(np.int64)  # 0 .. 16 (np.rint rounds halves to even); 16 carries
    code = ((E + 6).astype(np.int64) << 3) + q
    assert (code <= 0x7e).all()
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def quantize(x, n_keys=None):
    """x [..., keys, channels] (values of the 16-bit storage type, any float dtype) -> (codes uint8 like x, exponents int
    [..., channels]). Keys at or beyond n_keys take no part in amax and get code 0."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-2] if n_keys is None else n_keys
    amax = np.abs(x[..., :n, :]).max(axis=-2) if n > 0 else np.zeros(x.shape[:-2] + x.shape[-1:])
    e = np.vectorize(scale_exponent, otypes=[np.int64])(amax)
    y = x * np.exp2(-e.astype(np.float64))[..., None, :]
    y[..., n:, :] = 0.0
    return encode(y), e


def scales_of(e):
    return np.exp2(np.asarray(e, dtype=np.float64)).astype(np.float32)


def dequantize(codes, scales):
    """codes [..., keys, channels] uint8, scales [..., channels] -> float64 values."""
    return TABLE[codes] * np.asarray(scales, dtype=np.float64)[..., None, :]


# ------------------------------------------------------------------ inputs that exercise the format
def channel_families(rng, n, narrow):
    """[n][64] values of the 16-bit type: one channel per case the format has to get right."""
    x = rng.standard_normal((n, 64))
    x[:, 1] = 0.0                                   # a zero channel
    x[:, 2] = -np.abs(x[:, 2]) - 0.01               # an all-negative channel
    x[:, 3] *= 30.0                                 # a channel 30x the others
    x[:, 4] *= 2.0 ** -12                           # a small channel
    x[:, 5] = rng.integers(-448, 449, n) / 2.0      # halves up to 224: e = -1, the scaled values are integers, odd ones in [16, 32) etc. exact ties
    x[0, 5] = 224.0
    x[1:9, 5] = np.array([17, -19, 21, -23, 25, -27, 29, -31]) / 2.0
    x[:, 6] = rng.integers(-7, 8, n) * 2.0 ** -9    # multiples of the smallest subnormal code ...
    x[0, 6] = 256.0                                 # ... beside one key that sets e = 0: subnormal codes
    x[:, 7] = 448.0 * np.sign(x[:, 7])              # amax exactly 448 * 2^0
    x[:, 8] = 449.0 * rng.uniform(0.1, 1, n)
    x[1, 8] = 450.0                                 # amax just above 448: the next exponent
    return narrow(x)


# ------------------------------------------------------------------ device index maps (bytes within one (slot, head) image)
def k8_index(key, dim):
    """blocked [key / 64][dim / 16][key % 64][16]"""
    return (key >> 6) * 4096 + (dim >> 4) * 1024 + (key & 63) * 16 + (dim & 15)


def v8_index(key, dim):
    """row-major [key][64]"""
    return key * 64 + dim


def scale_index(layer, slot, head, kv, dim, n_slots, n_head):
    """fp32 [layer][slot][head][K, V][64]"""
    return (((layer * n_slots + slot) * n_head + head) * 2 + kv) * 64 + dim


def store_k8(codes, keys_pad, fill=0):
    """codes [keys][64] of one (slot, head) -> the blocked image [keys_pad * 64] (bytes the keys do not reach: fill)."""
    out = np.full(keys_pad * 64, fill, dtype=np.uint8)
    key, dim = np.meshgrid(np.arange(codes.shape[0]), np.arange(64), indexing="ij")
    out[k8_index(key, dim)] = codes
    return out


def load_k8(image, n_keys):
    key, dim = np.meshgrid(np.arange(n_keys), np.arange(64), indexing="ij")
    return image[k8_index(key, dim)]


# ------------------------------------------------------------------ attention over the codes
def attn_chain(cap_blocks, n_split):
    """Rescales a partial result of decode_cross_attention_fp8_kernel goes through: a wave takes two blocks per iteration, blocks
    blk and blk + 4 of every eight, then the fold over the four waves and over the splits."""
    return (cap_blocks + 7) // 8 + n_split + 2


def attn_expect(q, dq, k_codes, v_codes, k_scale, v_scale, cap_blocks, n_split):
    """One (clip, head): q, dq [64] float64; codes [n_keys][64]; scales [64]. The kernel forms q * k_scale (exact), attends over
    the code VALUES and multiplies the normalised output by v_scale (exact): decode_kernel_reference.softmax_expect on exactly those
    operands, its error scaled with the output. Returns (o, E) without the output pair's own rounding."""
    from decode_kernel_reference import softmax_expect

    ks, vs = np.asarray(k_scale, dtype=np.float64), np.asarray(v_scale, dtype=np.float64)
    o, e, _, _ = softmax_expect(q * ks, dq * ks, TABLE[k_codes], TABLE[v_codes], attn_chain(cap_blocks, n_split))
    return o * vs, e * vs
