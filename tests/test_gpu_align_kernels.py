"""GPU: the three alignment kernels of csrc/decode_align.hip, each alone on caller buffers (AX_WHISPER_AlignQKSoftmax,
AX_WHISPER_AlignNormalize, AX_WHISPER_AlignDTW), in both 16-bit builds, against float64 with per-element bounds derived from the
rounding points (u = 2^-24, the unit roundoff of fp32):

  QK-softmax   the inputs are exact in the 16-bit type; a score is 64 products accumulated in fp32 (|ds| <= 64 u sum|q k|); the
               exponent's argument is one fma of the score with the rounded scale (log2 e / 8) and the rounded scaled maximum; exp2
               is good to 2 ulp; the row sum is one fp32 add per key plus one rescale per block; one division, one product.
  normalise    P is exact fp32. The column mean is L / 4 + 3 adds and a division, the variance likewise over the centred squares,
               then a square root and a division per element; the median of 7 selects (it moves by no more than its inputs do);
               one fma per head into the matrix.
  DTW          entries are multiples of 2^-6 in [-8, 8]: every fp32 sum is exact and the jumps are those of the numpy float32
               DTW bit for bit, ties included."""
import numpy as np
import pytest

import word_reference as wr
from conftest import ModelCase

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = ((6, 1), (6, 3), (17, 4), (63, 63), (64, 64), (65, 65), (130, 750), (70, 1500))
DTW_SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (64, 65), (65, 64), (130, 750), (445, 1500))


@pytest.fixture(scope="module", params=("BF16", "F16"))
def eng(request, tmp_path_factory, built_lib, oracle_mod):
    case = ModelCase(tmp_path_factory.mktemp("align_" + request.param), "micro", 11, dtype=request.param)
    e = built_lib.Whisper("micro", case.root, "zh", device=0, max_batch=1)
    yield e, request.param
    e.close()


def narrow(a, dtype):
    """values representable in the engine's 16-bit type"""
    if dtype == "F16":
        return a.astype(np.float16).astype(np.float32)
    b = a.astype(np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).view(np.float32)


def qk_case(L, F, n_head, dtype, seed):
    """two ragged clips in slots 2 and 1 of three: (L, F) and a shorter one; NaN behind every key count and every length"""
    rng = np.random.default_rng(seed)
    lens, keys, slots = [L, max(L // 2, 1)], [F, max(F - 3, 1)], [2, 1]
    row0 = [1, 1 + L + 2]  # a gap in front of and between the clips' rows
    rows = row0[1] + lens[1] + 1
    keys_pad = (F + 63) // 64 * 64
    q = np.full((rows, 64 * n_head), np.nan, dtype=np.float32)
    k = np.full((3, n_head, keys_pad, 64), np.nan, dtype=np.float32)
    for c in range(2):
        q[row0[c]: row0[c] + lens[c]] = narrow(rng.normal(0, 1.5, (lens[c], 64 * n_head)), dtype)
        k[slots[c], :, : keys[c]] = narrow(rng.normal(0, 1.5, (n_head, keys[c], 64)), dtype)
    return q, k, row0, lens, keys, slots, keys_pad


@pytest.mark.parametrize("n_head", (2, 4))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_qk_softmax(eng, shape, n_head):
    e, dtype = eng
    L, F = shape
    q, k, row0, lens, keys, slots, keys_pad = qk_case(L, F, n_head, dtype, 7 * L + F)
    heads = [1, 0]  # (the aligned heads (0, 1), (1, 0) of a layer pair arrive as this layer's list)
    rows_pad, f_pad = L + 1, keys_pad
    P = e.align_qk_softmax(q, k, row0, lens, keys, slots, heads, rows_pad, f_pad, fill=np.nan)
    sc = float(np.float32(0.125) * np.float32(1.44269504088896340736))
    worst = 0.0
    for c in range(2):
        n_blocks = (keys[c] + 63) // 64
        for a, h in enumerate(heads):
            qq = q[row0[c]: row0[c] + lens[c], 64 * h: 64 * h + 64].astype(np.float64)
            kk = k[slots[c], h, : keys[c]].astype(np.float64)
            S, absS = qq @ kk.T, np.abs(qq) @ np.abs(kk).T
            ref = wr.head_softmax(qq, kk, keys[c])
            ds = 64 * U * absS
            m = S.max(-1, keepdims=True)
            arg = (S - m) * sc
            darg = (ds + ds.max(-1, keepdims=True)) * sc + (np.abs(S) + np.abs(m)) * sc * 2 * U + U * np.abs(arg)
            rel_term = np.log(2.0) * darg + 4 * U
            rel = rel_term + rel_term.max(-1, keepdims=True) + (keys[c] / 4 + 3 * n_blocks + 24) * U
            bound = rel * ref + 1e-37
            got = P[c, a, : lens[c], : keys[c]].astype(np.float64)
            assert np.isfinite(got).all()
            worst = max(worst, float((np.abs(got - ref) / bound).max()))
            assert (np.abs(got.sum(-1) - 1.0) <= bound.sum(-1) + U).all()  # rows sum to 1 within the bound
            # what the kernel writes and what it leaves: zeros up to the end of the last key block, the fill everywhere else
            assert (P[c, a, : lens[c], keys[c]: n_blocks * 64] == 0).all()
            assert np.isnan(P[c, a, : lens[c], n_blocks * 64:]).all() and np.isnan(P[c, a, lens[c]:]).all()
    print(f"{dtype} qk_softmax {L}x{F} heads {n_head}: worst error / bound {worst:.4f}")
    assert worst <= 1.0


def norm_bound(P, inv):
    """P [heads][L][F] float64 (exact fp32 values) -> (the contribution, its error bound) [L][F]"""
    H, L, F = P.shape
    total, err = np.zeros((L, F)), np.zeros((L, F))
    for h in range(H):
        p = P[h]
        mean = p.mean(0, keepdims=True)
        d = p - mean
        var = (d * d).mean(0, keepdims=True)
        sd = np.sqrt(var)
        dmean = (L / 4 + 4) * U * np.abs(p).mean(0, keepdims=True)
        dd = U * np.abs(d) + dmean
        dvar = (L / 4 + 6) * U * var + 2 * (np.abs(d) * dd).mean(0, keepdims=True)
        rel_sd = 0.5 * dvar / var + U
        z = d / sd
        dz = dd / sd + np.abs(z) * (rel_sd + 2 * U)
        if F > 3:
            pad = np.pad(dz, [(0, 0), (3, 3)], mode="reflect")
            dz = np.max(np.stack([pad[:, k: k + F] for k in range(7)]), axis=0)
        zz = wr.median7(z)
        total += zz * inv
        err += dz * inv + 2 * U * np.abs(total)
    return total, err


@pytest.mark.parametrize("shape", SHAPES + ((6, 7), (6, 8)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_normalize(eng, shape):
    e, dtype = eng
    L, F = shape
    rng = np.random.default_rng(31 * L + F)
    lens, keys, n_align = [L, max(L - 2, 1)], [F, max(F - 1, 1)], 3
    rows_pad, f_pad, m_rows, m_ld = L + 2, (F + 63) // 64 * 64, L + 1, (F + 3) // 4 * 4 + 4
    P = np.full((2, n_align, rows_pad, f_pad), np.nan, dtype=np.float32)
    for c in range(2):
        x = rng.gamma(0.3, 1.0, (n_align, lens[c], keys[c]))
        P[c, :, : lens[c], : keys[c]] = (x / x.sum(-1, keepdims=True)).astype(np.float32)
    fill = rng.normal(0, 1, (2, m_rows, m_ld)).astype(np.float32)
    inv = 1.0 / 5
    got = e.align_normalize(P, lens, keys, fill, inv)
    worst = 0.0
    for c in range(2):
        keep = np.ones((m_rows, m_ld), dtype=bool)
        keep[: lens[c], : keys[c]] = False
        assert np.array_equal(got[c][keep], fill[c][keep])  # untouched elements keep their fill
        inside = got[c, : lens[c], : keys[c]]
        if lens[c] < 2 or keys[c] == 1:
            # one row, or one frame (every probability 1): the standard deviation is zero, 0 / 0 on both sides
            assert np.isnan(inside).all()
            continue
        assert np.isfinite(inside).all()
        ref, bound = norm_bound(P[c, :, : lens[c], : keys[c]].astype(np.float64), float(np.float32(inv)))
        diff = inside.astype(np.float64) - fill[c, : lens[c], : keys[c]] - ref
        bound = bound + 2 * U * (np.abs(fill[c, : lens[c], : keys[c]]) + np.abs(ref)) * n_align
        worst = max(worst, float((np.abs(diff) / bound).max()))
    print(f"{dtype} normalize {L}x{F}: worst error / bound {worst:.4f}")
    assert worst <= 1.0


_DTW_CASES = {}


def dtw_case(shape):
    """the matrices of a shape and their float32 jumps, computed once for both builds"""
    if shape not in _DTW_CASES:
        N, F = shape
        rng = np.random.default_rng(N * 10007 + F)
        mats = [(rng.integers(-512, 513, (N, F)) / 64.0).astype(np.float32), np.full((N, F), 0.5, dtype=np.float32),
                np.where(rng.integers(0, 2, (N, F)) == 1, 1.0, -1.0).astype(np.float32)]
        if N > 2 and F > 2:
            mats.append(mats[0][: N - 1, : F - 2])  # a ragged further clip
        _DTW_CASES[shape] = (mats, [wr.align_path(m, np.float32) for m in mats])
    return _DTW_CASES[shape]


@pytest.mark.parametrize("shape", DTW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dtw_is_the_float32_dtw(eng, shape):
    e, dtype = eng
    N, F = shape
    mats, refs = dtw_case(shape)
    m_rows, m_ld = N + 4, (F + 3) // 4 * 4
    M = np.full((len(mats), m_rows, m_ld), np.nan, dtype=np.float32)
    for c, m in enumerate(mats):
        M[c, 3: 3 + m.shape[0], : m.shape[1]] = m
    lens, keys = [m.shape[0] + 4 for m in mats], [m.shape[1] for m in mats]
    jump = e.align_dtw(M, lens, keys, fill=-7)
    for c, m in enumerate(mats):
        assert np.array_equal(jump[c, : m.shape[0]], refs[c]), (c, shape)
        assert (jump[c, m.shape[0]:] == -7).all()


def test_kernel_calls_refuse_what_they_cannot_index(eng):
    e, _ = eng
    with pytest.raises(RuntimeError):
        e.align_dtw(np.zeros((1, 600, 8), dtype=np.float32), [600], [8])  # more rows than the kernel has threads
    with pytest.raises(RuntimeError):
        e.align_dtw(np.zeros((1, 8, 6), dtype=np.float32), [8], [6])  # a row stride that is no multiple of four floats
    with pytest.raises(RuntimeError):
        e.align_normalize(np.zeros((1, 1, 4, 64), dtype=np.float32), [5], [3], np.zeros((1, 8, 8), dtype=np.float32), 1.0)  # rows beyond P
