"""GPU: decode_self_attention_tree_kernel alone, through Whisper.beam_tree_attention (AX_WHISPER_BeamTreeAttention), against float64
attention over the keys gathered by the origin table, under the per-element bound DESIGN.md "Tree self-attention" derives: the grouped
cross-attention kernel's bound for a query read from a buffer and one split (tests/test_gpu_cross_group_kernel.py), plus one fp32
rounding of hi + lo, which the call returns as one float. The gather adds no term: selection is exact, the extra products are exact zeros.
Slot s is rank s % K of clip s // K. NaN bits sit in every K/V row that no live rank of the clip reads, in every row beyond the offset,
in the K/V slot behind the last clip; origin entries at and beyond the offset hold a slot index that does not exist."""
import numpy as np
import pytest

from attn_block_reference import pair_err
from conftest import ModelCase
from decode_kernel_reference import SCORE_FAMILIES, SENT16, U32, attn_qkv, softmax_expect
from encoder_kernel_reference import to_bits, u16

pytestmark = pytest.mark.gpu
PATTERNS = ("identity", "one_slot", "per_block", "random", "unreferenced")


@pytest.fixture(scope="module", params=[("micro", 11, "BF16"), ("miniturbo", 21, "F16")], ids=["micro_bf16", "miniturbo_fp16"])
def handle(request, built_lib, oracle_mod, tmp_path_factory):
    model_type, seed, dtype = request.param
    case = ModelCase(tmp_path_factory.mktemp("tree_" + model_type), model_type, seed, dtype=dtype)
    e = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=1)
    yield e, dtype.lower(), {}
    e.close()


def origin_rows(rng, pattern, K, c, off):
    """[K][off]: the local slot rank r of clip c reads position p from."""
    p = np.arange(off)
    if pattern == "one_slot":
        return np.full((K, off), (c + 1) % K)
    if pattern == "per_block":
        return np.tile((p // 64 + c) % K, (K, 1))
    if pattern == "random":
        return rng.integers(K, size=(K, off))
    if pattern == "unreferenced" and K > 1:  # slot c % K is read by nobody below the offset
        return (c % K + 1 + rng.integers(K - 1, size=(K, off))) % K
    return np.tile(np.arange(K)[:, None], (1, off))


def run(handle, K, n_keys, pattern, done=(), ranges=((0, None),), launches=1, clips=3):
    """The launches' merged output, the float64 reference and its bound over the live slots, and which slots they are."""
    e, dt, _ = handle
    H, D, cap = e.n_text_state // 64, e.n_text_state, e.n_text_ctx
    S, off = clips * K, n_keys - 1
    rng = np.random.default_rng(1000 * K + 7 * n_keys + PATTERNS.index(pattern))
    q, kf, vf = np.zeros((S, D), np.float32), np.zeros((S + 1, H, cap, 64)), np.zeros((S + 1, H, cap, 64))
    for s in range(S):
        for h in range(H):
            q[s, h * 64:h * 64 + 64], kf[s, h, :n_keys], vf[s, h, :n_keys] = attn_qkv(rng, n_keys, dt, SCORE_FAMILIES[(s + h) % len(SCORE_FAMILIES)])
    live = ~np.isin(np.arange(S), done)
    src = np.empty((S, n_keys), np.int64)  # the GLOBAL slot every (slot, position) is read from
    for c in range(clips):
        src[c * K:c * K + K, :off] = c * K + origin_rows(rng, pattern, K, c, off)
        src[c * K:c * K + K, off] = c * K + np.arange(K)
    origin = np.full((S, cap), 0xEE, np.uint8)
    origin[:, :off] = src[:, :off] % K
    read = np.zeros((S + 1, cap), bool)
    for s in np.nonzero(live)[0]:
        read[src[s], np.arange(n_keys)] = True
    kb, vb = to_bits(kf, dt).reshape(kf.shape), to_bits(vf, dt).reshape(vf.shape)
    kb.transpose(0, 2, 1, 3)[~read], vb.transpose(0, 2, 1, 3)[~read] = SENT16, SENT16  # (slot, position): every head, every dimension
    got = np.full((S, D), np.nan, np.float32)
    for s0, n in ranges:
        o = e.beam_tree_attention(q, kb, vb, origin, np.full(S, off), ~live, K, slot0=s0, nslots=n, launches=launches)
        inside = np.arange(S) >= s0 if n is None else (np.arange(S) >= s0) & (np.arange(S) < s0 + n)
        assert np.isnan(o[~inside | ~live]).all(), "a slot outside the range, or a done one, was written"
        got[inside] = o[inside]
    ref, bound = np.zeros((S, D)), np.zeros((S, D))
    pos = np.arange(n_keys)
    for s in np.nonzero(live)[0]:
        for h in range(H):
            qq = q[s, h * 64:h * 64 + 64].astype(np.float64)
            k, v = kf[src[s], h, pos], vf[src[s], h, pos]
            dq = pair_err(np.abs(qq), dt) + 64 * U32 * np.abs(qq)  # the (hi, lo) image of the query
            o, err, smax, _ = softmax_expect(qq, dq, k, v, (cap // 64 + 3) // 4 + 1 + 2)
            w = np.exp(0.125 * (k @ qq) - smax)
            pr, av = w / w.sum(), np.abs(v)
            err = err + 2 * (u16(dt) ** 2 * (pr @ av) + (2.0 ** -25 * av.sum(0) if dt == "f16" else 0.0) + (n_keys + 1) * U32 * (pr @ av))
            ref[s, h * 64:h * 64 + 64], bound[s, h * 64:h * 64 + 64] = o, err + pair_err(np.abs(o) + err, dt) + U32 * np.abs(o)
    return got, ref, bound, live


CASES = [(K, n, PATTERNS[(i + j) % len(PATTERNS)]) for i, K in enumerate((1, 2, 5, 8)) for j, n in enumerate((1, 63, 64, 65, 128, None))]


@pytest.mark.parametrize("K,n_keys,pattern", CASES, ids=["K%d-keys%s-%s" % c for c in CASES])
def test_tree_kernel_against_float64(handle, K, n_keys, pattern):
    n_keys = handle[0].n_text_ctx if n_keys is None else n_keys
    got, ref, bound, live = run(handle, K, n_keys, pattern)
    assert np.isfinite(got).all()
    w = float((np.abs(got - ref) / bound).max())
    handle[2]["worst"] = max(handle[2].get("worst", 0.0), w)
    print("%s tree self-attention K %d, %d keys, %s: worst error / bound %.4f (so far %.4f)" % (handle[1], K, n_keys, pattern, w, handle[2]["worst"]))
    assert w <= 1.0, (K, n_keys, pattern, w)


# one done rank of clip 1; every rank of clip 1 done (the group returns at once); rows only they read hold NaN bits
@pytest.mark.parametrize("K,done", [(5, (6,)), (5, (5, 6, 7, 8, 9)), (2, (2, 3))], ids=["one_rank", "a_group", "a_group_K2"])
def test_done_ranks_get_no_output(handle, K, done):
    got, ref, bound, live = run(handle, K, 100, "random", done=done)
    assert np.isnan(got[~live]).all() and (np.abs(got[live] - ref[live]) <= bound[live]).all()


def test_a_cut_range_and_a_relaunch_are_one_launch_bit_for_bit(handle):
    """3 x 8: the launches [0, 16) + [16, 24) meet between two clips. 5 x 5: [0, 16) + [16, 25) cut clip 3 (slots 15 .. 19), which both
    launches serve, each writing its own ranks. A second launch on the same buffers changes nothing."""
    one = run(handle, 8, 130, "random")
    cut = run(handle, 8, 130, "random", ranges=((0, 16), (16, 8)))
    twice = run(handle, 8, 130, "random", launches=2)
    assert (np.abs(one[0] - one[1]) <= one[2]).all()
    assert np.array_equal(one[0].view(np.uint32), cut[0].view(np.uint32)) and np.array_equal(one[0].view(np.uint32), twice[0].view(np.uint32))
    one, cut = run(handle, 5, 70, "random", clips=5), run(handle, 5, 70, "random", clips=5, ranges=((0, 16), (16, 9)))
    assert (np.abs(one[0] - one[1]) <= one[2]).all() and np.array_equal(one[0].view(np.uint32), cut[0].view(np.uint32))
