"""GPU: decode_cross_attention_group_kernel alone, through tests/cpp/cross_group_driver.cpp linked against the shipped object: the whole
per-slot output pair against float64 attention over the same h16 K/V and fp32 query inputs, under the per-element bound DESIGN.md
"Shared cross K/V" derives (expect() below states it). Slot s is rank s % K of clip s // K and attends over the K/V of slot s // K; the
K/V slot behind the clips and, in half of the cases, the rows beyond the key limit hold NaN bits."""
import numpy as np
import pytest

from decode_kernel_reference import (SCORE_FAMILIES, SENT16, U32, PairExpect, attn_qkv, check_pair, frag_index, kv_store, ln_rows,
                                     pair_err, query_expect, realistic_stream, sentinel, softmax_expect, to_bits, typed, weights)
from encoder_kernel_reference import u16
from kernel_driver import DTYPES, driver_exe
from test_gpu_cross_fp8_kernels import inner, run  # (one driver process over a manifest; a dump without its guards)

pytestmark = pytest.mark.gpu
H, D = 3, 192  # heads of 64, d_model


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, driver_exe(request.param, "cross_group_driver.cpp", linked=("decode_attention_group", "cross_kv_fp8"))  # (the driver shares cross_fp8_driver.cpp)


def inputs(dt, seed, mode, K, clips, cap, n_keys, nan_pad):
    """Buffers and keys of a launch over clips x K slots; the natural K / V [clips][H][n_keys][64] the reference attends over."""
    rng, S = np.random.default_rng(seed), clips * K
    nbs = (S + 15) // 16
    q = np.zeros((S, D), np.float32)
    kn, vn = np.zeros((clips, H, cap * 64, 64)), np.zeros((clips, H, cap * 64, 64))
    kn[:], vn[:] = (np.nan, np.nan) if nan_pad else (3e4, -3e4)  # rows at or beyond the key limit
    for c in range(clips):
        for h in range(H):
            for r in range(K):
                fam = SCORE_FAMILIES[(c * H + h + r + seed) % len(SCORE_FAMILIES)] if mode == "q" else "flat"
                qq, k1, v1 = attn_qkv(rng, n_keys, dt, fam)
                q[c * K + r, h * 64:h * 64 + 64] = qq
                if r == 0:  # (the K/V of rank 0's family; the other ranks meet it with queries of their own)
                    kn[c, h, :n_keys], vn[c, h, :n_keys] = k1, v1
    stride = H * cap * 4096
    pad = sentinel(stride, 2)  # clip c's K/V in slot c; one slot of NaN bits behind the clips
    b = dict(k=np.concatenate([kv_store(kn, stride, dt, True, SENT16), pad]), v=np.concatenate([kv_store(vn, stride, dt, False, SENT16), pad]),
             out_hi=sentinel(D // 32 * nbs * 512, 2), out_lo=sentinel(D // 32 * nbs * 512, 2))
    p = dict(group=K, n_slots=S, kv_slots=clips + 1, n_head=H, d_model=D, n_keys=n_keys, cap_blocks=cap, nbs=nbs, k="k", v="v", out_hi="out_hi",
             out_lo="out_lo", batch=S)
    if mode == "q":
        b["q"], p["q"] = q, "q"
    elif mode == "fused":
        x, g, be, _ = realistic_stream(rng, S, D) if seed % 2 else (ln_rows(rng, S, D), rng.uniform(0.5, 1.5, D).astype(np.float32), rng.uniform(-1, 1, D).astype(np.float32), ())
        b.update(x=x.astype(np.float32), ln_w=g, ln_b=be, wq=to_bits(weights(rng, D, D, dt, "realistic"), dt), bq=rng.uniform(-1, 1, D).astype(np.float32))
        p.update(x="x", ln_w="ln_w", ln_b="ln_b", wq="wq", bq="bq")
    else:  # folded: T rows, the block statistics of a residual row, two constant vectors, all taken as given
        xr = ln_rows(rng, S, D).astype(np.float64).reshape(S, D // 16, 16)
        s1 = xr.sum(2)
        b.update(tq=rng.standard_normal((S, D)).astype(np.float32), stat=np.stack([s1, ((xr - s1[..., None] / 16) ** 2).sum(2)], axis=2).astype(np.float32).ravel(),
                 fold_s=rng.standard_normal(D).astype(np.float32), fold_c=rng.standard_normal(D).astype(np.float32))
        p.update(tq="tq", stat_part="stat", fold_s="fold_s", fold_c="fold_c")
    return b, p, kn[:, :, :n_keys], vn[:, :, :n_keys]


def expect(dt, b, p, kn, vn, slots, done):
    """PairExpect of the slots in `slots` that are not done."""
    K, cap, ns, n = p["group"], p["cap_blocks"], p["n_split"], p["n_keys"]
    q, dq = query_expect(p, typed(p, b), dt)
    dq = dq + pair_err(np.abs(q) + dq, dt) + 64 * U32 * (np.abs(q) + dq)
    pe = PairExpect(b["out_hi"].size)
    for s in slots:
        for h in range(H if not done[s] else 0):
            k, v = kn[s // K, h], vn[s // K, h]
            o, e, smax, _ = softmax_expect(q[s, h * 64:h * 64 + 64], dq[s, h * 64:h * 64 + 64], k, v, (cap + 3) // 4 + ns + 2)
            w = np.exp(0.125 * (k @ q[s, h * 64:h * 64 + 64]) - smax)
            pr, av = w / w.sum(), np.abs(v)
            e = e + 2 * (u16(dt) ** 2 * (pr @ av) + (2.0 ** -25 * av.sum(0) if dt == "f16" else 0.0) + (n + 1) * U32 * (pr @ av))
            pe.put(frag_index(s, h * 64 + np.arange(64), p["nbs"]), o, e + pair_err(np.abs(o) + e, dt))
    return pe


MODES = ("q", "fused", "folded")
ONCE, TWICE = ((0, None),), ((0, None), (0, None))  # launch ranges (slot0, nslots; None: all); TWICE: a second launch on the tickets the first one left
CUT = ((0, 16), (16, 4))  # K = 5, 20 slots: clip 3 (slots 15 .. 19) is cut; its twin case runs the same inputs in one launch
CASES = [  # (mode, K, n_keys, cap_blocks, n_split, done slots, done_late, NaN rows beyond the keys, clips, launch ranges)
    *[(m, (1, 2, 5, 8)[(i + j) % 4], 1500, 24, s, (), 0, (i + j) % 2 == 0, 3, TWICE if s in (3, 6) else ONCE) for i, m in enumerate(MODES) for j, s in enumerate((1, 2, 3, 4, 6))],
    *[(MODES[j % 3], (8, 5, 2, 1, 5)[j], n, 24 if j % 2 else 4, 1 + j % 2, (), j % 2, n % 2 == 0, 3, ONCE) for j, n in enumerate((1, 63, 64, 65, 128))],
    ("q", 5, 1500, 24, 2, (6,), 0, True, 3, ONCE), ("fused", 5, 1500, 24, 2, (6,), 1, False, 3, ONCE),      # one done rank of clip 1
    ("folded", 5, 100, 2, 2, (5, 6, 7, 8, 9), 0, True, 3, ONCE), ("q", 2, 100, 2, 1, (2, 3), 1, True, 3, ONCE),  # every rank of clip 1 done
    *[(m, 5, 1500, 24, s, (), 0, True, 4, r) for m, s in (("fused", 1), ("folded", 3)) for r in (CUT, ONCE)],
]


def test_group_kernel_against_float64(driver, tmp_path):
    """Every launch: float64 on the slots of the ranges so far, the sentinel elsewhere, tickets back at zero; a cut range is its twin bit for bit."""
    dt, _ = driver
    bufs, launches, checks = {}, [], []
    for ci, (mode, K, n_keys, cap, ns, done_slots, late, nan_pad, clips, ranges) in enumerate(CASES):
        S = clips * K
        b, p, kn, vn = inputs(dt, 300 + 7 * K + ns + n_keys % 11 + len(mode), mode, K, clips, cap, n_keys, nan_pad)  # (twins share a seed)
        b.update(done=np.isin(np.arange(S), done_slots).astype(np.int32), mpart=sentinel(S * H * ns * 66, 4), mcnt=np.zeros(S * H, np.int32))
        p.update(n_split=ns, done_late=late, done="done", mpart="mpart", mcnt="mcnt")
        names = {k: f"c{ci}.{k}" for k in b}
        bufs.update({names[k]: v for k, v in b.items()})
        pp = {k: (names[v] if isinstance(v, str) and v in names else v) for k, v in p.items() if k != "batch"}
        seen = []
        for li, (s0, n) in enumerate(ranges):
            n = S if n is None else n
            seen = seen + list(range(s0, s0 + n))
            launches.append(("attng", f"{ci}.{li}", dict(pp, slot0=s0, nslots=n), [names[o] for o in ("out_hi", "out_lo", "mcnt")]))
            checks.append((ci, f"{mode}.K{K}.keys{n_keys}.s{ns}.{s0}+{n}", b, p, kn, vn, names, sorted(set(seen)), (ns, H, (s0 + n - 1) // K - s0 // K + 1)))
    grids, got = run(driver, str(tmp_path), bufs, launches, timeout=300)
    worst, final = {}, {}
    for (_, lid, _, _), (ci, ident, b, p, kn, vn, names, slots, grid), g in zip(launches, checks, got):
        assert grids[lid] == grid, (ident, grids[lid])
        w = check_pair(ident, g[names["out_hi"]], g[names["out_lo"]], b["out_hi"], b["out_lo"], expect(dt, b, p, kn, vn, slots, b["done"]), dt)
        assert w <= 1.0 and not inner(g[names["mcnt"]]).any(), (dt, ident, w, "error / bound, or tickets left")
        worst[ident.split(".")[0]] = max(worst.get(ident.split(".")[0], 0.0), w)
        final.setdefault(CASES[ci][:9], {})[CASES[ci][9]] = (g[names["out_hi"]], g[names["out_lo"]])
    for form, w in sorted(worst.items()):
        print(f"{dt} grouped cross-attention, query mode {form}: worst error / bound {w:.4f}")
    twins = [v for v in final.values() if len(v) == 2]
    assert len(twins) == 2 and all(np.array_equal(v[CUT][i], v[ONCE][i]) for v in twins for i in (0, 1))
