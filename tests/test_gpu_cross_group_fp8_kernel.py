"""GPU: decode_cross_attention_group_fp8_kernel alone, through tests/cpp/cross_group_fp8_driver.cpp linked against the shipped object: the
whole per-slot output pair against float64 attention over the DEQUANTISED codes (cross_fp8_reference) and the same fp32 query inputs,
under the h16 grouped kernel's bound on those values plus the one term the K-scale fold adds (expect() below; DESIGN.md "Shared cross
K/V over FP8 codes"). Bytes beyond the key limit and the whole slot behind the clips hold 0x7f (NaN); the launch takes no h16 K/V."""
import numpy as np
import pytest

import cross_fp8_reference as R
import test_gpu_cross_group_kernel as G
from decode_kernel_reference import U32, PairExpect, frag_index, pair_err, query_expect, round16, softmax_expect, typed
from encoder_kernel_reference import u16
from kernel_driver import DTYPES, driver_exe

pytestmark = pytest.mark.gpu
H, H16_INPUTS = G.H, G.inputs  # (the test below runs G's test body with this file's inputs in G.inputs' place)
TINY = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}   # the smallest normal and the largest finite value of the 16-bit type:
HUGE = {"f16": 65504.0, "bf16": 2.0 ** 127 * 1.9921875}  # the extremes of amax, hence of the scale, the quantiser can produce
# G.CASES' tuples, whose eighth field here says "scale extremes" (bytes beyond the keys are NaN codes in every case)
CASES = [c[:7] + (False,) + c[8:] for c in G.CASES] + [("q", K, n, 24, s, (), 0, True, 3, G.ONCE) for K, n, s in ((5, 1500, 2), (8, 1500, 6), (2, 65, 1))]


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    # (the driver shares cross_group_driver.cpp and, through it, cross_fp8_driver.cpp: hence their objects)
    return request.param, driver_exe(request.param, "cross_group_fp8_driver.cpp", linked=("decode_attention_group_fp8", "decode_attention_group", "cross_kv_fp8"),
                                     also=("common.hpp", "decode_layout.hpp", "decode_attention_common.hpp", "decode_attention_group_common.hpp"))


def inputs(dt, seed, mode, K, clips, cap, n_keys, extreme):
    """G.inputs with clip c's K/V as codes and scales in slot c; returns the dequantised K (with K's scales and the flag) and V."""
    b, p, kn, vn = H16_INPUTS(dt, seed, mode, K, clips, cap, n_keys, True)
    kn, vn = kn.copy(), vn.copy()
    if extreme:  # channels 61 .. 63 of K and of V: amax the smallest normal, the largest finite value, zero; a query that lets them count
        rng = np.random.default_rng(seed)
        for x in (kn, vn):
            u = rng.uniform(-1, 1, x.shape[:3])
            u[:, :, n_keys // 2] = 1.0  # (the key that sets amax: neither the first nor the last, which the falling / rising scores single out)
            x[..., 61], x[..., 62], x[..., 63] = round16(u * TINY[dt], dt), round16(u * HUGE[dt], dt), 0.0
        q = b["q"].reshape(clips * K, H, 64)
        q[..., 61], q[..., 62], q[..., 63] = 1e3, np.float32(8.0 / HUGE[dt]), 5.0
    kc, ke = R.quantize(kn)
    vc, ve = R.quantize(vn)
    ksc, vsc = R.scales_of(ke), R.scales_of(ve)
    head = cap * 4096
    k8, v8 = np.full((clips + 1, H, head), 0x7F, np.uint8), np.full((clips + 1, H, head), 0x7F, np.uint8)  # one slot of NaN codes behind the clips
    for c in range(clips):
        for h in range(H):
            k8[c, h] = R.store_k8(kc[c, h], cap * 64, fill=0x7F)
            v8[c, h, :n_keys * 64] = vc[c, h].ravel()
    sc = np.full((clips + 1, H, 2, 64), np.nan, np.float32)
    sc[:clips, :, 0], sc[:clips, :, 1] = ksc, vsc
    for name in ("k", "v"):
        del b[name], p[name]
    b.update(k8=k8.ravel(), v8=v8.ravel(), scales=sc.ravel())
    p.update(k8="k8", v8="v8", scales="scales")
    return b, p, (R.dequantize(kc, ksc), ksc.astype(np.float64), extreme), R.dequantize(vc, vsc)


def expect(dt, b, p, kd, vd, slots, done):
    """G.expect on the dequantised values. The kernel's A operand is the (hi, lo) pair of A_d = q_d 2^(e_d - s), s = max_d (ilogb q_d +
    e_d) - 14 per (slot, head): where A_d is below the type's normal range the pair's error is absolute, 2^-25 (half) / 2^-126
    (bfloat16, taken as flushed) of A, i.e. that times 2^(s - e_d) of q_d — in place of pair_err's own 2^-25 of an unscaled half pair.
    s from the reference q may be one below the kernel's (a q at a binade's edge): one binade of slack."""
    K, cap, ns, n = p["group"], p["cap_blocks"], p["n_split"], p["n_keys"]
    kd, ksc, extreme = kd
    q, dq = query_expect(p, typed(p, b), dt)
    pe = PairExpect(b["out_hi"].size)
    for s in slots:
        for h in range(H if not done[s] else 0):
            c, qs, dqs = s // K, q[s, h * 64:h * 64 + 64], dq[s, h * 64:h * 64 + 64]
            k, v, ks = kd[c, h], vd[c, h], ksc[c, h]
            nz = qs != 0
            shift = (np.floor(np.log2(np.abs(qs[nz]))) + np.log2(ks[nz])).max() - 14 if nz.any() else 0.0
            floor = (2.0 ** -25 if dt == "f16" else 2.0 ** -126) * 2.0 ** (shift + 1) / ks
            dqs = dqs + u16(dt) ** 2 * (np.abs(qs) + dqs) + floor + 64 * U32 * (np.abs(qs) + dqs)
            o, e, smax, _ = softmax_expect(qs, dqs, k, v, (cap + 3) // 4 + ns + 2)
            w = np.exp(0.125 * (k @ qs) - smax)
            pr, av = w / w.sum(), np.abs(v)
            e = e + 2 * (u16(dt) ** 2 * (pr @ av) + (2.0 ** -25 * av.sum(0) if dt == "f16" else 0.0) + (n + 1) * U32 * (pr @ av))
            # (the extremes' tiny V channel has subnormal bfloat16 outputs: the output pair rounds those to multiples of 2^-133)
            pe.put(frag_index(s, h * 64 + np.arange(64), p["nbs"]), o, e + pair_err(np.abs(o) + e, dt) + (2.0 ** -134 if extreme and dt == "bf16" else 0.0))
    return pe


def test_group_fp8_kernel_against_float64(driver, tmp_path, monkeypatch):
    """The h16 grouped kernel's test body (sentinel outside the ranges, tickets at zero, cut twins bit for bit) over this file's parts."""
    for name, mine in (("CASES", CASES), ("inputs", inputs), ("expect", expect)):
        monkeypatch.setattr(G, name, mine)
    G.test_group_kernel_against_float64(driver, tmp_path)
