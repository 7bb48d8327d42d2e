"""The checker of tests/encoder_kernel_reference.py checked without a GPU: a float32 numpy emulation of each encoder kernel's
arithmetic (fp32 accumulation, narrowing to the 16-bit type at the kernel's points through torch casts, the online softmax with
the threshold rule of csrc/encoder_attn.hip) must PASS the checker on every input family the GPU tests use — the proof that the
inputs and the derived bounds leave a correct kernel inside — and seeded wrong variants of the emulation must each FAIL it.
The emulation places its outputs with code of its own (reshapes and an explicit frame order), not with the reference's index
formulas, so a wrong layout formula in the reference fails here too.

Worst error / bound of the faithful emulations (printed with -s): GEMM epilogues 0.996 and LayerNorm 0.999 (a 16-bit output
is at most half an ulp off, and some are), attention 0.449."""
import numpy as np
import pytest
import torch

import encoder_kernel_reference as ekr
from encoder_kernel_reference import EPI_BIAS, EPI_CROSS_KV, EPI_GELU, EPI_GELU_POS, EPI_PARTIAL, EPI_QKV, EPI_RESID

F = np.float32
DTYPES = ("bf16", "f16")
FAMILIES = ("uniform", "realistic")
FRAME_ORDER = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]  # stored position -> frame of the 16-group


def f32(bits, dt):
    return ekr.from_bits(bits, dt).astype(F)


def gelu_fast2(x):
    """gelu_erf_fast2 of csrc/common.hpp in float32."""
    ax = np.abs(x)
    t = F(1) / (ax * F(0.3275911 * 0.70710678118654752440) + F(1))
    poly = t * F(0.5 * 1.061405429) + F(0.5 * -1.453152027)
    poly = poly * t + F(0.5 * 1.421413741)
    poly = poly * t + F(0.5 * -0.284496736)
    poly = poly * t + F(0.5 * 0.254829592)
    poly = poly * t
    u = ax * F(0.84932180028801904272)
    e = F(0.5) - poly * np.exp2(-u * u)
    return (ax * e + x * F(0.5)).astype(F)


def gelu_erff(x):
    return (F(0.5) * x * (F(1) + torch.erf(torch.from_numpy(x * F(0.70710678118654752440))).numpy())).astype(F)


def gelu_tanh(x):
    return (F(0.5) * x * (F(1) + np.tanh(F(0.7978845608) * (x + F(0.044715) * x * x * x)))).astype(F)


def emulate_gemm(p, bufs, dt, wrong=None):
    """The launch in float32; returns {buffer: content after it}. wrong: None or the name of a seeded defect."""
    epi, M, N, K, B, d = p["epi"], p["M"], p["N"], p["K"], p["batch"], p["d"]
    A = f32(bufs[p["A"]], dt)
    W = f32(bufs[p["W"]], dt).reshape(N, K)
    bias = bufs[p["bias"]].astype(F)
    out = {k: np.array(bufs[p[k]]) for k in ("C", "C2", "C3", "part") if p.get(k)}
    r16 = lambda x: ekr.to_bits(x, dt)
    for b in range(B):
        a = ekr.gather_rows(A, p.get("A_off", 0) + b * p["a_bs"], p["lda"], M, K)
        if wrong == "neighbour_row" and b + 1 < B:  # the last row of a clip taken from the first of the next one
            a = np.array(a)
            a[M - 1] = ekr.gather_rows(A, p.get("A_off", 0) + (b + 1) * p["a_bs"], p["lda"], 1, K)[0]
        if epi == EPI_PARTIAL:
            ks = p["ksplit"]
            slab = out["part"].view(F)
            for q in range(ks):
                sl = slice(q * K // ks, (q + 1) * K // ks)
                o = q * p["part_stride"] + b * M * N
                slab[o:o + M * N] = (a[:, sl] @ W[:, sl].T).ravel()
            continue
        acc = (a @ W.T).astype(F) + bias
        if wrong == "bias_twice":
            acc = acc + bias
        if epi in (EPI_BIAS, EPI_GELU, EPI_GELU_POS, EPI_RESID):
            C = out["C"].view(F) if epi in (EPI_GELU_POS, EPI_RESID) else out["C"]
            rows = C[p.get("C_off", 0) + b * p["c_bs"]:][:M * p["ldc"]].reshape(M, p["ldc"])[:, :N]
            if epi == EPI_BIAS:
                rows[:] = r16(acc)
            elif epi == EPI_GELU:
                rows[:] = r16(gelu_tanh(acc) if wrong == "gelu_tanh" else gelu_fast2(acc))
            elif epi == EPI_GELU_POS:
                rows[:] = (gelu_tanh(acc) if wrong == "gelu_tanh" else gelu_erff(acc)) + bufs[p["aux"]].reshape(M, N)
            else:
                rows[:] = acc if wrong == "resid_store" else acc + rows
        elif epi == EPI_QKV:
            tp = p["t_pad"]
            if p["qkv_part"] != 2:
                out["C"][b * p["c_bs"]:][:M * d].reshape(M, d)[:] = r16(acc[:, :d])
                out["C2"][b * p["c2_bs"]:][:M * d].reshape(M, d)[:] = r16(acc[:, d:2 * d])
            if p["qkv_part"] != 1:
                vt = out["C3"][b * p["c3_bs"]:][:d * tp].reshape(d, tp // 16, 16)
                nat = vt.copy()  # natural frame order; frames >= M keep what was there
                if wrong != "vt_natural":
                    nat = np.ascontiguousarray(nat[:, :, np.argsort(FRAME_ORDER)])  # stored -> natural
                nat.reshape(d, tp)[:, :M] = r16(acc[:, 2 * d:]).T
                vt[:] = nat if wrong == "vt_natural" else nat[:, :, FRAME_ORDER]
        elif epi == EPI_CROSS_KV:
            L, tp, nbt, H = p["n_layer"], p["t_pad"], p["nbt"], d // 64
            slot = int(bufs[p["slot_map"]][b])
            ck = out["C"].reshape(L, nbt, H, tp // 64, 8, 64, 8)   # [l][slot][head][m/64][dd/8][m%64][dd%8]
            cv = out["C2"].reshape(L, nbt, H, tp, 64)               # [l][slot][head][m][dd]
            k16 = r16(acc[:, :L * d]).reshape(M, L, H, 8, 8)        # [m][l][head][dd/8][dd%8]
            v16 = r16(acc[:, L * d:]).reshape(M, L, H, 64)
            for m in range(M):
                ck[:, slot, :, m // 64, :, m % 64, :] = k16[m]
            cv[:, slot, :, :M, :] = v16.transpose(1, 2, 0, 3)
    return {p[k]: v for k, v in out.items()}


def check_gemm(p, bufs, dt, wrong=None):
    exp = ekr.gemm_expect(p, bufs, dt)
    got = emulate_gemm(p, bufs, dt, wrong)
    assert set(got) == set(exp)
    return max(ekr.check(f"{p['kind']}.{name}", got[name], exp[name], dt, guard=False) for name in exp)


SMALL = dict(T=100, n_layer=2)
KINDS = [(k, 0) for k in ekr.GEMM_KINDS if not k.endswith("part")] + [("oproj_part", 2), ("ffn2_part", 2), ("ffn2_part", 4)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_faithful_gemm_emulation_passes(dt, family):
    worst = 0.0
    for i, (kind, ks) in enumerate(KINDS):
        for clips in (1, 2):
            p, bufs = ekr.gemm_case(kind, 128, clips, dt, family, 100 + i, ksplit=ks, **SMALL)
            w = check_gemm(p, bufs, dt)
            print(f"{dt} {family} {kind} clips {clips}: worst error / bound {w:.3f}")
            worst = max(worst, w)
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wrong, kind", [("resid_store", "oproj_resid"), ("resid_store", "ffn2_resid"), ("bias_twice", "qkv"),
                                         ("bias_twice", "ffn1"), ("bias_twice", "cross"), ("bias_twice", "ffn2_resid"),
                                         ("neighbour_row", "conv2"), ("neighbour_row", "qkv"), ("neighbour_row", "oproj_part"),
                                         ("neighbour_row", "cross"), ("gelu_tanh", "conv1"), ("gelu_tanh", "conv2"),
                                         ("gelu_tanh", "ffn1"), ("vt_natural", "qkv"), ("vt_natural", "v")])
def test_wrong_gemm_variant_fails(dt, wrong, kind):
    p, bufs = ekr.gemm_case(kind, 128, 2, dt, "uniform", 7, ksplit=2, **SMALL)
    check_gemm(p, bufs, dt)
    with pytest.raises(AssertionError):
        check_gemm(p, bufs, dt, wrong)


def test_stray_store_and_guard_are_noticed():
    p, bufs = ekr.gemm_case("conv1", 128, 2, "bf16", "uniform", 3, **SMALL)
    exp = ekr.gemm_expect(p, bufs, "bf16")["h1"]
    got = emulate_gemm(p, bufs, "bf16")["h1"]
    ekr.check("h1", got, exp, "bf16", guard=False)
    for el in (0, 127, 201 * 128, got.size - 1):  # h1 row 0, the trailing row of clip 0, the very last element
        bad = got.copy()
        bad[el] = 0
        with pytest.raises(AssertionError, match="outside the valid output"):
            ekr.check("h1", bad, exp, "bf16", guard=False)
    g = ekr.sentinel(ekr.GUARD, 1)
    ekr.check("h1", np.concatenate([g, got, g]), exp, "bf16")
    for where in (ekr.GUARD // 2 - 1, -1):
        dump = np.concatenate([g, got, g])
        dump[where] = 0
        with pytest.raises(AssertionError, match="guard"):
            ekr.check("h1", dump, exp, "bf16")


# ------------------------------------------------------------------------------------------ LayerNorm
def emulate_layernorm(x, g, b, dt, part=None, part_bias=None, skip_slice=None):
    x = x.astype(F).copy()
    if part is not None:
        x += part_bias
        for q in range(part.shape[0]):
            if q != skip_slice:
                x += part[q]
    d = x.shape[1]
    mean = (x.sum(1, dtype=F) / F(d))[:, None]
    a = x - mean
    r = (F(1) / np.sqrt((a * a).sum(1, dtype=F) / F(d) + F(1e-5)))[:, None]
    return x, ekr.to_bits(a * r * g + b, dt)


def layernorm_rows(rng, rows, d, family):
    x = rng.standard_normal((rows, d)).astype(F)
    if family == "outlier":
        ch = rng.choice(d, 3, replace=False)
        x[:, ch] += rng.uniform(150, 500, 3).astype(F) * rng.choice([-1, 1], 3).astype(F)
    elif family == "constant":
        x[:] = rng.choice([0.0, 0.5, -3.0, 1.7], (rows, 1)).astype(F)
    return x


@pytest.mark.parametrize("dt", DTYPES)
def test_faithful_layernorm_emulation_passes_and_a_skipped_slice_fails(dt):
    rng = np.random.default_rng(5)
    worst = 0.0
    for d in (128, 384):
        for family in ("normal", "outlier", "constant"):
            for n_part in (0, 2, 3, 4):
                x = layernorm_rows(rng, 37, d, family)
                g, b = rng.uniform(0.5, 1.5, d).astype(F), rng.uniform(-1, 1, d).astype(F)
                part = rng.standard_normal((n_part, 37, d)).astype(F) if n_part else None
                pb = rng.uniform(-1, 1, d).astype(F) if n_part else None
                xr, xb, yr, yb = ekr.layernorm_expect(x, g, b, dt, part, pb)
                xe, ye = emulate_layernorm(x, g, b, dt, part, pb)
                w = ekr.check_values("y", ekr.from_bits(ye, dt), yr, yb)
                if n_part:
                    w = max(w, ekr.check_values("x", xe, xr, xb))
                    if family != "constant":
                        xw, yw = emulate_layernorm(x, g, b, dt, part, pb, skip_slice=n_part - 1)
                        with pytest.raises(AssertionError):
                            ekr.check_values("x", xw, xr, xb)
                        with pytest.raises(AssertionError):
                            ekr.check_values("y", ekr.from_bits(yw, dt), yr, yb)
                print(f"{dt} layernorm d {d} {family} n_part {n_part}: worst error / bound {w:.3f}")
                worst = max(worst, w)
    assert 0.0 < worst <= 1.0


# ------------------------------------------------------------------------------------------ attention
def emulate_attention(q, k, vt_stored, T, t_pad, dt, thr, wrong=None):
    """One (clip, head): q, k float32 [T][64], vt_stored float32 [64][t_pad] in the stored frame order. 32 query rows (one
    wave) share the rescale decision, as the ballot of encoder_attn.hip:141 makes them."""
    sc = F(0.125) * F(1.44269504088896340736)
    if wrong == "scale":
        sc = sc * F(1 + 2.0 ** -10)
    vt = vt_stored.reshape(64, t_pad // 16, 16)
    v = (vt if wrong == "vt_natural" else vt[:, :, np.argsort(FRAME_ORDER)]).reshape(64, t_pad).T  # [key][64]
    kp = np.zeros((t_pad, 64), F)
    kp[:T] = k  # keys >= T read as zeros (the buffer resource ends behind row T - 1)
    o_all = np.zeros((T, 64), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for w0 in range(0, T, 32):
            qw = q[w0:w0 + 32]
            n = qw.shape[0]
            m_run, l_run, oacc = np.full(n, -np.inf, F), np.zeros(n, F), np.zeros((n, 64), F)
            for kt in range(t_pad // 64):
                s = (qw @ kp[kt * 64:kt * 64 + 64].T).astype(F)
                if kt == t_pad // 64 - 1 and wrong != "no_tail_mask":
                    s[:, np.arange(kt * 64, kt * 64 + 64) >= T] = -np.inf
                mt = s.max(1)
                if ((mt - m_run) * sc > F(thr)).any():
                    m_new = np.maximum(m_run, mt)
                    alpha = np.exp2((m_run - m_new) * sc).astype(F)
                    m_run = m_new
                    if wrong != "no_alpha":
                        l_run *= alpha
                        oacc *= alpha[:, None]
                pv = np.exp2(s * sc - (m_run * sc)[:, None]).astype(F)
                l_run += pv.sum(1, dtype=F)
                oacc += ekr.round16(pv, dt) @ v[kt * 64:kt * 64 + 64]
            o_all[w0:w0 + n] = oacc * (F(1) / l_run)[:, None]
    return ekr.round16(o_all, dt)


def store_vt(v, t_pad, fill):
    """v [T][64] -> V^T [64][t_pad] in the stored frame order, frames >= T = fill."""
    nat = np.full((64, t_pad), fill, F)
    nat[:, :v.shape[0]] = v.T
    return nat.reshape(64, t_pad // 16, 16)[:, :, FRAME_ORDER].reshape(64, t_pad)


ATTN_T = (4, 64, 128, 132, 200)
THRS = (0.0, 0.5, 8.0, 16.0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", ekr.ATTN_FAMILIES)
def test_faithful_attention_emulation_passes(dt, family):
    rng = np.random.default_rng(11)
    worst = 0.0
    for T in ATTN_T:
        t_pad = (T + 63) // 64 * 64
        q, k, v = ekr.attention_inputs(rng, T, dt, family)
        ref, bound = ekr.attention_expect(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), dt, t_pad)
        for thr in THRS:
            o = emulate_attention(q, k, store_vt(v, t_pad, 0.0), T, t_pad, dt, thr)
            worst = max(worst, ekr.check_values(f"{family} T {T} thr {thr}", o, ref, bound))
            o2 = emulate_attention(q, k, store_vt(v, t_pad, 3.0), T, t_pad, dt, thr)
            assert np.array_equal(o, o2), "finite garbage in the padded frames changed the result"
    print(f"{dt} attention {family}: worst error / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0


def test_wrong_softmax_scale_fails():
    """Scale off by one part in 2^10. The softmax is invariant under a shift of the scores, so the defect moves weight only
    between keys whose scores DIFFER: two groups with weights a, 1 - a a gap of g nats apart move by a (1 - a) g 2^-10. One
    key against the N others at equal weight has g = ln N: 0.25 ln(199) 2^-10 = 1.3e-3 of |v| here. That is above the half
    build's bound (2 * 2^-11 PV) and, for any N up to the 1500 keys of a clip, BELOW the bfloat16 build's (2 * 2^-8 PV: its
    probabilities carry 2^-9 each): in bfloat16 this defect is inside the kernel's own rounding and no bound derived from the
    arithmetic can see it, so the variant is run in half only."""
    dt, T, t_pad = "f16", 200, 256
    rng = np.random.default_rng(17)
    q, k, v = ekr.attention_inputs(rng, T, dt, "flat")
    q[:, 1:] *= 0.25
    q[:, 0], k[:, 0] = 8.0, 0.0
    k[0, 0] = ekr.round16([np.log(T - 1.0)], dt)[0]
    v[0] = 3.0 * np.sign(v[0])
    ref, bound = ekr.attention_expect(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), dt, t_pad)
    vt = store_vt(v, t_pad, 0.0)
    for thr in THRS:
        ekr.check_values("faithful", emulate_attention(q, k, vt, T, t_pad, dt, thr), ref, bound)
        with pytest.raises(AssertionError):
            ekr.check_values("scale", emulate_attention(q, k, vt, T, t_pad, dt, thr, "scale"), ref, bound)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wrong, family, T, thr", [("no_alpha", "rise6", 200, 0.0), ("no_alpha", "rise10", 200, 8.0),
                                                   ("no_alpha", "rise10", 200, 16.0), ("no_tail_mask", "flat", 132, 8.0),
                                                   ("no_tail_mask", "flat", 4, 0.0), ("vt_natural", "flat", 200, 8.0),
                                                   ("vt_natural", "domtail", 200, 8.0), ("vt_natural", "dom0", 132, 0.5)])
def test_wrong_attention_variant_fails(dt, wrong, family, T, thr):
    rng = np.random.default_rng(13)
    t_pad = (T + 63) // 64 * 64
    q, k, v = ekr.attention_inputs(rng, T, dt, family)
    if wrong == "vt_natural" and family.startswith("dom"):  # the dominant key where the two frame orders differ
        j = T - 1 if family == "dom0" else (T - 1) // 64 * 64 + 4
        k[:, 0] = 0
        k[j if family != "dom0" else 5, 0] = 40
    ref, bound = ekr.attention_expect(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), dt, t_pad)
    vt = store_vt(v, t_pad, 0.0)
    ekr.check_values("faithful", emulate_attention(q, k, vt, T, t_pad, dt, thr), ref, bound)
    with pytest.raises(AssertionError):
        ekr.check_values(wrong, emulate_attention(q, k, vt, T, t_pad, dt, thr, wrong), ref, bound)


def test_half_probability_overflows_at_threshold_16():
    """A probability may reach 2^thr before it is narrowed: a row maximum that rises by exactly 16 log2 units is not rescaled
    at thr = 16 and 2^16 is beyond IEEE half (65504) -> inf -> NaN in that row, which the checker reports; at 15 (where the
    engine stops the half build's AX_WHISPER_ENC_RESCALE_THR) and in bfloat16 at 16 the same input is inside the bound."""
    sc = F(0.125) * F(1.44269504088896340736)
    rng = np.random.default_rng(19)
    T, t_pad = 128, 128
    q, k, v = ekr.attention_inputs(rng, T, "f16", "flat")
    q[:], k[:] = 0, 0
    q[:, 0], q[:, 1] = 8.0, 1.0
    cand = ekr.round16(np.arange(0.70, 0.74, 2.0 ** -12), "f16")  # fine-tunes 8 * 11 + b into the last 3e-4 below 16 / sc
    diff = (F(88.0) + cand) * sc
    b = cand[(diff <= F(16)) & (diff > F(15.9997))]
    assert b.size, "no half value lands in the window"
    k[64, 0], k[64, 1] = 11.0, b[-1]  # tile 0: every score 0; tile 1: one key exactly at the threshold above them
    ref, bound = ekr.attention_expect(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), "f16", t_pad)
    vt = store_vt(v, t_pad, 0.0)
    ekr.check_values("thr 15", emulate_attention(q, k, vt, T, t_pad, "f16", 15.0), ref, bound)
    with pytest.raises(AssertionError):
        ekr.check_values("thr 16", emulate_attention(q, k, vt, T, t_pad, "f16", 16.0), ref, bound)
    refb, boundb = ekr.attention_expect(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), "bf16", t_pad)
    ekr.check_values("bf16 thr 16", emulate_attention(q, k, vt, T, t_pad, "bf16", 16.0), refb, boundb)
