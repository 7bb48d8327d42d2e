"""No GPU: the bounds of tests/decode_kernel_reference.py hold for a faithful float32 emulation of every batched decode-step
kernel, and do not hold for sixteen seeded defects — at the shapes tests/test_gpu_decode_kernels.py runs, through the very check
(`verify`) it applies to the GPU's dumps.

The emulations follow the kernels' arithmetic in numpy float32: the one-pass LayerNorm statistics in the lanes' and waves' order,
the pair split, k-steps dealt round-robin over eight waves with hi and lo accumulated one after the other and the waves added in
order behind the bias, erf GELU, 16-bit stores; the two-pass statistics of act_prep behind its fixed-order partial fold; the
online softmax per wave over every fourth 64-key block, the waves' merge, the splits' fold in split order, exp in float32.

Defect 9 (softmax scale 0.125 + 2^-10, 0.8 % of every score) is visible in BOTH builds: the attention output leaves as an (hi, lo)
pair or as fp32 partials, never as one 16-bit value, so 16 (bfloat16) or 22 (half) bits of it are checked. Defect 11 is modelled
as an empty split recording (m, l) = (0, 1) — one phantom key of weight 1 — because a record of (-inf, 0, 0) adds nothing whatever
weight the fold gives it. Defects 1 and 2 drop terms of relative size u16 with random signs, sqrt(K) u16 |w||a| in all, against an
any-order accumulation bound of 2 K u K |w||a| (4 K u on the fold rows): their ratio is 2^15 / K^1.5 in bfloat16 and 2^11 / K^1.5 in
half. So defect 1 is visible in bfloat16 at every K here and in half at K = 128 only (1.4; 0.1 at K = 768), and defect 2 (K = 384,
768) in bfloat16 only — in half M_hi alone carries 11 bits and what M_lo adds lies below what any fp32 summation order may lose.
Defect 4 (tanh GELU, up to 5e-4 from erf) needs the pair input at K = 128 for the same reason. Defect 1 is asserted on stored-pair inputs; behind the LayerNorm prologue the any-order bound of the
statistics (K u on the mean, (3 K + 4) kappa u on the variance) is as large as the lo half in bfloat16 at these K.

The GEMV family, advance and embed (tests/gemv_kernel_reference.py, tests/test_gpu_gemv_kernels.py) follow further down: float32
emulations pass every case of the GPU file when substituted for the driver process, and eighteen seeded defects (and a nineteenth,
advance's tie going to the higher index) fail at the cases and for the reasons GEMV_DEFECTS names. The first of them, `shift_x0`,
is the arithmetic both LayerNorm prologues of decode_gemv.hip had: a one-pass variance about x[b][0]. It stays inside the two-pass
bound on every family whose outlier sits elsewhere and leaves it on `outlier0`, on about three rows in ten."""
import os
import subprocess

import numpy as np
import pytest
import torch

import decode_kernel_reference as R
import encoder_kernel_reference as E
import gemv_kernel_reference as G
import kernel_driver
import test_gpu_gemv_kernels as T
from encoder_kernel_reference import GUARD, from_bits, round16, sentinel, to_bits

F = np.float32
DTYPES = ("bf16", "f16")


def guarded(a):
    g = sentinel(GUARD // 2, 2)
    return np.concatenate([g, np.ascontiguousarray(a).ravel().view(np.uint16), g])


def exp32(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp(x.astype(F) if isinstance(x, np.ndarray) else F(x)).astype(F)


# ------------------------------------------------------------------------------------------ emulations
def emu_ln_onepass(x, g, b, eps=True):
    """decode_cgemm_kernel's prologue: x fp32 [B][K]; lane (r, q) of wave w sums its 8 values of the k-steps w, w + 8, ...; the four
    q lanes pair up as (0 + 1) + (2 + 3); the eight waves are added in order."""
    B, K = x.shape
    KS = K // 32
    v = x.reshape(B, KS, 4, 2, 4)
    s1w, s2w = np.zeros((8, B, 4), F), np.zeros((8, B, 4), F)
    for ks in range(KS):
        for u in range(2):
            t = v[:, ks, :, u]
            s1w[ks % 8] += (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
            s2w[ks % 8] += (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + (t[..., 2] * t[..., 2] + t[..., 3] * t[..., 3])
    lanes = lambda s: (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    s1, s2 = np.zeros(B, F), np.zeros(B, F)
    for w in range(8):
        s1 += lanes(s1w[w]); s2 += lanes(s2w[w])
    mean = (s1 / F(K))[:, None]
    var = np.maximum(s2[:, None] / F(K) - mean * mean, F(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (F(1) / np.sqrt(var + (F(1e-5) if eps else F(0)))).astype(F)
        return ((x - mean) * rstd * g + b).astype(F)


def emu_mma(W, hi, lo, bias, Wl=None, drop_lo=False, drop_wl=False):
    """y[b][n]: eight waves take the k-steps round-robin, hi then lo per k-step (fp32), then bias + the waves in order."""
    K = W.shape[1]
    acc = np.zeros((8, hi.shape[0], W.shape[0]), F)
    for ks in range(K // 32):
        sl = slice(ks * 32, ks * 32 + 32)
        a = acc[ks % 8]
        a += hi[:, sl] @ W[:, sl].T
        if not drop_lo:
            a += lo[:, sl] @ W[:, sl].T
        if Wl is not None and not drop_wl:
            a += hi[:, sl] @ Wl[:, sl].T
            a += lo[:, sl] @ Wl[:, sl].T
    y = np.broadcast_to(bias.astype(F), acc[0].shape).copy()
    for w in range(8):
        y += acc[w]
    return y


def gelu32(y, tanh=False):
    t = torch.from_numpy(y)
    if tanh:
        return (0.5 * t * (1 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))).numpy()
    return (F(0.5) * y * (F(1) + torch.erf(t * F(0.70710678118654752440)).numpy())).astype(F)


def put_pair(state, hn, ln_, idx, y, dt):
    hb, lb = R.pair_bits(y, dt)
    h, l = state[hn].copy(), state[ln_].copy()
    h[idx], l[idx] = hb, lb
    return {hn: guarded(h), ln_: guarded(l)}


def emu_gemm(p, state, dt, defect=None):
    st = R.typed(p, state)
    N, K, B, nbs, epi = p["N"], p["K"], p["batch"], p["nbs"], p["epilogue"]
    fr0 = p.get("fold_row0", 0)
    W = from_bits(R.unpack_weight(st[p["W"]], N, K), dt).astype(F)
    bias = st[p["bias"]].astype(F) if p.get("bias") else np.zeros(N, F)
    drop_lo = defect == "drop_lo"
    hi2 = lo2 = None
    if p.get("ln_w"):
        x = st[p["x"]][:B * K].reshape(B, K)
        hi, lo = R.pair_split(emu_ln_onepass(x, st[p["ln_w"]], st[p["ln_b"]], eps=defect != "no_eps"), dt)
        if p.get("ln_w2"):
            hi2, lo2 = R.pair_split(x * st[p["ln_w2"]], dt)
    else:
        idx = R.frag_index(np.arange(B)[:, None], np.arange(K)[None, :], nbs)
        hi, lo = from_bits(st[p["a_hi"]][idx], dt).astype(F), from_bits(st[p["a_lo"]][idx], dt).astype(F)
    bi, ni = np.arange(B)[:, None], np.arange(N)[None, :]
    got = {}
    if epi == R.GEPI_PARTIAL:
        ks, pb = p["ksplit"], p["part_batch"]
        out = st[p["out"]].copy()
        for s in range(ks):
            sl = slice(s * K // ks, (s + 1) * K // ks)
            out[((s * pb + bi) * N + ni).ravel()] = emu_mma(W[:, sl], hi[:, sl], lo[:, sl], np.zeros(N, F), drop_lo=drop_lo).ravel()
        return {p["out"]: guarded(out)}
    nx = fr0 if fr0 else N
    y = emu_mma(W[:nx], hi, lo, bias[:nx], drop_lo=drop_lo)
    y2 = None
    if fr0 and hi2 is not None:
        y2 = emu_mma(W[fr0:], hi2, lo2, bias[fr0:], drop_lo=drop_lo)
    elif fr0:
        Wl = from_bits(R.unpack_weight(st[p["W_lo"]], N - fr0, K), dt).astype(F)
        y2 = emu_mma(W[fr0:], hi, lo, bias[fr0:], Wl=Wl, drop_lo=drop_lo, drop_wl=defect == "drop_mlo")
    if epi == R.GEPI_STORE:
        out = st[p["out"]].copy()
        out[:B * N] = y.ravel()
        got[p["out"]] = guarded(out)
    elif epi == R.GEPI_RESID:
        out = st[p["out"]].copy()
        xn = y if defect == "resid_store" else out[:B * nx].reshape(B, nx) + y
        out[:B * nx] = xn.ravel()
        got[p["out"]] = guarded(out)
        if fr0:
            o2 = st[p["out2"]].copy()
            o2[:B * (N - fr0)] = (o2[:B * (N - fr0)].reshape(B, -1) + y2).ravel()
            got[p["out2"]] = guarded(o2)
        if p.get("stat_part"):
            xb = xn.reshape(B, nx // 16, 16)
            s1 = xb.sum(2, dtype=F)
            dm = xb - (s1 * F(1 / 16))[..., None]
            sp = st[p["stat_part"]].copy()
            sp[:B * (nx // 16) * 2] = np.stack([s1, (dm * dm).sum(2, dtype=F)], 2).ravel()
            got[p["stat_part"]] = guarded(sp)
    elif epi == R.GEPI_GELU:
        got.update(put_pair(st, p["out_hi"], p["out_lo"], R.frag_index(bi, ni, nbs), gelu32(y, tanh=defect == "gelu_tanh"), dt))
    elif epi == R.GEPI_QKV_CACHE:
        d, bs, Tc = p["d_model"], p["kv_batch_stride"], p["n_ctx_pad"]
        out = st[p["out"]].copy()
        out[:B * d] = y[:, :d].ravel()
        got[p["out"]] = guarded(out)
        off = st[p["off"]][:B].astype(np.int64)[:, None]
        if defect == "cache_clip0":
            off = np.full_like(off, off[0, 0])
        if defect == "cache_plus1":
            off = off + 1
        c = np.arange(d)[None, :]
        base = bi * bs + (c >> 6) * Tc * 64
        kc, vc = st[p["k_cache"]].copy(), st[p["v_cache"]].copy()
        kc[(base + R.kcache_index(off, c & 63, "swap" if defect == "cache_swap" else None)) % kc.size] = to_bits(y[:, d:2 * d], dt)  # (a kernel would leave the buffer)
        vc[base + R.vcache_index(off, c & 63)] = to_bits(y[:, 2 * d:3 * d], dt)
        got.update({p["k_cache"]: guarded(kc), p["v_cache"]: guarded(vc)})
        if fr0:
            o2 = st[p["out2"]].copy()
            o2[:B * d] = y2.ravel()
            got[p["out2"]] = guarded(o2)
    elif epi == R.GEPI_LOGITS:
        grid, stv = R.dgemm_grid(N, p["rt"]), p["amax_stride"]
        av, ai = st[p["amax_val"]].copy(), st[p["amax_idx"]].copy()
        dump = st[p["logits_dump"]].copy() if p.get("logits_dump") else None
        if (st[p["off"]][:B] >= p["skip_before_step"]).any():
            seen = np.ones(N, dtype=bool)
            if defect == "skip_block" and p["rt"] == 0:  # the third body of the last trip of the 3 G loop is left out
                n_rb = (N + 15) // 16
                for w in range(grid):
                    mine = np.arange(w, n_rb, grid)
                    if mine.size % 3 == 0:
                        seen[mine[-1] * 16:mine[-1] * 16 + 16] = False
            ym = np.where(seen[None, :], y, -np.inf).astype(F)
            v, i = R.argmax_expect(ym, N, p["rt"], grid, last=defect == "argmax_last")
            for c in range(B):
                av[c * stv:c * stv + grid], ai[c * stv:c * stv + grid] = v[c], i[c]
                if dump is not None:
                    row = dump[c * p["logits_dump_stride"]:c * p["logits_dump_stride"] + N]
                    row[seen] = y[c, seen]
        got.update({p["amax_val"]: guarded(av), p["amax_idx"]: guarded(ai)})
        if dump is not None:
            got[p["logits_dump"]] = guarded(dump)
    return got


def emu_actprep(p, state, dt, defect=None):
    st = R.typed(p, state)
    B, K, nbs, n_part, pb = p["batch"], p["K"], p["nbs"], p["n_part"], p.get("part_batch", 0)
    x = st[p["x"]].copy()
    v = x[:B * K].reshape(B, K).copy()
    if n_part:
        v += st[p["part_bias"]]
        for s in range(n_part - (1 if defect == "slice_left_out" else 0)):
            v += st[p["part"]][s * pb * K:(s * pb + B) * K].reshape(B, K)
        x[:B * K] = v.ravel()
    if p["do_ln"]:
        mean = (v.sum(1, dtype=F) / F(K))[:, None]
        t = v - mean
        rstd = F(1) / np.sqrt((t * t).sum(1, dtype=F)[:, None] / F(K) + F(1e-5))
        v = (t * rstd * st[p["g"]] + st[p["be"]]).astype(F)
    got = put_pair(st, p["hi"], p["lo"], R.frag_index(np.arange(B)[:, None], np.arange(K)[None, :], nbs), v, dt)
    got[p["x"]] = guarded(x)
    return got


def emu_query(p, st, dt, defect):
    B, d = p["batch"], p["d_model"]
    if p.get("tq"):
        tq = st[p["tq"]][:B * d].reshape(B, d)
        sp = st[p["stat_part"]][:B * (d // 16) * 2].reshape(B, d // 16, 2)
        mean = (sp[..., 0].sum(1, dtype=F) / F(d))[:, None]
        dm = sp[..., 0] * F(1 / 16) - mean
        t = sp[..., 1] + (F(0) if defect == "fold_no_between" else F(16) * dm * dm)
        rstd = F(1) / np.sqrt(t.sum(1, dtype=F)[:, None] / F(d) + F(1e-5))
        return (rstd * (tq - mean * st[p["fold_s"]]) + st[p["fold_c"]]).astype(F)
    if p.get("wq"):
        x = st[p["x"]][:B * d].reshape(B, d)
        s1, s2 = x.sum(1, dtype=F), (x * x).sum(1, dtype=F)  # one pass, as the kernel (its order: 256 threads x 4, then the waves)
        mean = (s1 / F(d))[:, None]
        var = np.maximum(s2[:, None] / F(d) - mean * mean, F(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            y = ((x - mean) * (F(1) / np.sqrt(var + (F(1e-5) if defect != "no_eps" else F(0)))) * st[p["ln_w"]] + st[p["ln_b"]]).astype(F)
        return (y @ from_bits(st[p["wq"]], dt).astype(F).reshape(d, d).T + st[p["bq"]]).astype(F)
    return st[p["q"]][:B * d].reshape(B, d)


def emu_split(q, k, v, n_keys, blk0, blk1, defect):
    """One workgroup: blocks [blk0, blk1) dealt over four waves; returns (m, l, o[64]) of the split."""
    scale = F(0.125) + (F(2.0 ** -10) if defect == "scale" else F(0))
    recs = []
    for w in range(4):
        m_w, l, o = F(-np.inf), np.zeros(64, F), np.zeros(64, F)
        for blk in range(blk0 + w, min(blk1, (n_keys + 63) // 64), 4):
            kk, vv = k[blk * 64:blk * 64 + 64], v[blk * 64:blk * 64 + 64]
            sc = (kk @ q).astype(F) * scale
            key = blk * 64 + np.arange(64)
            sc[(key > n_keys) if defect == "mask_gt" else (key >= n_keys)] = -np.inf
            m_new = max(m_w, sc.max())
            alpha, pk = exp32(m_w - m_new), exp32(sc - m_new)
            l = l * alpha + pk
            o = o * alpha + (pk @ vv).astype(F)
            m_w = m_new
        recs.append((m_w, l.sum(dtype=F), o))
    m = max(r[0] for r in recs)
    L, O = F(0), np.zeros(64, F)
    if m > -np.inf:
        for mw, lw, ow in recs:
            f = exp32(mw - m)
            L, O = L + f * lw, O + f * ow
    elif defect == "empty_weight1":
        m, L = F(0), F(1)
    return m, L, O


def emu_attn(p, state, dt, defect=None):
    st = R.typed(p, state)
    B, H, d, cap, ns = p["batch"], p["n_head"], p["d_model"], p["cap_blocks"], p.get("n_split", 1)
    q = emu_query(p, st, dt, defect)
    k = R.kv_natural(st[p["k"]], B, H, cap, p["kv_batch_stride"], dt, True).astype(F)
    v = R.kv_natural(st[p["v"]], B, H, cap, p["kv_batch_stride"], dt, False).astype(F)
    bps = (cap + ns - 1) // ns
    pair = bool(p.get("out_hi"))
    vals = np.zeros((B, d), F)
    part = None if pair else st[p["part"]].copy()
    for b in range(B):
        if st[p["done"]][b]:
            continue
        nk = p["n_keys"] if p["n_keys"] >= 0 else int(st[p["off"]][b]) + 1
        for h in range(H):
            recs = [emu_split(q[b, h * 64:h * 64 + 64], k[b, h], v[b, h], nk, s * bps, min(cap, (s + 1) * bps), defect) for s in range(ns)]
            if not pair:
                for s, (m, l, o) in enumerate(recs):
                    at = ((b * H + h) * ns + s) * R.PART
                    part[at], part[at + 1], part[at + 2:at + R.PART] = m, l, o
                continue
            M, Ls, O = F(-np.inf), F(0), np.zeros(64, F)
            for m2, l2, o2 in recs:
                mn = max(M, m2)
                if defect == "no_rescale":
                    f1, f2 = F(M > -np.inf), F(m2 > -np.inf)
                else:
                    f1, f2 = (exp32(M - mn) if M > -np.inf else F(0)), (exp32(m2 - mn) if m2 > -np.inf else F(0))
                Ls, O, M = f1 * Ls + f2 * l2, f1 * O + f2 * o2, mn
            vals[b, h * 64:h * 64 + 64] = O / Ls
    if not pair:
        return {p["part"]: guarded(part)}
    act = np.nonzero(st[p["done"]][:B] == 0)[0]
    got = put_pair(st, p["out_hi"], p["out_lo"], R.frag_index(act[:, None], np.arange(d)[None, :], p["nbs"]), vals[act], dt)
    if p.get("mcnt"):
        got[p["mpart"]], got[p["mcnt"]] = guarded(st[p["mpart"]]), guarded(st[p["mcnt"]])
    return got


def emu_pack(cmd, p, state, dt):
    st = R.typed(p, state, cmd)
    w = st[p["w"]].reshape(p["N"], p["K"])
    if cmd == "packw":
        return {p["wp"]: guarded(R.pack_weight(w))}
    hi, lo = R.pair_bits(w, dt)
    return {p["hi"]: guarded(R.pack_weight(hi)), p["lo"]: guarded(R.pack_weight(lo))}


def run_emulated(dt, group, defect=None):
    bufs, launches = group
    state, prev, notes = dict(bufs), None, {}
    for cmd, ident, p, outs in launches:
        got = (emu_gemm if cmd in ("cgemm", "dgemm") else emu_actprep if cmd == "actprep" else emu_attn if cmd == "attn" else
               (lambda p_, s_, d_, x_: emu_pack(cmd, p_, s_, d_)))(p, state, dt, defect)
        assert set(got) == set(outs), (ident, sorted(got), outs)
        for k_, v_ in R.verify(cmd, ident, p, state, got, dt, prev).items():
            notes[k_] = max(notes.get(k_, 0.0), v_)
        prev = got
        for name in outs:
            state[name] = R.strip(ident, got[name])
    return notes


# ------------------------------------------------------------------------------------------ the groups (shapes of the GPU test)
OFFS8 = (0, 7, 63, 64, 65, 127, 128, 447)
GROUPS = {
    "cgemm_ln_store": lambda dt: R.linear_group(dt, 1, "cgemm", K=384, N=40, batch=17, nbs=3, epi=R.GEPI_STORE, ln=True),
    "cgemm_ln_store_1280": lambda dt: R.linear_group(dt, 2, "cgemm", K=1280, N=72, batch=15, nbs=2, epi=R.GEPI_STORE, rt=2, ln=True),
    "cgemm_pair_resid_128": lambda dt: R.linear_group(dt, 3, "cgemm", K=128, N=48, batch=16, nbs=2, epi=R.GEPI_RESID),
    "cgemm_pair_resid_768": lambda dt: R.linear_group(dt, 4, "cgemm", K=768, N=40, batch=17, nbs=3, epi=R.GEPI_RESID),
    "cgemm_pair_resid_3072": lambda dt: R.linear_group(dt, 5, "cgemm", K=3072, N=24, batch=4, nbs=1, epi=R.GEPI_RESID, family="realistic"),
    "cgemm_ln_gelu": lambda dt: R.linear_group(dt, 6, "cgemm", K=384, N=100, batch=40, nbs=4, epi=R.GEPI_GELU, rt=2, ln=True),
    "cgemm_qkv": lambda dt: R.linear_group(dt, 7, "cgemm", K=384, N=1152, batch=8, nbs=1, epi=R.GEPI_QKV_CACHE, ln=True, d_model=384, offs=OFFS8),
    "dgemm_gelu": lambda dt: R.linear_group(dt, 8, "dgemm", K=1280, N=100, batch=17, nbs=3, epi=R.GEPI_GELU, rt=4),
    "dgemm_qkv": lambda dt: R.linear_group(dt, 9, "dgemm", K=1280, N=1152, batch=8, nbs=2, epi=R.GEPI_QKV_CACHE, d_model=384, offs=OFFS8[::-1]),
    "partial_768": lambda dt: R.partial_group(dt, 10, K=768, d=384, batch=17, nbs=2),
    "partial_1280": lambda dt: R.partial_group(dt, 11, K=1280, d=384, batch=3, nbs=1),
    "logits_rt4": lambda dt: R.logits_group(dt, 12, K=1280, N=300, batch=17, nbs=2, rt=4),
    "logits_rt0_769": lambda dt: R.logits_group(dt, 13, K=128, N=769 * 16 - 5, batch=16, nbs=1, rt=0),
    "logits_rt0_768": lambda dt: R.logits_group(dt, 14, K=128, N=768 * 16 - 5, batch=17, nbs=2, rt=0),
    "logits_skip": lambda dt: R.logits_group(dt, 15, K=128, N=83, batch=16, nbs=1, rt=0, offs=np.arange(16) % 3, skip=3),
    "actprep": lambda dt: (lambda b: (b, [R.actprep_launch(np.random.default_rng(16), b, K=1280, batch=17, nbs=3, n_part=3, do_ln=True, part_batch=20)]))({}),
    "actprep_plain": lambda dt: (lambda b: (b, [R.actprep_launch(np.random.default_rng(17), b, K=384, batch=1, nbs=1, n_part=0, do_ln=False, part_batch=0)]))({}),
    "fold_384": lambda dt: R.fold_group(dt, 18, d=384, batch=4, nbs=1, n_split=6, n_keys=200),
    "fold_384_benign": lambda dt: R.fold_group(dt, 19, d=384, batch=4, nbs=1, n_split=1, n_keys=65, family="benign"),
    "attn_self_pair": lambda dt: R.attn_group(dt, 20, cap=7, offs=(0, 62, 63, 64, 127, 128, 255, 256, 447), batch=9),
    "attn_self_part2": lambda dt: R.attn_group(dt, 21, cap=7, offs=(0, 63, 64, 255), batch=4, n_split=2, out="part"),
    "attn_cross_65_s3": lambda dt: R.attn_group(dt, 22, cap=24, n_keys=65, n_split=3, relaunch=True),
    "attn_cross_1500_s6": lambda dt: R.attn_group(dt, 23, cap=24, n_keys=1500, n_split=6, relaunch=True),
    "attn_fused_384": lambda dt: R.attn_group(dt, 24, H=6, batch=5, cap=24, n_keys=64, mode="fused"),
    "attn_cross_1476_s4": lambda dt: R.attn_group(dt, 29, cap=24, n_keys=1476, n_split=4),
    "cgemm_pair_gelu_128": lambda dt: R.linear_group(dt, 30, "cgemm", K=128, N=100, batch=17, nbs=2, epi=R.GEPI_GELU),
    "attn_fused_640": lambda dt: R.attn_group(dt, 26, H=10, cap=24, n_keys=65, mode="fused", n_split=2),
    "attn_done": lambda dt: R.attn_group(dt, 27, cap=24, n_keys=65, n_split=2, done=(0, 1, 0), done_late=1),
    "pack": lambda dt: (lambda gs: (dict(gs[0][0], **{"w2": gs[1][0]["w"], "hi": gs[1][0]["hi"], "lo": gs[1][0]["lo"]}),
                                    [gs[0][1][0], R.launch("packw_split", "packw_split", N=37, K=96, w="w2", hi="hi", lo="lo")]))(R.pack_groups(dt, 28, 37, 96)),
}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_float32_emulation_stays_within_the_bounds(name, dt):
    notes = run_emulated(dt, GROUPS[name](dt))
    for what, w in sorted(notes.items()):
        print(f"{dt} {name} {what}: emulation error / bound {w:.3f}")
        assert w <= 1.0


# defect -> the groups it must fail on (each at a shape of the GPU test)
DEFECTS = {
    "drop_lo": {"bf16": ("cgemm_pair_resid_128", "cgemm_pair_resid_768", "dgemm_gelu", "partial_768", "logits_rt4"),  # 1
                "f16": ("cgemm_pair_resid_128", "cgemm_pair_gelu_128")},
    "drop_mlo": {"bf16": ("fold_384", "fold_384_benign"), "f16": ()},                                             # 2 (half: see above)
    "resid_store": ("cgemm_pair_resid_128", "cgemm_pair_resid_3072"),                                            # 3
    "gelu_tanh": ("cgemm_pair_gelu_128",),                                                                # 4
    "cache_clip0": ("cgemm_qkv", "dgemm_qkv"),                                                                   # 5
    "cache_plus1": ("cgemm_qkv", "dgemm_qkv"),                                                                   # 6
    "cache_swap": ("cgemm_qkv", "dgemm_qkv"),                                                                    # 7
    "mask_gt": ("attn_self_pair", "attn_cross_65_s3", "attn_self_part2"),                                        # 8
    "scale": ("attn_self_pair", "attn_cross_1500_s6"),                                                           # 9
    "no_rescale": ("attn_cross_1500_s6", "attn_cross_1476_s4"),                                                    # 10
    "empty_weight1": ("attn_self_part2", "attn_cross_65_s3"),                                                    # 11
    "fold_no_between": ("fold_384", "fold_384_benign"),                                                          # 12
    "no_eps": ("cgemm_ln_store", "attn_fused_384"),                                                              # 13
    "argmax_last": ("logits_rt4", "logits_rt0_769"),                                                             # 14
    "skip_block": ("logits_rt0_768",),                                                                           # 15
    "slice_left_out": ("actprep", "partial_768"),                                                                # 16
}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defect_fails(defect, dt):
    names = DEFECTS[defect]
    for name in names[dt] if isinstance(names, dict) else names:
        try:
            run_emulated(dt, GROUPS[name](dt), defect)
        except AssertionError as e:
            print(f"{dt} {defect}: caught at {name}: {str(e)[:150]}")
            continue
        pytest.fail(f"{dt}: defect {defect} passes at {name}")


# ------------------------------------------------------------------------------------------ the GEMV family, advance, embed
# Float32 emulations of gemv1_kernel / gemv_kernel (the lanes' fused multiply-add chains, the lane butterfly, the bias; two-pass
# LayerNorm; the combine's exp in float32) substituted for the driver process of tests/test_gpu_gemv_kernels.py: every case of that
# file passes, and each of eighteen seeded defects fails at the cases named in GEMV_DEFECTS. advance and embed are integer- and
# bit-exact: their "emulation" is the reference state machine itself (written once), the defects are switches in it.
def lane_sum(v, lpr):
    """Sum over the row in the kernels' order. gemv1_kernel (lpr lanes): lane j adds the chunks j + lpr i one value after the
    other, then the xor butterfly; gemv_kernel (lpr None): thread t adds t + 256 e, a butterfly per wave, the four waves in order."""
    B, K = v.shape
    if lpr:
        per = v.reshape(B, K // (8 * lpr), lpr, 8).transpose(0, 2, 1, 3).reshape(B, lpr, -1)
    else:
        pad = np.zeros((B, 2048), F)
        pad[:, :K] = v
        per = pad.reshape(B, 8, 256).transpose(0, 2, 1)
    acc = np.zeros(per.shape[:2], F)
    for e in range(per.shape[2]):
        acc = acc + per[:, :, e]
    if not lpr:
        acc = acc.reshape(B, 4, 64)
    n = acc.shape[-1]
    while n > 1:
        acc = acc[..., :n // 2] + acc[..., n // 2:n]
        n //= 2
    acc = acc[..., 0]
    return acc if lpr else ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def emu_ln_gemv(x, g, b, lpr, shift_x0=False):
    K = F(x.shape[1])
    if shift_x0:  # the prologues' arithmetic before the fix: one-pass variance about shift = x[b][0]
        shift = x[:, :1]
        t = x - shift
        dm = lane_sum(t, lpr)[:, None] / K
        var = np.maximum(lane_sum(t * t, lpr)[:, None] / K - dm * dm, F(0))
        mean = shift + dm
    else:
        mean = lane_sum(x, lpr)[:, None] / K
        t = x - mean
        var = lane_sum(t * t, lpr)[:, None] / K
    return ((x - mean) * (F(1) / np.sqrt(var + F(1e-5))) * g + b).astype(F)


def emu_combine(part, B, H, ns, ignore_m=False):
    rec = part[:B * H * ns * G.PART].reshape(B, H, ns, G.PART)
    m_s, l_s, o_s = rec[..., 0], rec[..., 1], rec[..., 2:]
    m = m_s.max(2, keepdims=True)
    w = np.where(np.isfinite(m_s), F(1), F(0)) if ignore_m else exp32(m_s - m)
    l, o = np.zeros((B, H), F), np.zeros((B, H, 64), F)
    for s_ in range(ns):
        l, o = l + w[..., s_] * l_s[..., s_], o + w[..., s_, None] * o_s[..., s_, :]
    return (o / l[..., None]).reshape(B, H * 64).astype(F)


def emu_dot(W, a, lpr, ch):
    """y[b][n]: lane j of a row group runs one fmaf chain over its chunks j + lpr i, then the xor butterfly; lane 0's sum."""
    B, N = a.shape[0], W.shape[0]
    Wr, ar = W.reshape(N, ch, lpr, 8).astype(np.float64), a.reshape(B, ch, lpr, 8).astype(np.float64)
    acc = np.zeros((B, N, lpr), F)
    for i in range(ch):
        for e in range(8):
            acc = (Wr[None, :, i, :, e] * ar[:, None, i, :, e] + acc).astype(F)  # one rounding per fused multiply-add
    o = lpr // 2
    while o:
        acc = acc + acc[..., np.arange(lpr) ^ o]
        o //= 2
    return acc[..., 0]


def emu_gemv(p, state, dt, defect=None):
    st = G.typed("gemv", p, state)
    N, K, B, epi, pro = p["N"], p["K"], p["batch"], p["epilogue"], p["prologue"]
    lpr = G.pick_lpr(K)
    ch, rp, rpw = K // (8 * lpr), 256 // lpr, G.rows_per_wg_for(N, lpr)
    W = from_bits(st[p["W"]][:N * K], dt).astype(F).reshape(N, K)
    bias = st[p["bias"]][:N] if p.get("bias") else np.zeros(N, F)
    if pro == G.PRO_LAYERNORM:
        a = emu_ln_gemv(st[p["in"]][:B * K].reshape(B, K), st[p["ln_w"]], st[p["ln_b"]], lpr if B == 1 else None, shift_x0=defect == "shift_x0")
    elif pro == G.PRO_ATTN_COMBINE:
        a = emu_combine(st[p["part"]], B, p["n_head"], p["n_split"], ignore_m=defect == "combine_no_m")
    else:
        a = st[p["in"]][:B * K].reshape(B, K)
    rows = np.arange(N)
    first = rows - (rows % rpw) // rp * rp  # the row of the workgroup's first pass that the same lanes held
    y = emu_dot(W[first if defect == "pass2_weights" else rows], a, lpr, ch) + bias[first if defect == "bias_first" else rows]
    keep = np.ones(N, dtype=bool)
    if defect == "last_row":
        keep[N - 1] = False
    got = {name: guarded(st[name]) for name in G.launch("gemv", "", **p)[3]}
    bi = np.arange(B)[:, None]
    if epi in (R.GEPI_STORE, R.GEPI_GELU, R.GEPI_RESID):
        out = st[p["out"]].copy()
        v = out[:B * N].reshape(B, N)
        new = y if epi == R.GEPI_STORE else gelu32(y) if epi == R.GEPI_GELU else (v[:, first] if defect == "resid_stale" else v) + y
        v[:, keep] = new[:, keep]
        got[p["out"]] = guarded(out)
    elif epi == R.GEPI_QKV_CACHE:
        d, bs, Tc = p["d_model"], p["kv_batch_stride"], p["n_ctx_pad"]
        out = st[p["out"]].copy()
        out[:B * d] = y[:, :d].ravel()
        off = st[p["off"]][:B].astype(np.int64)[:, None]
        if defect == "cache_clip0":
            off = np.full_like(off, off[0, 0])
        if defect == "cache_plus1":
            off = off + 1
        c = np.arange(d)[None, :]
        base = bi * bs + (c >> 6) * Tc * 64
        kc, vc = st[p["k_cache"]].copy(), st[p["v_cache"]].copy()
        kc[(base + R.kcache_index(off, c & 63)) % kc.size] = to_bits(y[:, d:2 * d], dt)  # (a kernel would leave the buffer)
        vc[(base + (R.kcache_index if defect == "cache_vswap" else R.vcache_index)(off, c & 63)) % vc.size] = to_bits(y[:, 2 * d:], dt)
        got.update({p["out"]: guarded(out), p["k_cache"]: guarded(kc), p["v_cache"]: guarded(vc)})
    else:
        if (st[p["off"]][:B] >= p["skip_before_step"]).any():
            grid, stv = G.gemv_grid(N, K), p["amax_stride"]
            av, ai = st[p["amax_val"]].copy(), st[p["amax_idx"]].copy()
            v, i = G.wg_argmax(np.where(keep[None, :], y, -np.inf).astype(F), N, K, last=defect == "argmax_last", local=defect == "idx_local")
            for c in range(B):
                av[c * stv:c * stv + grid], ai[c * stv:c * stv + grid] = v[c], i[c]
            got.update({p["amax_val"]: guarded(av), p["amax_idx"]: guarded(ai)})
            if p.get("logits_dump"):
                dump = st[p["logits_dump"]].copy()
                for c in range(B):
                    dump[c * p["logits_dump_stride"]:c * p["logits_dump_stride"] + N][keep] = y[c, keep]
                got[p["logits_dump"]] = guarded(dump)
    return got


def emu_exact(cmd, p, state, dt, defect=None):
    st = G.typed(cmd, p, state)
    new = G.advance_reference(p, st, dt, defect) if cmd == "advance" else G.embed_reference(p, st, dt)
    return {name: guarded(new.get(name, st[name])) for name in G.launch(cmd, "", **p)[3]}


def run_gemv_case(name, dt, defect=None, session=None):
    def result(gi, li, l, state):
        cmd, _, p, _ = l
        return G.grid_of(cmd, p), (emu_gemv(p, state, dt, defect) if cmd == "gemv" else emu_exact(cmd, p, state, dt, defect))
    return kernel_driver.check_groups(session or kernel_driver.Session(), G.verify, G.gemv_form, G.grid_of, dt, T.CASES[name](dt), result)


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_emulations_pass_the_whole_gpu_file(dt):
    session = kernel_driver.Session()
    for name in T.CASES:
        for what, w in sorted(run_gemv_case(name, dt, session=session).items()):
            assert w <= 1.0, (name, what, w)
    want = T.wanted_forms()
    assert want <= session.ran[dt], sorted(want - session.ran[dt], key=str)


def test_multipass_sizes_are_the_smallest_with_a_one_row_last_pass():
    for lpr, (K, N) in T.MULTIPASS.items():
        rp = 256 // lpr
        assert G.pick_lpr(K) == lpr and G.rows_per_wg_for(N, lpr) == 2 * rp and N % (2 * rp) == rp + 1
        assert G.rows_per_wg_for(2048 * rp, lpr) == rp  # one pass up to here; the first N beyond with a one-row last pass is N
        assert N == min(n for n in range(2048 * rp + 1, 2048 * rp + 4 * rp) if G.rows_per_wg_for(n, lpr) == 2 * rp and n % (2 * rp) == rp + 1)
    assert {K: (G.pick_lpr(K), K // (8 * G.pick_lpr(K))) for K in T.KS} == T.KS and G.pick_lpr(1152) == 16 and 1152 // 128 == 9


# defect -> the cases of tests/test_gpu_gemv_kernels.py it must fail on, and what the failure must say
GEMV_DEFECTS = {
    "shift_x0": (("LayerNorm outlier0 K=384", "LayerNorm outlier0 K=768", "LayerNorm outlier0 K=1280"), "its bound"),
    "last_row": (("two passes LPR=64 epilogue=0", "instantiation K=384", "two passes LPR=16 epilogue=4"), ("outside the valid output", "its bound", "not the maximum")),
    "pass2_weights": (("two passes LPR=32 epilogue=0", "two passes LPR=64 epilogue=4"), "its bound"),
    "resid_stale": (("two passes LPR=16 epilogue=2", "two passes LPR=64 epilogue=2"), "its bound"),
    "bias_first": (("two passes LPR=32 epilogue=0", "two passes LPR=16 epilogue=2"), "its bound"),
    "cache_clip0": (("LN -> QKV_CACHE d=384", "LN -> QKV_CACHE d=1280"), "outside the valid output changed"),
    "cache_plus1": (("LN -> QKV_CACHE d=384", "LN -> QKV_CACHE d=1280"), "outside the valid output changed"),
    "cache_vswap": (("LN -> QKV_CACHE d=384", "LN -> QKV_CACHE d=1280"), "outside the valid output changed"),
    "argmax_last": (("two passes LPR=64 epilogue=4", "LN -> LOGITS", "vocabulary N=51865"), "lowest row with the maximum"),
    "idx_local": (("LN -> LOGITS", "two passes LPR=32 epilogue=4"), "lowest row with the maximum"),
    "combine_no_m": (("COMBINE -> RESID n_split=3", "COMBINE -> RESID n_split=8"), "its bound"),
    "eot_recorded": (("advance batch=17", "advance batch=33"), ("n_out", "out_ids")),
    "budget": (("advance batch=17", "advance batch=33"), ("state", "done", "n_out")),
    "done_advances": (("advance batch=17", "advance batch=33"), "off"),
    "pos_row_plus1": (("advance batch=17", "advance batch=33"), " x"),
    "n_prefix4": (("advance batch=17", "advance batch=33"), ("state", "off", "tok")),
    "no_candidate": (("advance batch=17", "advance batch=33"), ("tok", "out_ids")),
    "done_no_reseed": (("advance batch=17", "advance batch=33"), " x"),
    "tie_high": (("advance batch=17", "advance batch=33"), ("tok", "out_ids")),
}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("defect", sorted(GEMV_DEFECTS))
def test_seeded_gemv_defect_fails(defect, dt):
    names, reason = GEMV_DEFECTS[defect]
    for name in names:
        try:
            run_gemv_case(name, dt, defect)
        except AssertionError as e:
            print(f"{dt} {defect}: caught at {name}: {str(e)[:160]}")
            assert any(r in str(e) for r in ([reason] if isinstance(reason, str) else reason)), (defect, name, str(e)[:300])
            continue
        pytest.fail(f"{dt}: defect {defect} passes at {name}")


def test_outlier0_is_the_only_family_the_shifted_variance_fails(capsys):
    """The finding: today's-before-the-fix arithmetic (one-pass variance about x[b][0]) stays inside the two-pass bound on every other
    LayerNorm case of the GPU file."""
    for name in T.CASES:
        if name.startswith("LayerNorm") and "outlier0" not in name:
            run_gemv_case(name, "bf16", "shift_x0")


def layout_tables(tmp_path):
    """The engine's own index functions (csrc/decode_layout.hpp), printed by tests/cpp/decode_layout_tables.cpp built with g++."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "decode_layout_tables"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "whisper.axera_amd", "csrc"), "-o", str(exe),
                    os.path.join(root, "tests", "cpp", "decode_layout_tables.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in out.splitlines()}


def test_index_maps(tmp_path):
    """frag_index / wfrag_index are bijections onto whole tiles; the K cache map covers a head's blocks exactly once; and the ONE
    definition the kernels and the engine index through (csrc/decode_layout.hpp) equals these maps element for element."""
    i = R.frag_index(np.arange(40)[:, None], np.arange(96)[None, :], 3)
    assert np.unique(i).size == i.size and i.max() < 3 * 3 * 512
    j = R.wfrag_index(np.arange(48)[:, None], np.arange(96)[None, :], 3)
    assert sorted(j.ravel()) == list(range(48 * 96))
    k = R.kcache_index(np.arange(448)[:, None], np.arange(64)[None, :])
    assert sorted(k.ravel()) == list(range(448 * 64))
    assert R.kcache_index(65, 9) == 4096 + 512 + 8 + 1 and R.frag_index(17, 41, 3) == ((1 * 3 + 1) * 64 + 1 * 16 + 1) * 8 + 1

    T = layout_tables(tmp_path)
    keys, dims = np.arange(448)[:, None], np.arange(64)[None, :]
    assert np.array_equal(T["frag"].reshape(40, 96), i)
    assert np.array_equal(T["wfrag"].reshape(40, 96), j[:40])
    assert np.array_equal(T["k"].reshape(448, 64), k)
    assert np.array_equal(T["v"].reshape(448, 64), R.vcache_index(keys, dims))
    # the packing kernels' direction is the inverse of wfrag_index; rows 40..47 are the padding of the last row block
    src = T["wfrag_source"].reshape(48 * 96, 2)
    assert np.array_equal(R.wfrag_index(src[:, 0], src[:, 1], 3), np.arange(48 * 96))
    # the readers' pieces: (block, 8-dim chunk, key) of K is where kcache_index puts dimension 8 * chunk of key 64 * block + key
    blk, ch, row = np.arange(7)[:, None, None], np.arange(8)[None, :, None], np.arange(64)[None, None, :]
    assert np.array_equal(T["kv_chunk"].reshape(7, 8, 64), R.kcache_index(blk * 64 + row, ch * 8))
    assert np.array_equal(T["v_row"], R.vcache_index(np.arange(448), 0))
    # the persistent launches' LDS V, [key / 64][(key % 64) / 8][dim][8 keys], stated here: a bijection per block whose 16-byte
    # pieces the same (block, chunk, row) walk reads with chunk = 8-key group, row = dim
    vt = T["vt"].reshape(448, 64)
    assert np.array_equal(vt, (keys >> 6) * 4096 + ((keys >> 3) & 7) * 512 + dims * 8 + (keys & 7))
    assert sorted(vt.ravel()) == list(range(448 * 64))
    assert np.array_equal(T["sizes"], [3 * 3 * 512, 48 * 96, 3 * 512, 2 * 512, 512, 448 * 64, (2 * 3 + 1) * 512])
    assert np.array_equal(T["part"], [66, 0, 1, 2, 6, ((3 * 12 + 5) * 6 + 2) * 66, 4 * 12 * 6 * 66])

    # the encoder reference's cross-K / cross-V formulas (EPI_CROSS_KV of gemm_expect): a launch whose value at (key t, column n) is
    # 128 t + n exactly, two heads, so the position of every value in the expected buffers IS the reference's map
    d, tp = 128, 448
    a = np.stack([np.arange(tp), np.ones(tp)], axis=1)
    w = np.stack([np.full(2 * d, d), np.arange(2 * d) % d], axis=1)
    bufs = dict(A=to_bits(a, "f16"), W=to_bits(w, "f16"), C=np.zeros(2 * tp * 64, np.uint16), C2=np.zeros(2 * tp * 64, np.uint16))
    exp = E.gemm_expect(dict(epi=E.EPI_CROSS_KV, M=tp, N=2 * d, K=2, batch=1, d=d, A="A", W="W", a_bs=0, lda=2, n_layer=1, t_pad=tp,
                             nbt=1, C="C", C2="C2"), bufs, "f16")
    want = (128 * keys + dims).astype(np.float64)
    for head in range(2):
        assert np.array_equal(exp["C"].ref[head * T["sizes"][5] + T["k"].reshape(448, 64)], want + 64 * head)
        assert np.array_equal(exp["C2"].ref[head * T["sizes"][5] + T["v"].reshape(448, 64)], want + 64 * head)
    assert exp["C"].written.all() and exp["C2"].written.all()


@pytest.mark.parametrize("dt", DTYPES)
def test_pair_split_carries_16_or_22_bits(dt):
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-9, 9, 200000))).astype(F)
    hi, lo = R.pair_split(x, dt)
    err = np.abs(x.astype(np.float64) - (hi.astype(np.float64) + lo))
    assert (err <= R.pair_err(x.astype(np.float64), dt)).all()
    bits = 16 if dt == "bf16" else 22
    assert (err[np.abs(x) > 2.0 ** -2] <= 2.0 ** -bits * np.abs(x[np.abs(x) > 2.0 ** -2])).all()
    assert (err / np.abs(x)).max() > 2.0 ** -(bits + 3)  # and not many more: the bound is the format's


def test_ksplit_rule_and_resident_shapes():
    assert [R.ksplit_for(k) for k in (384, 512, 768, 1280, 5120)] == [1, 2, 3, 4, 4]
    assert R.logits_resident_ok(1280, 48) and not R.logits_resident_ok(1280, 64) and R.logits_resident_ok(768, 64) and not R.logits_resident_ok(1536, 16)
