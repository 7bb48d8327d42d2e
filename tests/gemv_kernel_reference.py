"""Float64 references of the GEMV decode family (whisper.axera_amd/csrc/decode_gemv.hip: gemv1_kernel, gemv_kernel, advance_kernel)
and of embed_kernel (decoder.hip), with per-element bounds derived from the arithmetic, no free constants. The notation, the
LayerNorm bound, the cache index maps and the generators are those of tests/decode_kernel_reference.py: u = 2^-24,
hulp(x) = half an ulp of the build's 16-bit type at |x|; every bound is first order, worst case, for a kernel that does the
stated arithmetic in fp32 in ANY order.

Linear, y[b][n] = sum_k W[n][k] a[b][k] + bias[n]: W is h16 (exact), a is fp32 with error ea (0 for PRO_PLAIN). An h16 x fp32
product has up to 35 significant bits and is NOT exact in fp32, but the kernels never round it alone: every term enters through
one fmaf, which rounds once, and an fmaf whose weight is zero returns its addend unchanged. With z_n the number of non-zero weights
of row n, a term is therefore rounded at most z_n times by the fused multiply-adds (one chain over the whole row is the worst
order; the kernels use K / LPR per lane), at most 6 times by the lane reduction (LPR <= 64 = 2^6) and once by the bias add:
z_n + 7 roundings, gamma_n = (z_n + 7) u / (1 - (z_n + 7) u) (Higham's gamma, so that the second order is in). z_n = K for the
generators' rows; the identity rows of the LayerNorm cases (z_n = 1) hand the prologue's values through under 8 u:
    E_y = |W| ea + gamma_n (|W| (|a| + ea) + |bias|)
  GEPI_STORE, q rows of GEPI_QKV_CACHE   E_y
  GEPI_RESID  out += y                   E_y + u |old| + u |ref|          (ref = old + y)
  GEPI_GELU   fp32 out                   1.13 E_y + 8 u |y|               (|g'| <= 1.13, erff within 4 ulp: decode_kernel_reference.py)
  GEPI_QKV_CACHE K / V rows (h16)        E_y + hulp(|ref| + E_y), at row off[b] of the clip's OWN slab (kcache_index / vcache_index)
  GEPI_LOGITS the dumped logits          E_y. The (amax_val, amax_idx) of a workgroup is EXACTLY the maximum, at its lowest global
              row, of the logits the GPU itself dumped for the workgroup's rows [w rpw, (w + 1) rpw), rpw = rows_per_wg_for(N, LPR).
              Without a dump: the value within the largest E_y of those rows, at a row whose own logit is that close.

PRO_LAYERNORM: the two-pass bound ln_expect(..., onepass=False) — mean K u S1, a = x - mean, var = mean a^2 — which does not depend
on which channel holds what. (Until this file existed both prologues used a one-pass variance shifted by x[b][0]; with the row's
outlier in channel 0 that is the plain E[x^2] - mean^2 cancellation: family `outlier0`.)

PRO_ATTN_COMBINE, records (m_s, l_s, o_s[64]) of a (clip, head) taken as given: m = max m_s, w_s = e^(m_s - m), l = sum w_s l_s,
o = sum w_s o_s, a = o / l. Per factor, as in the attention derivation: the argument x_s = m_s - m carries the rounding of the
subtraction and of the product with log2 e, 2 u |x_s| in the result; v_exp_f32 2 u; the multiplication with l_s or o_s u:
    ew_s = 2 u |x_s| + 3 u.   n_split terms summed in fp32: n_split u on top.
    dl = sum w_s |l_s| (ew_s + n_split u) ; do = sum w_s |o_s| (ew_s + n_split u) ; ea = (do + |a| dl) / |l| + u |a|  (one division)
  A split recorded as (-inf, 0, 0) has w_s = e^-inf = 0 exactly and contributes exactly nothing, to the value and to the bound.

advance_kernel and embed_kernel are integer- and bit-exact: advance_reference is the state machine written once (tests/ts_reference.py's
description of the loop and the kernel's comments), x[b] = float32(tok_emb[tok]) + pos[row] one correctly rounded fp32 add.
Every buffer of a launch comes back whole and is compared bit for bit; after a launch state.step is one higher and state.pad0 is 0.
"""
import numpy as np

import decode_kernel_reference as R
from decode_kernel_reference import GEPI_GELU, GEPI_LOGITS, GEPI_QKV_CACHE, GEPI_RESID, GEPI_STORE, LN_FAMILIES, SCORE_FAMILIES, f32_slack, ln_expect, strip
from encoder_kernel_reference import U32, Expect, check, check_values, from_bits, gelu64, mm64, sentinel, to_bits

PRO_PLAIN, PRO_LAYERNORM, PRO_ATTN_COMBINE = range(3)
PART = R.PART
NO_INDEX = 0x7FFFFFFF


# ------------------------------------------------------------------------------------------ launch_gemv's rules
def pick_lpr(K):
    if K % 512 == 0 and K // 512 <= 10 and K >= 1024:
        return 64
    if K % 256 == 0 and K // 256 <= 6:
        return 32
    if K % 128 == 0 and K // 128 <= 10:
        return 16
    return 0


def rows_per_wg_for(N, lpr):
    rp = 256 // lpr
    rows = (N + 2047) // 2048
    rows = (rows + rp - 1) // rp * rp
    return max(rows, rp)


def gemv_grid(N, K):
    rpw = rows_per_wg_for(N, pick_lpr(K))
    return (N + rpw - 1) // rpw


def gemv_form(cmd, p, qall=None):
    """What a launch exercises: kernel, (LPR, CH), prologue, epilogue."""
    if cmd == "gemv":
        lpr = pick_lpr(p["K"])
        kern = "gemv1" if p["batch"] == 1 and p["prologue"] != PRO_ATTN_COMBINE else "gemv<1>" if p["batch"] == 1 else "gemv<4>"
        return (kern, lpr, p["K"] // (8 * lpr), p["prologue"], p["epilogue"])
    if cmd == "advance":
        return ("advance", (p["batch"] + 15) // 16, "forced" if p.get("forced") else "greedy")
    return (cmd,)


def grid_of(cmd, p):
    if cmd == "gemv":
        return gemv_grid(p["N"], p["K"]), 1, 1
    if cmd == "advance":
        return (p["batch"] + 15) // 16, 1, 1
    return p["batch"], 1, 1


# ------------------------------------------------------------------------------------------ buffers
GEMV_H16 = ("W", "k_cache", "v_cache")
GEMV_I32 = ("off", "amax_idx")
ADV_I32 = ("amax_idx", "state", "off", "tok", "done", "n_out", "out_ids", "done_host", "max_new_clip", "sot", "forced", "argmax_dump")
POINTERS = {"gemv": ("W", "bias", "in", "ln_w", "ln_b", "part", "out", "k_cache", "v_cache", "off", "amax_val", "amax_idx", "logits_dump"),
            "advance": ("amax_val", "amax_idx", "state", "off", "tok", "done", "n_out", "out_ids", "done_host", "max_new_clip", "sot", "forced",
                        "argmax_dump", "tok_emb", "pos", "x"),
            "embed": ("tok_emb", "pos", "tok", "off", "x")}


def typed(cmd, p, bufs):
    out = dict(bufs)
    for k in POINTERS[cmd]:
        if p.get(k):
            if cmd == "gemv":
                t = np.uint16 if k in GEMV_H16 else np.int32 if k in GEMV_I32 else np.float32
            else:
                t = np.uint16 if k == "tok_emb" else np.int32 if (k in ADV_I32 or k in ("tok", "off")) else np.float32
            out[p[k]] = np.ascontiguousarray(bufs[p[k]]).ravel().view(t)
    return out


def launch(cmd, ident, **p):
    """Every buffer the launch names is dumped: what it must write is checked against the reference, everything else bit for bit."""
    outs = []
    for k in POINTERS[cmd]:
        if p.get(k) and p[k] not in outs and k not in ("W", "tok_emb", "pos"):  # (the large read-only tables stay on the device)
            outs.append(p[k])
    return cmd, ident, p, outs


# ------------------------------------------------------------------------------------------ gemv
def combine_expect(part, B, H, n_split):
    """(a, ea) float64 [B][64 H] of the attention-combine prologue from the fp32 records part[B][H][n_split][66]."""
    rec = part[:B * H * n_split * PART].astype(np.float64).reshape(B, H, n_split, PART)
    m_s, l_s, o_s = rec[..., 0], rec[..., 1], rec[..., 2:]
    m = m_s.max(2, keepdims=True)
    assert np.isfinite(m).all(), "a (clip, head) without any key"
    with np.errstate(invalid="ignore"):
        x = np.where(np.isfinite(m_s), m_s - m, 0.0)
    w = np.where(np.isfinite(m_s), np.exp(x), 0.0)
    ew = 2 * U32 * np.abs(x) + 3 * U32 + n_split * U32
    l = (w * l_s).sum(2)
    o = (w[..., None] * o_s).sum(2)
    dl = (w * np.abs(l_s) * ew).sum(2)
    do = ((w * ew)[..., None] * np.abs(o_s)).sum(2)
    a = o / l[..., None]
    ea = (do + np.abs(a) * dl[..., None]) / np.abs(l)[..., None] + U32 * np.abs(a)
    return a.reshape(B, H * 64), ea.reshape(B, H * 64)


def gemv_inputs(p, bufs):
    B, K = p["batch"], p["K"]
    if p["prologue"] == PRO_ATTN_COMBINE:
        return combine_expect(bufs[p["part"]], B, p["n_head"], p["n_split"])
    x = bufs[p["in"]][:B * K].astype(np.float64).reshape(B, K)
    if p["prologue"] == PRO_LAYERNORM:
        y, e, _ = ln_expect(x, bufs[p["ln_w"]], bufs[p["ln_b"]], onepass=False)
        return y, e
    return x, np.zeros_like(x)


def gemv_expect(p, bufs, dt):
    """One launch_gemv: ({buffer name: Expect} for every buffer it may write, info)."""
    N, K, B, epi = p["N"], p["K"], p["batch"], p["epilogue"]
    W = from_bits(bufs[p["W"]][:N * K], dt).reshape(N, K)
    bias = bufs[p["bias"]][:N].astype(np.float64) if p.get("bias") else np.zeros(N)
    a, ea = gemv_inputs(p, bufs)
    z = (W != 0).sum(1) + 7
    gamma = (z * U32 / (1 - z * U32))[None, :]
    ref = mm64(a, W) + bias
    bound = mm64(ea, np.abs(W)) + gamma * (mm64(np.abs(a) + ea, np.abs(W)) + np.abs(bias)) + 1e-300
    out = {}
    for key, size in (("out", 4), ("k_cache", 2), ("v_cache", 2), ("logits_dump", 4)):
        if p.get(key):
            out[p[key]] = Expect(np.ascontiguousarray(bufs[p[key]]).view(np.uint16).ravel(), size)
    bi, ni = np.arange(B)[:, None], np.arange(N)[None, :]
    info = dict(logits=ref, bound=bound)
    if epi == GEPI_STORE:
        out[p["out"]].put(bi * N + ni, ref, bound)
    elif epi == GEPI_GELU:
        out[p["out"]].put(bi * N + ni, gelu64(ref), 1.13 * bound + 8 * U32 * np.abs(ref))
    elif epi == GEPI_RESID:
        old = bufs[p["out"]][:B * N].astype(np.float64).reshape(B, N)
        out[p["out"]].put(bi * N + ni, old + ref, bound + U32 * np.abs(old) + U32 * np.abs(old + ref))
    elif epi == GEPI_QKV_CACHE:
        d = p["d_model"]
        out[p["out"]].put(bi * d + np.arange(d)[None, :], ref[:, :d], bound[:, :d])
        R._cache_put(out, p, bufs, dt, ref[:, d:], bound[:, d:])
    elif epi == GEPI_LOGITS:
        info["wrote"] = bool((bufs[p["off"]][:B] >= p["skip_before_step"]).any())
        if p.get("logits_dump") and info["wrote"]:
            out[p["logits_dump"]].put(bi * p["logits_dump_stride"] + ni, ref, bound)
    else:
        raise ValueError(epi)
    return out, info


def wg_argmax(logits, N, K, last=False, local=False):
    """(max, lowest row holding it) per workgroup of fp32 logits [B][N], by launch_gemv's row split."""
    rpw = rows_per_wg_for(N, pick_lpr(K))
    grid = (N + rpw - 1) // rpw
    val, idx = np.zeros((logits.shape[0], grid), np.float32), np.zeros((logits.shape[0], grid), np.int32)
    for w in range(grid):
        sub = logits[:, w * rpw:min(N, (w + 1) * rpw)]
        val[:, w] = sub.max(1)
        hit = sub == val[:, w:w + 1]
        at = (hit.shape[1] - 1 - np.argmax(hit[:, ::-1], 1)) if last else np.argmax(hit, 1)
        idx[:, w] = at + (0 if local else w * rpw)
    return val, idx


def same_bits(ident, name, got_bits, want):
    a, b = np.ascontiguousarray(got_bits).view(np.uint16).ravel(), np.ascontiguousarray(want).view(np.uint16).ravel()
    assert a.size == b.size, (ident, name, a.size, b.size)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{ident} {name}: {bad.size} 16-bit words differ from what the launch must leave, first at word {bad[0]}"


def verify_gemv(ident, p, state, got, dt):
    exp, info = gemv_expect(p, state, dt)
    epi, N, K, B = p["epilogue"], p["N"], p["K"], p["batch"]
    label = f"gemv {gemv_form('gemv', p)[0]} prologue {p['prologue']} epilogue {epi}"
    notes = {}
    for name, e in exp.items():
        key = [k for k in ("out", "k_cache", "v_cache", "logits_dump") if p.get(k) == name][0]
        notes[f"{label} {key}"] = check(f"{ident} {name}", got[name], e, dt)
    written = set(exp) | ({p["amax_val"], p["amax_idx"]} if epi == GEPI_LOGITS else set())
    for name in got:  # the inputs: read-only
        if name not in written:
            same_bits(ident, name, strip(ident, got[name]), state[name])
    if epi != GEPI_LOGITS:
        return notes
    grid, st = gemv_grid(N, K), p["amax_stride"]
    av, ai = strip(ident, got[p["amax_val"]]), strip(ident, got[p["amax_idx"]])
    if not info["wrote"]:
        same_bits(ident, "amax_val (every clip below skip_before_step)", av, state[p["amax_val"]])
        same_bits(ident, "amax_idx (every clip below skip_before_step)", ai, state[p["amax_idx"]])
        return notes
    gv, gi = av.view(np.float32), ai.view(np.int32)
    want_v, want_i = state[p["amax_val"]].copy(), state[p["amax_idx"]].copy()
    if p.get("logits_dump"):
        lg = strip(ident, got[p["logits_dump"]]).view(np.float32)
        lg = np.stack([lg[c * p["logits_dump_stride"]:c * p["logits_dump_stride"] + N] for c in range(B)])
        rv, ri = wg_argmax(lg, N, K)
        for c in range(B):
            want_v[c * st:c * st + grid], want_i[c * st:c * st + grid] = rv[c], ri[c]
        assert np.array_equal(gv.view(np.uint32), want_v.view(np.uint32)), f"{ident}: an argmax partial is not the maximum of its workgroup's dumped rows (or a slot beyond the grid changed)"
        bad = np.nonzero(gi != want_i)[0]
        assert bad.size == 0, f"{ident}: argmax index {gi[bad[0]]} in slot {bad[0]} where the lowest row with the maximum is {want_i[bad[0]]}"
        return notes
    mask = np.zeros(gv.size, dtype=bool)
    for c in range(B):
        mask[c * st:c * st + grid] = True
    assert np.array_equal(gv.view(np.uint32)[~mask], want_v.view(np.uint32)[~mask]) and np.array_equal(gi[~mask], want_i[~mask]), f"{ident}: an amax slot beyond the grid changed"
    rpw = rows_per_wg_for(N, pick_lpr(K))
    refv = wg_argmax(info["logits"], N, K)[0]
    bmax = np.stack([info["bound"][:, w * rpw:(w + 1) * rpw].max(1) for w in range(grid)], 1)
    for c in range(B):
        v, i = gv[c * st:c * st + grid].astype(np.float64), gi[c * st:c * st + grid]
        assert ((i >= np.arange(grid) * rpw) & (i < np.minimum(N, (np.arange(grid) + 1) * rpw))).all(), f"{ident}: an argmax index outside its workgroup's rows"
        notes[f"{label} max"] = max(notes.get(f"{label} max", 0.0), check_values(ident, v, refv[c], bmax[c]),
                                    check_values(ident + " row of the index", v, info["logits"][c, i], info["bound"][c, i]))
    return notes


# ------------------------------------------------------------------------------------------ advance, embed
def embed_row(tok_emb_bits, pos, tok, row, d, dt):
    """float32(tok_emb[tok]) + pos[row]: one correctly rounded fp32 add per element."""
    e = from_bits(tok_emb_bits[tok * d:(tok + 1) * d], dt).astype(np.float32)
    return e + pos[row * d:(row + 1) * d]


def merge_partials(val, idx):
    """argmax_take over the partials from (-inf, NO_INDEX): greater wins, equal with the lower index wins, a NaN never."""
    v, i = np.float32(-np.inf), NO_INDEX
    for ov, oi in zip(val, idx):
        if ov > v or (ov == v and oi < i):
            v, i = ov, int(oi)
    return i


def advance_reference(p, bufs, dt, defect=None):
    """The loop state machine of one launch_advance. bufs: typed initial content. Returns {buffer name: content after}."""
    B, n_ctx, d, V = p["batch"], p["n_ctx"], p["d_model"], p["n_vocab"]
    new = {p[k]: bufs[p[k]].copy() for k in POINTERS["advance"] if p.get(k)}
    get = lambda k: new[p[k]] if p.get(k) else None  # noqa: E731
    state, off, tok, done, n_out, out_ids, x = (get(k) for k in ("state", "off", "tok", "done", "n_out", "out_ids", "x"))
    forced, dump, done_host, mnc, sot = (get(k) for k in ("forced", "argmax_dump", "done_host", "max_new_clip", "sot"))
    av, ai = bufs[p["amax_val"]], bufs[p["amax_idx"]]
    n_pre = p.get("n_prefix", 0) or 4
    if defect == "n_prefix4":
        n_pre = 4
    nf = p.get("n_forced", 0)
    for b in range(B):
        s = int(off[b])
        room = s + 1 < n_ctx
        pos_row = s + 1 if (room or defect == "pos_row_plus1") else n_ctx - 1
        greedy = forced is None
        done_b = bool(done[b]) if greedy else False
        t, adv = int(tok[b]), not done_b
        if done_b:
            if defect == "done_advances":
                adv = True
        elif s < n_pre - 1:
            t = int(sot[s + 1])
            tok[b] = t
        else:
            st = p["amax_stride"]
            idx = merge_partials(av[b * st:b * st + p["n_part"]], ai[b * st:b * st + p["n_part"]])
            if defect == "tie_high":
                vals = av[b * st:b * st + p["n_part"]]
                ok = ~np.isnan(vals)
                if ok.any() and vals[ok].max() > -np.inf:
                    idx = int(ai[b * st:b * st + p["n_part"]][ok][vals[ok] == vals[ok].max()].max())
            if not 0 <= idx < V and defect != "no_candidate":
                idx = 0
            gi = s - (n_pre - 1)
            if not greedy:
                if gi < nf:
                    t = int(forced[b * nf + gi])
            else:
                budget = min(int(mnc[b]), p["max_new"]) if mnc is not None else p["max_new"]
                if defect == "budget":
                    budget += 1
                if idx == p["eot"] and defect == "eot_recorded":
                    out_ids[b * n_ctx + n_out[b]] = idx
                    n_out[b] += 1
                if idx == p["eot"] or s + 1 >= n_ctx or (n_out[b] - (idx == p["eot"] and defect == "eot_recorded")) >= budget:
                    done[b] = 1
                    state[1] += 1
                    if done_host is not None:
                        done_host[b] = 1
                    adv = False
                else:
                    out_ids[b * n_ctx + n_out[b]] = idx
                    n_out[b] += 1
                    t = idx
            if dump is not None and gi <= nf:
                dump[b * (nf + 1) + gi] = idx
            tok[b] = t
        if adv and room:
            off[b] = s + 1
        if not (done_b and defect == "done_no_reseed"):
            x[b * d:(b + 1) * d] = embed_row(bufs[p["tok_emb"]], bufs[p["pos"]], t % V, pos_row % n_ctx, d, dt)
    state[0] += 1
    state[2] = 0
    return new


def verify_exact(cmd, ident, p, state, got, dt):
    want = advance_reference(p, state, dt) if cmd == "advance" else embed_reference(p, state, dt)
    for name in got:
        same_bits(ident, name, strip(ident, got[name]), want.get(name, state[name]))
    return {cmd: 0.0}


def embed_reference(p, bufs, dt):
    x = bufs[p["x"]].copy()
    d = p["d"]
    for b in range(p["batch"]):
        x[b * d:(b + 1) * d] = embed_row(bufs[p["tok_emb"]], bufs[p["pos"]], int(bufs[p["tok"]][b]), int(bufs[p["off"]][b]), d, dt)
    return {p["x"]: x}


def verify(cmd, ident, p, state, got, dt, prev=None):
    """state: buffer name -> content before the launch; got: buffer name -> uint16 dump with guards after it."""
    st = typed(cmd, p, state)
    return verify_gemv(ident, p, st, got, dt) if cmd == "gemv" else verify_exact(cmd, ident, p, st, got, dt)


# ------------------------------------------------------------------------------------------ generators
def outlier0_stream(rng, B, K):
    """realistic_stream with its LARGER outlier channel (the one at -14 sqrt(K)) exchanged with channel 0 in x, gains and bias; the
    caller exchanges the weight columns alike. The generators of this suite and tools/modelgen.py keep outliers off channel 0."""
    x, g, b, oc = R.realistic_stream(rng, B, K)
    c = int(oc[1])
    for a in (x, g, b):
        a[..., [0, c]] = a[..., [c, 0]]
    return x, g, b, np.array([oc[0], 0]), c


def combine_records(rng, dt, B, H, n_split, n_keys, empty):
    """fp32 records [B][H][n_split][66] as the attention kernel leaves them: the score families of SCORE_FAMILIES dealt over the
    (clip, head) pairs, keys dealt over the splits in contiguous ranges, split `empty` (if any) without a key: (-inf, 0, 0)."""
    rec = np.zeros((B, H, n_split, PART), np.float32)
    live = [s for s in range(n_split) if s != empty]
    edges = np.linspace(0, n_keys, len(live) + 1).astype(int)
    for c in range(B):
        for h in range(H):
            q, k, v = R.attn_qkv(rng, n_keys, dt, SCORE_FAMILIES[(c * H + h) % len(SCORE_FAMILIES)])
            s = 0.125 * (k.astype(np.float64) @ q.astype(np.float64))
            rec[c, h, :, 0] = -np.inf
            for i, sp in enumerate(live):
                ss, vv = s[edges[i]:edges[i + 1]], v[edges[i]:edges[i + 1]].astype(np.float64)
                w = np.exp(ss - ss.max())
                rec[c, h, sp, 0], rec[c, h, sp, 1], rec[c, h, sp, 2:] = ss.max(), w.sum(), w @ vv
    return rec.ravel()


def gemv_group(dt, seed, *, K, N, batch, pro, epi, family="benign", ln_shift=0, d_model=0, offs=None, n_ctx_pad=448, n_split=1, empty=None,
               skip=0, dump=True, ties=False, bias=True, probe=False):
    """One launch_gemv with everything around its outputs holding the sentinel. probe: rows 0 .. K - 1 of W are the identity, so
    that those outputs are the prologue's own values and their bound is the prologue's (under random rows the common-mode error of
    a wrong rstd cancels like the dot product itself, by ~ sqrt(K), and hides below the any-sign bound |W| ea)."""
    rng = np.random.default_rng(seed)
    B = batch
    b, p = {}, dict(N=N, K=K, batch=B, prologue=pro, epilogue=epi)
    oc, swap = (), None
    if pro == PRO_LAYERNORM:
        if family == "realistic":
            x, g, be, oc = R.realistic_stream(rng, B, K)
        elif family == "outlier0":
            x, g, be, oc, swap = outlier0_stream(rng, B, K)
        else:
            fams = LN_FAMILIES[ln_shift % len(LN_FAMILIES):] + LN_FAMILIES[:ln_shift % len(LN_FAMILIES)]
            x, g, be = R.ln_rows(rng, B, K, fams), rng.uniform(0.5, 1.5, K).astype(np.float32), rng.uniform(-1, 1, K).astype(np.float32)
        b.update({"in": f32_slack(x, K), "ln_w": g, "ln_b": be})
        p.update({"in": "in", "ln_w": "ln_w", "ln_b": "ln_b"})
    elif pro == PRO_PLAIN:
        b["in"], p["in"] = f32_slack(R.hidden_rows(rng, B, K, family), K), "in"
    else:
        H = K // 64
        b["part"] = f32_slack(combine_records(rng, dt, B, H, n_split, 37 + 11 * n_split, empty), PART)
        p.update(part="part", n_head=H, n_split=n_split)
    wfam = "benign" if family == "benign" else "realistic"
    if swap is not None:  # the small columns sit on the outlier channels: draw them where realistic_stream has them, then exchange
        w = R.weights(rng, N, K, dt, wfam, (oc[0], swap))
        w[:, [0, swap]] = w[:, [swap, 0]]
    else:
        w = R.weights(rng, N, K, dt, wfam, oc)
    if probe:
        w[:K] = np.eye(K, dtype=np.float32)
    bias_v = rng.uniform(-1, 1, N).astype(np.float32)
    if epi == GEPI_LOGITS and ties and N >= 8:  # rows (and bias) of clip 0's largest logit duplicated: the lowest index has to win
        a, _ = gemv_inputs(dict(p, batch=1), typed("gemv", p, b))
        top = int(np.argmax(mm64(a, w.astype(np.float64))[0] + (bias_v if bias else 0)))
        lpr = pick_lpr(K)
        rp, rpw = 256 // lpr, rows_per_wg_for(N, lpr)
        for r in {(top + 1) % N, (top + max(rp // 2, 1)) % N, (top + rp) % N, (top + rpw) % N, (top + 3 * rpw + 1) % N, N - 1}:
            w[r], bias_v[r] = w[top], bias_v[top]
    b["W"], p["W"] = to_bits(w, dt), "W"
    if bias:
        b["bias"], p["bias"] = bias_v, "bias"
    if epi in (GEPI_STORE, GEPI_GELU):
        b["out"] = sentinel((B + 1) * N, 4)
    elif epi == GEPI_RESID:
        b["out"] = f32_slack(rng.standard_normal(B * N) * (1.0 if family == "benign" else 3.0), N)
    elif epi == GEPI_QKV_CACHE:
        bs = d_model * n_ctx_pad + 4096 + 64  # slack between the clips' slabs
        b.update(out=sentinel((B + 1) * d_model, 4), k_cache=sentinel(B * bs, 2), v_cache=sentinel(B * bs, 2), off=np.asarray(offs, dtype=np.int32))
        p.update(k_cache="k_cache", v_cache="v_cache", off="off", d_model=d_model, n_ctx_pad=n_ctx_pad, kv_batch_stride=bs)
    elif epi == GEPI_LOGITS:
        grid = gemv_grid(N, K)
        b.update(off=np.asarray(offs if offs is not None else np.arange(B) + 3, dtype=np.int32), amax_val=sentinel(B * (grid + 2), 4),
                 amax_idx=sentinel(B * (grid + 2), 4))
        p.update(off="off", amax_val="amax_val", amax_idx="amax_idx", amax_stride=grid + 2, skip_before_step=skip)
        if dump:
            b["logits_dump"] = sentinel(B * (N + 7), 4)
            p.update(logits_dump="logits_dump", logits_dump_stride=N + 7)
    if "out" in b:
        p["out"] = "out"
    return b, [launch("gemv", f"gemv.K{K}.N{N}.b{B}.p{pro}.e{epi}.{family}{ln_shift}.s{n_split}.skip{skip}.{'dump' if dump else 'nodump'}.{seed}", **p)]


V_ADV, CTX_ADV, EOT_ADV = 1000, 24, 997


def advance_group(dt, seed, *, batch, d, n_part, n_prefix=0, forced=False, n_forced=5, dump=True, done_host=True, max_new_clip=True, relaunch=True):
    """One launch_advance (and a second on the same buffers) over a batch whose clips are dealt over every state of the loop:
    prefix steps, the first sampled step, an ordinary step, a tie whose lower index sits in a LATER partial, the winner in the last
    partial, no candidate at all, eot, the context end, the budget reached / one below it, a finished clip. Partials a clip does
    not read (prefix, finished) hold the NaN sentinel."""
    rng = np.random.default_rng(seed)
    B, V, T = batch, V_ADV, CTX_ADV
    n_pre = n_prefix or 4
    stride = n_part + 3
    av = sentinel(B * stride, 4).view(np.float32).copy()
    ai = sentinel(B * stride, 4).view(np.int32).copy()
    off, tok, done, n_out = np.zeros(B, np.int32), rng.integers(0, V - 10, B).astype(np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    mnc = np.full(B, 50, np.int32)
    max_new = 12
    kinds = ("prefix0", "prefix_last", "first", "ordinary", "tie_later", "win_last", "none", "none_inf0", "eot", "ctx_end", "budget", "budget_m1",
             "done", "done_ctx_end", "clip_budget", "nan_mixed")
    for c in range(B):
        kind = kinds[(c + seed) % len(kinds)]
        sl = slice(c * stride, c * stride + n_part)
        vals = rng.standard_normal(n_part).astype(np.float32)
        idxs = rng.permutation(V - 10)[:n_part].astype(np.int32)  # ids below 990: never eot
        s = n_pre - 1 + 2 + c % 5
        n_out[c] = s - (n_pre - 1)
        if kind == "prefix0":
            s, vals, idxs = 0, None, None
            n_out[c] = 0
        elif kind == "prefix_last":
            s, vals, idxs = n_pre - 2, None, None
            n_out[c] = 0
        elif kind == "first":
            s = n_pre - 1
            n_out[c] = 0
        elif kind == "tie_later" and n_part >= 2:
            i, j = sorted(rng.choice(n_part, 2, replace=False))
            vals[i] = vals[j] = 9.0
            idxs[i], idxs[j] = 700, 300  # the lower index sits in the later partial
        elif kind == "win_last":
            vals[-1] = 9.0
        elif kind == "none":
            vals[:], idxs[:] = -np.inf, NO_INDEX
        elif kind == "none_inf0":
            vals[:] = -np.inf
        elif kind == "eot":
            vals[rng.integers(n_part)] = 9.0
            idxs[np.argmax(vals)] = EOT_ADV
        elif kind == "ctx_end":
            s = T - 1
            n_out[c] = 3
        elif kind == "budget":
            n_out[c] = max_new
        elif kind == "budget_m1":
            n_out[c] = max_new - 1
        elif kind == "clip_budget":
            mnc[c] = n_out[c]
        elif kind in ("done", "done_ctx_end"):
            done[c] = 1
            s = T - 1 if kind == "done_ctx_end" else s
            vals, idxs = None, None
        elif kind == "nan_mixed" and n_part >= 2:
            vals[0] = np.nan
        if forced and kind in ("done", "done_ctx_end"):
            done[c] = 0
        off[c] = s
        if vals is not None:
            av[sl], ai[sl] = vals, idxs
    b = dict(amax_val=av, amax_idx=ai, state=np.array([7, 2, 0, 0], np.int32), off=off, tok=tok, sot=rng.integers(0, V, 4).astype(np.int32),
             tok_emb=to_bits(rng.standard_normal(V * d), dt), pos=rng.standard_normal(T * d).astype(np.float32), x=sentinel((B + 1) * d, 4),
             done=np.concatenate([done, sentinel(2, 4).view(np.int32)]), n_out=np.concatenate([n_out, sentinel(2, 4).view(np.int32)]),
             out_ids=sentinel((B + 1) * T, 4))
    b["off"] = np.concatenate([off, sentinel(2, 4).view(np.int32)])
    b["tok"] = np.concatenate([tok, sentinel(2, 4).view(np.int32)])
    p = dict(batch=B, n_part=n_part, amax_stride=stride, n_ctx=T, eot=EOT_ADV, max_new=max_new, n_vocab=V, d_model=d, n_prefix=n_prefix,
             amax_val="amax_val", amax_idx="amax_idx", state="state", off="off", tok="tok", sot="sot", tok_emb="tok_emb", pos="pos", x="x",
             done="done", n_out="n_out", out_ids="out_ids")
    if forced:
        # gi < n_forced, gi == n_forced (off = n_pre - 1 + n_forced) and beyond are all among the clips
        f_off = np.array([n_pre - 1 + (c % (n_forced + 2)) for c in range(B)], np.int32)
        keep = off[:B] < n_pre - 1
        b["off"][:B] = np.where(keep, off[:B], f_off)
        b["forced"] = np.concatenate([rng.integers(0, V, B * n_forced).astype(np.int32), sentinel(2, 4).view(np.int32)])
        p.update(forced="forced", n_forced=n_forced)
        for c in range(B):  # every clip that samples reads partials
            sl = slice(c * stride, c * stride + n_part)
            if not keep[c] and np.isnan(av[sl]).all():
                av[sl], ai[sl] = rng.standard_normal(n_part).astype(np.float32), rng.permutation(V - 10)[:n_part].astype(np.int32)
        if dump:
            b["argmax_dump"] = sentinel((B + 1) * (n_forced + 1), 4)
            p["argmax_dump"] = "argmax_dump"
    else:
        if max_new_clip:
            b["max_new_clip"], p["max_new_clip"] = np.concatenate([mnc, sentinel(2, 4).view(np.int32)]), "max_new_clip"
        if done_host:
            b["done_host"], p["done_host"] = np.zeros(B + 2, np.int32), "done_host"
    ident = f"advance.b{B}.d{d}.np{n_part}.pre{n_prefix}.{'forced' if forced else 'greedy'}.{seed}"
    ls = [launch("advance", ident, **p)]
    if relaunch:
        ls.append(launch("advance", ident + ".again", **p))
    return b, ls


def embed_group(dt, seed, *, batch, d):
    rng = np.random.default_rng(seed)
    V, T = 50, CTX_ADV
    off = rng.integers(0, T, batch).astype(np.int32)
    off[0], off[-1] = 0, T - 1
    b = dict(tok_emb=to_bits(rng.standard_normal(V * d), dt), pos=rng.standard_normal(T * d).astype(np.float32),
             tok=rng.integers(0, V, batch).astype(np.int32), off=off, x=sentinel((batch + 1) * d, 4))
    return b, [launch("embed", f"embed.b{batch}.d{d}", batch=batch, d=d, n_vocab=V, n_ctx=T, tok_emb="tok_emb", pos="pos", tok="tok", off="off", x="x")]
