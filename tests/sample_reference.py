"""Python restatement of the temperature-fallback contract (DESIGN.md "Temperature fallback"): Philox4x32-10 in uint64
arithmetic, the uniforms and float64 Gumbel keys made from it, the sampler on top of ts_reference / score_reference, the text a
window's compression ratio is taken of, the ratio, the fallback rule and the attempt loop of the long-form pass.

The sampled rules kernel (whisper.axera_amd/csrc/decode_timestamps.hip), AX_WHISPER_CompressionRatio,
AX_WHISPER_WindowNeedsFallback and the fallback long-form loop are checked against these.

The near-tie bound. The kernel computes key = x / t - logf(-logf(u)) in float32, the reference in float64 (u itself is exact in
both). With eps = 2^-24 (half a float32 ulp, relative): the quotient x / t is off by at most eps |x| / t (2.5 eps with a division
that is not correctly rounded); L = -logf(u) lies in [6e-8, 16.7] and carries a relative error of about 2 eps (a 1-ulp logf), which
the outer logarithm turns into an ABSOLUTE error of 2 eps, plus its own rounding of at most 2 eps |g| with |g| <= 16.7; the final
sum rounds by eps |key|. One key is therefore off by at most eps (|key| + 2.5 |x| / t + 2 + 34), and a comparison of two keys by
twice that. NEAR_TIE = 16 eps (|key| + |x| / t + 20) is above that sum for both candidates with a factor of at least two to spare
(16 (|key| + |x| / t + 20) >= 2 (|key| + 2.5 |x| / t + 36) as 16 * 20 > 2 * 36). A decision whose two best reference keys are
closer than NEAR_TIE may come out either way on the GPU; every other one must match. Equal keys (two +inf logits) are no near tie:
the lowest id wins on both sides."""
import math
import zlib

import numpy as np

import longform_reference as lfr
import score_reference as sr
import ts_reference as tsr

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64 -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & MASK
        h1, l1 = p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def uniforms(words):
    """u = ((word >> 9) + 0.5) * 2^-23: exact in float32 (24 bits), never 0 or 1; returned as float64."""
    w = np.asarray(words, dtype=np.uint64)
    u = ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))
    return u


def gumbel_at(ids, n, stream, seed):
    """float64 [len(ids)]: g_i = -log(-log(u_i)) of the given ids, u_i from word i & 3 of Philox(counter (i >> 2, n, stream low,
    stream high), key (seed low, seed high))."""
    ids = np.asarray(ids, dtype=np.uint64)
    m = len(ids)
    stream, seed = int(stream), int(seed)
    w = philox4x32_10(ids >> np.uint64(2), np.full(m, n, dtype=np.uint64), np.full(m, stream & 0xFFFFFFFF, dtype=np.uint64),
                      np.full(m, stream >> 32, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    u = uniforms(np.stack(w, axis=1)[np.arange(m), (ids & np.uint64(3)).astype(np.int64)]) if m else np.zeros(0)
    return -np.log(-np.log(u))


def gumbel_row(nv, n, stream, seed):
    """gumbel_at of every id of a row."""
    return gumbel_at(np.arange(nv), n, stream, seed)


def near_tie_bound(key, x, t):
    return 16.0 * 2.0 ** -24 * (abs(key) + abs(x) / t + 20.0)


def sample(logits, seq, T, E, t, stream, seed, allowed=None):
    """One sampled step with history `seq` at temperature t -> (chosen id, float32 untempered log-probability, info).
    t <= 0: score_reference.token_logprob (the greedy decision). info adds near_tie (bool) and key_gap.
    allowed: (decide()'s info, final_allowed()) of (logits, seq) where the caller has them already (many draws on one row)."""
    t = float(np.float32(t))
    if not t > 0.0:
        c, lp, info = sr.token_logprob(logits, seq, T, E)
        return c, lp, dict(info, near_tie=False, key_gap=math.inf)
    x = np.asarray(logits, dtype=np.float64)
    info, A = allowed if allowed is not None else (tsr.decide(logits, seq, T, E)[1], sr.final_allowed(logits, seq, T, E))
    lse = tsr._lse(x[A])
    cand = np.flatnonzero(A & (x != -math.inf))  # (a -inf logit has key -inf: never drawn)
    if cand.size == 0:  # nothing finite left: eot, the clip ends
        return E, np.float32(-math.inf), dict(info, lse_allowed=lse, x_chosen=-math.inf, near_tie=False, key_gap=math.inf)
    keys = x[cand] / t + gumbel_at(cand, len(seq), stream, seed)
    best = float(keys.max())
    k = int(np.argmax(keys == best))  # lowest id among equal keys
    c = int(cand[k])
    rest = keys.copy()
    rest[k] = -math.inf
    k2 = int(np.argmax(rest))
    c2, second = int(cand[k2]), float(rest[k2])
    if second == -math.inf or best == math.inf:  # one candidate, or an exact tie of infinities: decided the same way on both sides
        gap, near = math.inf, False
    else:
        gap = best - second
        near = gap < max(near_tie_bound(best, float(x[c]), t), near_tie_bound(second, float(x[c2]), t))
    xc = float(x[c])
    return c, np.float32(sr._logprob(xc, lse)), dict(info, lse_allowed=lse, x_chosen=xc, near_tie=bool(near), key_gap=gap, runner_up=c2)


# ---------------------------------------------------------------------------------------------------- the long-form side
ASCII_SPACE = b" \t\n\r\v\f"


def window_text(ids, E, detokenize):
    """The bytes a window's compression ratio is taken of: its ids below eot, detokenised (before any post-pass), ASCII whitespace
    stripped at both ends."""
    return bytes(detokenize([i for i in ids if i < E])).strip(ASCII_SPACE)


def compression_ratio(b):
    """openai-whisper: len(text_bytes) / len(zlib.compress(text_bytes)); empty: 0 / 8."""
    b = bytes(b)
    return np.float32(len(b) / len(zlib.compress(b)))


def needs_fallback(cr, avg_lp, no_speech_lp, cr_thr, lp_thr, ns_thr):
    """openai-whisper's rule in float32; a NaN threshold switches its part off (every comparison with NaN is false)."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        need = bool(f(cr) > f(cr_thr)) or bool(f(avg_lp) < f(lp_thr))
        if bool(np.exp(f(no_speech_lp)) > f(ns_thr)) and bool(f(avg_lp) < f(lp_thr)):
            need = False  # silence: left to the silent-window rule
    return need


def loop_fallback(n_samples, decode, T, E, temperatures, cr_thr, lp_thr, ns_thr):
    """The seek loop of one file under temperature fallback. decode(seek, window_frames, attempt, temperature) -> (ids,
    no_speech_logprob, avg_logprob, text bytes). Returns every attempt, in order:
    [(seek, window_frames, advance, ids, attempt, temperature, compression_ratio, kept, skipped)]; an attempt that is not kept
    advances by 0; the last attempt is kept whatever it gives; the silent-window rule and the window rule apply to the kept one."""
    content = n_samples // lfr.HOP
    seek, out = 0, []
    while seek < content:
        wf = min(lfr.WINDOW, content - seek)
        for a, t in enumerate(temperatures):
            ids, nsp, avg, text = decode(seek, wf, a, t)
            ids = list(ids)
            cr = compression_ratio(text)
            if needs_fallback(cr, avg, nsp, cr_thr, lp_thr, ns_thr) and a + 1 < len(temperatures):
                out.append((seek, wf, 0, ids, a, float(np.float32(t)), float(cr), False, False))
                continue
            skipped = sr.is_silent(nsp, avg, ns_thr, lp_thr)
            adv = wf if skipped else lfr.split_window(ids, T, E, wf)[1]
            out.append((seek, wf, adv, ids, a, float(np.float32(t)), float(cr), True, skipped))
            seek += adv
            break
    return out
