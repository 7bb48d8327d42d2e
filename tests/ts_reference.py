"""Python restatement of the segment-timestamp contract (DESIGN.md "Segment timestamps"): the decoding rules applied at
every sampled step, the host-side segment split, and the timestamp-mode greedy loop over the oracle's decoder_step.

The GPU kernel (whisper.axera_amd/csrc/decode_timestamps.hip) and AX_WHISPER_SplitSegments are checked against these."""
import math

import numpy as np

N_TIMESTAMPS = 1501  # 0.00 .. 30.00 s in 0.02 s steps
MAX_INITIAL = 50     # rule 4: the first id is a timestamp of at most 1.0 s


def allowed(seq, T, E, nv):
    """Rules 1-4: bool [nv], True where the id may follow the history `seq` (ids sampled so far, prefix excluded)."""
    n = len(seq)
    ok = np.ones(nv, dtype=bool)
    ok[E + 1:T] = False                                         # rule 1
    last_ts = n >= 1 and seq[-1] >= T
    penult_ts = n < 2 or seq[-2] >= T
    if last_ts and penult_ts:                                   # rule 2
        ok[T:] = False
    if last_ts and not penult_ts:
        ok[:E] = False
    ts = [t for t in seq if t >= T]
    if ts:                                                      # rule 3
        t_last = ts[-1]
        ok[T:min(t_last if (last_ts and not penult_ts) else t_last + 1, nv)] = False
    if n == 0:                                                  # rule 4
        ok[:T] = False
        ok[T + MAX_INITIAL + 1:] = False
    return ok


def _lse(v):
    v = v[~np.isnan(v)]
    if v.size == 0:
        return -math.inf
    m = float(v.max())
    if m == -math.inf or m == math.inf:
        return m
    return m + math.log(float(np.exp(v - m).sum()))


def decide(logits, seq, T, E):
    """Rules 1-6 on one fp32 row -> (chosen id, info). info: lse, max_text, rule5 (bool), branch2 ("closed" / "open" / None),
    margin (the smaller of the top-two gap of the candidates and |lse - max_text|, inf where undefined)."""
    x = np.asarray(logits, dtype=np.float64)
    nv = x.size
    ok = allowed(seq, T, E, nv) & ~np.isnan(x)
    text = ok.copy()
    text[T:] = False
    tsm = ok.copy()
    tsm[:T] = False
    max_text = float(x[text].max()) if text.any() else -math.inf
    lse = _lse(x[tsm])
    rule5 = lse > max_text                                      # rule 5 (strict)
    cand = tsm if rule5 else ok
    vals = np.where(cand, x, -math.inf)
    best = float(vals.max())
    chosen = E if best == -math.inf else int(np.argmax(vals == best))  # rule 6: first maximum, nothing finite -> eot
    srt = np.sort(vals[np.isfinite(vals)])
    gap = float(srt[-1] - srt[-2]) if srt.size >= 2 else math.inf
    d5 = abs(lse - max_text) if math.isfinite(lse) and math.isfinite(max_text) else math.inf
    n = len(seq)
    last_ts = n >= 1 and seq[-1] >= T
    penult_ts = n < 2 or seq[-2] >= T
    branch2 = ("closed" if penult_ts else "open") if last_ts else None
    return chosen, dict(lse=lse, max_text=max_text, rule5=bool(rule5), branch2=branch2, margin=min(gap, d5))


def split_segments(ids, T, E, clip_seconds):
    """The segmenter's pseudo-code, literally -> [(start, end, tok_begin, tok_end)]."""
    ids = list(ids)
    n = len(ids)
    ts = lambda i: ids[i] >= T
    time = lambda t: (t - T) * 0.02
    segs = []

    def emit(lo, hi, t0, t1):
        txt = [i for i in range(lo, hi) if ids[i] < E]
        if txt:
            segs.append((t0, t1, txt[0], txt[-1] + 1))

    cuts = [i for i in range(1, n) if ts(i - 1) and ts(i)]
    if cuts:
        bounds = cuts + ([n] if n >= 2 and ts(n - 1) and not ts(n - 2) else [])
        prev, prev_end = 0, 0.0
        for b in bounds:
            prev_end = time(ids[b - 1])
            emit(prev, b, time(ids[prev]), prev_end)
            prev = b
        if prev < n:
            emit(prev, n, time(ids[prev]) if ts(prev) else prev_end, clip_seconds)
    else:
        last = [t for t in ids if t >= T]
        end = time(last[-1]) if last and last[-1] != T else clip_seconds
        emit(0, n, 0.0, end)
    return segs


def greedy_ts(orc, ck, cv, prefix, max_new=0, want_logits=False):
    """The engine's timestamp-mode loop on the oracle: prefix [sot, lang, transcribe], a decision at every step from the
    one that fed `transcribe` on; a clip stops at eot, at the context end or at its budget (advance_kernel).
    Returns (ids, infos[, logits rows])."""
    cfg = orc.cfg
    T, E, n_ctx = int(cfg["no_timestamps"]) + 1, int(cfg["eot"]), int(cfg["n_text_ctx"])
    if max_new <= 0 or max_new > n_ctx - 3:
        max_new = n_ctx - 3
    sk, sv = orc.new_self_cache()
    ids, infos, rows = [], [], []
    tok = prefix[0]
    for s in range(n_ctx):
        lg = orc.decoder_step(tok, s, ck, cv, sk, sv, want_logits=s >= 2)
        if s < 2:
            tok = prefix[s + 1]
            continue
        c, info = decide(lg, ids, T, E)
        infos.append(info)
        if want_logits:
            rows.append(lg.copy())
        if c == E or s + 1 >= n_ctx or len(ids) >= max_new:
            break
        ids.append(c)
        tok = c
    return (ids, infos, np.array(rows)) if want_logits else (ids, infos)


def crafted_cases(nv):
    """Hand-built (name, logits, history, expected id): one case per branch of rules 1-6, exact ties, NaN, all -inf.
    nv 51865 (multilingual) or 51866 (turbo layout)."""
    E = 50257
    T = 50364 if nv == 51865 else 50365
    base = lambda v=-10.0: np.full(nv, v, dtype=np.float32)
    out = []

    x = base(); x[E + 5] = 100.0; x[7] = 5.0
    out.append(("rule1_specials_masked", x, [T, 5], 7))
    x = base(); x[T + 40] = 50.0; x[9] = 1.0
    out.append(("rule2_pair_closed_masks_timestamps", x, [T, 5, T + 30, T + 30], 9))
    x = base(); x[5] = 50.0; x[E] = 3.0; x[T + 12] = 2.0
    out.append(("rule2_pair_open_masks_text_keeps_eot", x, [T, 5, T + 10], E))
    x = base(); x[5] = 50.0; x[E] = 3.0; x[T + 12] = 4.0
    out.append(("rule2_pair_open_timestamp_wins", x, [T, 5, T + 10], T + 12))
    x = base(); x[T + 15] = 30.0; x[T + 20] = 29.0; x[T + 25] = 10.0; x[8] = 9.0
    out.append(("rule3_monotonic_after_text", x, [T + 20, 5], T + 25))
    x = base(); x[T + 29] = 20.0; x[T + 30] = 10.0
    out.append(("rule3_monotonic_pair_open_keeps_t_last", x, [T + 20, 5, T + 30], T + 30))
    x = base(); x[3] = 100.0; x[T + 51] = 90.0; x[T + 50] = 1.0; x[T] = 0.5
    out.append(("rule4_first_token", x, [], T + 50))
    x = base(); x[T + 1:T + 101] = 0.0; x[7] = 2.0
    out.append(("rule5_mass_wins_first_of_tied_timestamps", x, [T, 5], T + 1))
    x = base(); x[T + 1:T + 101] = 0.0; x[7] = 6.0
    out.append(("rule5_text_wins", x, [T, 5], 7))
    x = base(-np.inf); x[T + 3] = 2.0; x[7] = 2.0
    out.append(("rule5_strict_equal_then_first_max", x, [T, 5], 7))
    x = base(); x[5] = 3.0; x[9] = 3.0
    out.append(("rule6_exact_tie_text", x, [T, 5], 5))
    x = base(); x[4] = np.nan; x[6] = 1.0; x[T + 2] = np.nan
    out.append(("rule6_nan_is_masked", x, [T, 5], 6))
    out.append(("rule6_all_minus_inf_is_eot", base(-np.inf), [T, 5], E))
    out.append(("rule6_all_nan_is_eot", base(np.nan), [], E))
    x = base(); x[E] = 10.0
    out.append(("rule6_eot", x, [T, 5], E))
    return out
