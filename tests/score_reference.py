"""Python restatement of the confidence contract (DESIGN.md "Confidence"): the log-probability of a timestamp-mode decision under
the final allowed set, the no-speech log-probability of the row at decode offset 0, a clip's average, the silent-window rule and
the seek loop under it. Everything is computed in float64 and returned as float32, the type the engine hands out.

The scored rules kernel, the no-speech kernel (whisper.axera_amd/csrc/decode_timestamps.hip), AX_WHISPER_LongWindowIsSilent and
the scored long-form loop are checked against these."""
import math

import numpy as np

import longform_reference as lfr
import ts_reference as tsr


def final_allowed(logits, seq, T, E):
    """bool [nv]: the set A the chosen id is normalised over — rules 1-4 without NaN entries, and without every id below T when
    rule 5 fires."""
    x = np.asarray(logits, dtype=np.float64)
    ok = tsr.allowed(seq, T, E, x.size) & ~np.isnan(x)
    _, info = tsr.decide(logits, seq, T, E)
    if info["rule5"]:
        ok[:T] = False
    return ok


def _logprob(xc, lse):
    if lse == -math.inf or xc == -math.inf:  # nothing finite left (the decision is eot)
        return -math.inf
    if xc == math.inf:
        return 0.0
    return xc - lse


def token_logprob(logits, seq, T, E):
    """(chosen id, float32 log-probability of it, decide()'s info) of one sampled step with history `seq`."""
    x = np.asarray(logits, dtype=np.float64)
    c, info = tsr.decide(logits, seq, T, E)
    A = final_allowed(logits, seq, T, E)
    lse = tsr._lse(x[A])
    xc = float(x[c]) if A[c] else -math.inf  # (eot chosen because nothing finite was left is not in A's finite part)
    return c, np.float32(_logprob(xc, lse)), dict(info, lse_allowed=lse, x_chosen=xc)


def no_speech_logprob(row, no_speech):
    """float32 log p(no_speech) over the WHOLE unfiltered row, NaN entries left out of the normaliser."""
    x = np.asarray(row, dtype=np.float64)
    return np.float32(_logprob(float(x[no_speech]), tsr._lse(x)))


def avg_logprob(token_logprobs, n_ids, ended_eot):
    """openai-whisper's sum_logprobs / (len(tokens) + 1): the kept ids' values, plus the ending decision's when it was eot."""
    lp = np.asarray(token_logprobs, dtype=np.float64)
    s = float(lp[:n_ids].sum()) + (float(lp[n_ids]) if ended_eot else 0.0)
    return np.float32(s / (n_ids + 1))


def is_silent(no_speech_lp, avg_lp, no_speech_threshold, logprob_threshold):
    """The silent-window rule in float32, both comparisons strict."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.exp(f(no_speech_lp)) > f(no_speech_threshold)) and not bool(f(avg_lp) > f(logprob_threshold))


def loop_scored(n_samples, decode, score, T, E, no_speech_threshold, logprob_threshold):
    """longform_reference.loop with a per-window score callback: decode(seek, window_frames) -> ids, score(seek, window_frames)
    -> (no_speech_logprob, avg_logprob). A silent window yields no segment and advances by window_frames.
    Returns [(seek, window_frames, advance, ids, segments, skipped)]."""
    content = n_samples // lfr.HOP
    seek, out = 0, []
    while seek < content:
        wf = min(lfr.WINDOW, content - seek)
        ids = list(decode(seek, wf))
        nsp, avg = score(seek, wf)
        skipped = is_silent(nsp, avg, no_speech_threshold, logprob_threshold)
        if skipped:
            segs, adv = [], wf
        else:
            segs, adv, _ = lfr.split_window(ids, T, E, wf)
        out.append((seek, wf, adv, ids, segs, skipped))
        seek += adv
    return out


def clip_scores(rows, ids, T, E):
    """A clip's record from the rows of its decisions: rows[i] is the row decision i was taken on with history ids[:i]
    (len(rows) == len(ids) + 1; the last decision ended the clip: eot, or an id dropped at the budget / context end).
    Returns dict(token_logprob float32 [len(ids) + 1], ended_eot, avg_logprob, infos)."""
    lps, infos = [], []
    last = E
    for i in range(len(ids) + 1):
        c, lp, info = token_logprob(rows[i], ids[:i], T, E)
        lps.append(lp)
        infos.append(dict(info, chosen=c))
        last = c
    return dict(token_logprob=np.array(lps, dtype=np.float32), ended_eot=bool(last == E), avg_logprob=avg_logprob(lps, len(ids), last == E),
                infos=infos)


def oracle_rows(orc, ck, cv, prefix, ids):
    """The oracle teacher-forced with `ids` behind the prefix [sot, language, transcribe] -> (row of decode offset 0, rows of the
    len(ids) + 1 decisions)."""
    sk, sv = orc.new_self_cache()
    toks = list(prefix) + list(ids)
    row0, rows = None, []
    for s, tok in enumerate(toks):
        lg = orc.decoder_step(tok, s, ck, cv, sk, sv, want_logits=(s == 0 or s >= 2))
        if s == 0:
            row0 = np.array(lg, dtype=np.float32)
        elif s >= 2:
            rows.append(np.array(lg, dtype=np.float32))
    return row0, np.array(rows)
