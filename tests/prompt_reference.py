"""Python restatement of prompt conditioning (DESIGN.md "Prompt conditioning"): the prompted context, the timestamp-mode greedy loop
behind a context of any length on the oracle, the window ranges the carry appends, and the carry rule itself.

The engine (whisper.axera_amd/csrc/engine_prefill.cpp, decode_prefill.hip, engine_long.cpp) and AX_WHISPER_CarryPrompt are checked
against these."""
import numpy as np

import ts_reference as tsr

KEEP = 223  # n_text_ctx / 2 - 1: the ids of a prompt the decoder takes (its last ones)
MARGIN = 2e-3  # the oracle decision margin a prompt case must have over its first decisions
LENGTHS = (1, 60, 61, 62, 124, 125, 126, 223)  # P: L = P + 3 on both sides of every 64-key block edge
MODELS = (("micro", 11, "BF16"), ("miniturbo", 21, "F16"))
N_DECISIONS = 12


def context(cfg, prompt, prefix):
    """[sot_prev, the last KEEP prompt ids, sot, language, transcribe]; an empty prompt: the bare prefix (no sot_prev either)."""
    prompt = [int(t) for t in prompt][-KEEP:]
    return ([int(cfg["sot_prev"])] + prompt if prompt else []) + [int(t) for t in prefix[:3]]


def greedy_prompted(orc, ck, cv, ctx, max_new=0, want_logits=False, want_cache=False):
    """ts_reference.greedy_ts with a prefix of any length: every id of ctx is fed at its position, a decision is made at every step
    from the one that fed ctx[-1] on; a clip stops at eot, at the context end or at its budget.
    Returns (ids, infos[, logits rows][, (self_k, self_v, row of the step that fed ctx[-3], the sot position)])."""
    cfg = orc.cfg
    T, E, n_ctx = int(cfg["no_timestamps"]) + 1, int(cfg["eot"]), int(cfg["n_text_ctx"])
    L = len(ctx) - 1  # position of transcribe
    if max_new <= 0 or max_new > n_ctx - 1 - L:
        max_new = n_ctx - 1 - L
    sk, sv = orc.new_self_cache()
    ids, infos, rows, sot_row = [], [], [], None
    tok = ctx[0]
    for s in range(n_ctx):
        lg = orc.decoder_step(tok, s, ck, cv, sk, sv, want_logits=s >= L or (want_cache and s == L - 2))
        if s == L - 2 and want_cache:
            sot_row = lg.copy()
        if s < L:
            tok = ctx[s + 1]
            continue
        c, info = tsr.decide(lg, ids, T, E)
        infos.append(info)
        if want_logits:
            rows.append(lg.copy())
        if c == E or s + 1 >= n_ctx or len(ids) >= max_new:
            break
        ids.append(c)
        tok = c
    out = (ids, infos)
    if want_logits:
        out += (np.array(rows),)
    if want_cache:
        out += ((sk, sv, sot_row),)
    return out


def case_prompt(eot, P, sd):
    return np.random.default_rng(1000 * P + sd).integers(0, eot, P).tolist()


def find_case(orc, ck, cv, prefix, P, max_sd=16):
    """The lowest seed whose prompt gives the oracle a decision margin of at least MARGIN over its first N_DECISIONS decisions ->
    (sd, prompt, ids, infos)."""
    for sd in range(max_sd):
        prompt = case_prompt(int(orc.cfg["eot"]), P, sd)
        ids, infos = greedy_prompted(orc, ck, cv, context(orc.cfg, prompt, prefix), max_new=N_DECISIONS)
        if min(i["margin"] for i in infos[:N_DECISIONS]) >= MARGIN:
            return sd, prompt, ids, infos
    raise AssertionError(f"no prompt of length {P} with margin {MARGIN} among {max_sd} seeds")


def segment_ranges(ids, T, E):
    """The id ranges [lo, hi) of the segments the window rule emits, from each segment's opening timestamp to its closing one
    (longform.hpp split_window, restated): consecutive timestamps close segments, ids after the last closed pair are dropped unless
    the ids end in a single timestamp, without any pair the whole window is one segment; a range without a text id is not emitted."""
    ids = list(ids)
    n = len(ids)
    ts = lambda i: ids[i] >= T
    cuts = [i for i in range(1, n) if ts(i - 1) and ts(i)]
    if cuts:
        if n >= 2 and ts(n - 1) and not ts(n - 2):
            cuts.append(n)
        bounds, lo = [], 0
        for hi in cuts:
            bounds.append((lo, hi))
            lo = hi
    else:
        bounds = [(0, n)]
    return [(lo, hi) for lo, hi in bounds if any(t < E for t in ids[lo:hi])]


def carry(all_ids, reset_since, window_ids, T, E, skipped=False, condition_on_previous_text=True, temperature=0.0):
    """One step of the carry rule after a kept window -> (all_ids, reset_since). The next prompt is all_ids[reset_since:][-KEEP:]."""
    all_ids = list(all_ids)
    if not skipped:
        for lo, hi in segment_ranges(window_ids, T, E):
            all_ids += list(window_ids[lo:hi])
    if not condition_on_previous_text or np.float32(temperature) > np.float32(0.5):
        reset_since = len(all_ids)
    return all_ids, reset_since


def window_prompt(all_ids, reset_since):
    return list(all_ids[reset_since:])[-KEEP:]
