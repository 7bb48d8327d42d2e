"""Float64 restatement of the repetition rules (DESIGN.md "Repetition rules") on top of the rules references: both edit the raw row
before suppression and rules 2 to 5, from the clip's history `seq`; timestamps and eot are never scaled and never banned.

The bound on a log-probability: the scored kernel's against float64 on the SAME float32 row, 1e-4 + 1e-6 max(|x[c]|, |logsumexp|)
(tests/test_gpu_scores.py), plus the kernel's one float32 rounding of x * p or x / p: at most 2^-24 |x'[c]| on the chosen id and,
logsumexp being monotone with partial derivatives that sum to 1, 2^-24 max |x'[i]| over the finite elements on the logsumexp."""
import math

import numpy as np

import score_reference as sr

def banned(seq, E, g):
    """the ids the n-gram rule bans after `seq`: seq[i + g - 1] < E for every i in [0, n - g] with seq[i : i + g - 1] == the last g - 1"""
    seq = [int(i) for i in seq]
    n = len(seq)
    if g < 2 or n < g:
        return set()
    tail = seq[n - g + 1:]
    return {seq[i + g - 1] for i in range(n - g + 1) if seq[i:i + g - 1] == tail and seq[i + g - 1] < E}


def edit_row(row, seq, E, penalty=1.0, ngram=0, suppress=()):
    """float64 copy of the row after the penalty (each DISTINCT text id of seq once, by sign), the bans and the suppress set"""
    x = np.array(row, dtype=np.float64, copy=True)
    p = float(np.float32(penalty))
    for c in {int(i) for i in seq if 0 <= int(i) < E}:
        x[c] = x[c] * p if x[c] < 0 else x[c] / p
    for c in banned(seq, E, ngram):
        x[c] = -math.inf
    for c in suppress:
        x[c] = -math.inf
    return x


def logprob_bound(x_edited, info):
    """the bar of the module docstring for one decision: info is score_reference.token_logprob's on the edited row"""
    xc, lse = np.nan_to_num(np.abs([info["x_chosen"], info["lse_allowed"]]), posinf=0.0)
    return 1e-4 + 1e-6 * max(xc, lse) + 2.0 ** -24 * (xc + np.abs(x_edited[np.isfinite(x_edited)]).max(initial=0.0))


def decide(row, seq, T, E, penalty=1.0, ngram=0, suppress=(), min_margin=1e-3):
    """(chosen id, float32 log-probability, info + bound) of a scored step under the rules; min_margin: asserted of the decision (the
    rows of the tests keep it this far from a tie)"""
    x = edit_row(row, seq, E, penalty, ngram, suppress)
    c, lp, info = sr.token_logprob(x, seq, T, E)
    assert min_margin is None or info["margin"] >= min_margin, (info["margin"], c)
    return c, lp, dict(info, bound=logprob_bound(x, info), row=x)
