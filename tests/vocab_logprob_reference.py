"""Float64 reference of the fused vocabulary log-probability kernel (whisper.axera_amd/csrc/vocab_logprob.hip), its per-row error
bound, a numpy emulation of the kernel's rounding, and the inputs of the GPU test (tests/test_gpu_vocab_logprob.py).

Contract: lp[r] = logit[r][id[r]] - logsumexp over columns [0, eot) of logit[r][.], logit = LayerNorm(x) . W^T, W the tied embedding
in the build's 16-bit type, id[r] in [0, eot).

Bound, in the notation of tests/decode_kernel_reference.py (u = 2^-24, hulp(x) = half an ulp of the 16-bit type at |x|, first order,
worst case, fp32 arithmetic in ANY order):
  LayerNorm     y with error E_ln: the two-pass bound ln_expect(..., onepass=False) (layernorm_bf16_kernel: mean, then centred squares).
  fused route   a = rn16(y): ea = E_ln + hulp(|y| + E_ln). Products of two 16-bit values are exact in fp32; d of them and the
                accumulator's additions in fp32: E_logit[c] = |W_c| ea + (d + 9) u |W_c| (|a| + ea)
  rows route    a = y in fp32 (ea = E_ln), every term through one fmaf, the lane reduction, no bias (tests/gemv_kernel_reference.py):
                E_logit[c] = |W_c| ea + gamma |W_c| (|a| + ea), gamma = (d + 7) u / (1 - (d + 7) u)
  logsumexp     L = m + log sum_c e^(x_c - m). An error e_c of x_c moves L by p_c e_c (p = softmax over [0, eot)): sum_c p_c E_logit[c].
                A term's weight passes through one expf of its own and through the rescaling factors of the online fold (a lane's tiles
                of a split, two lane-group steps, three wave steps, the splits of the merge: C of them at most, C = tiles per lane of a
                split + 5 + splits; for the rows route C = 2: one pass over the stored row); their arguments add up to at most
                m - x_c. Per factor, as in the attention derivation of decode_kernel_reference.py: the argument's rounding is worth
                u |arg| in the result, expf 2 u, the multiplication u:   eps_c = u (3 C + 2 (m - x_c)), weighted by p_c.
                The sum of eot positive terms in fp32 in any order: (eot + C) u, relative, i.e. absolute in L. logf within 2 ulp and
                the addition of m: 3 u |L| + 2 u |log s|, bounded by 5 u (|L| + |m|).
                The first-order terms of the exponentials carry a factor 2 for what first order leaves out.
  result        E_lp = E_logit[id] + E_L + u |lp|
"""
import numpy as np

from decode_kernel_reference import ln_expect
from encoder_kernel_reference import U32, hulp, mm64, round16

CHUNK = 256  # columns a workgroup covers per sweep of its row tile (4 waves x 4 tiles of 16)
ROWS = (1, 17, 64, 65, 200)


def plan(d, rows, eot):
    """-> (rows per row tile, vocabulary splits, columns per split): csrc/vocab_logprob_plan.hpp restated"""
    if d < 128 or d % 128 or d > 2048 or rows < 1 or eot < 1:
        raise ValueError("a shape the kernel does not take")
    rt = 64 if d <= 512 else 32 if d <= 1024 else 16
    tiles, chunks = -(-rows // rt), -(-eot // CHUNK)
    s0 = min(-(-1024 // tiles), chunks)
    per = -(-chunks // s0)
    return rt, -(-chunks // per), per * CHUNK


def dtype_of(case_dtype):
    return "f16" if case_dtype == "F16" else "bf16"


def reference(x, g, b, W, ids, eot):
    """float64: dict(lp [R], logits [R][eot], p [R][eot] softmax, m, L [R], y [R][d] LayerNorm output, e_ln its fp32 bound)"""
    x64 = np.asarray(x, dtype=np.float64)
    y, e_ln, _ = ln_expect(x64, np.asarray(g, dtype=np.float32), np.asarray(b, dtype=np.float32), onepass=False)
    W64 = np.asarray(W, dtype=np.float64)[:eot]
    return _from_activations(y, e_ln, W64, ids)


def _from_activations(y, e_ln, W64, ids):
    logits = mm64(y, W64)
    m = logits.max(1)
    e = np.exp(logits - m[:, None])
    s = e.sum(1)
    L = m + np.log(s)
    ids = np.asarray(ids, dtype=np.int64)
    return dict(lp=logits[np.arange(len(ids)), ids] - L, logits=logits, p=e / s[:, None], m=m, L=L, y=y, e_ln=e_ln)


def bound(ref, W, ids, eot, dt, route, n_chain):
    """per-row bound [R] of |lp - reference| for route "fused" or "rows"; n_chain = C of the docstring"""
    W64 = np.abs(np.asarray(W, dtype=np.float64)[:eot])
    d = W64.shape[1]
    y, e_ln = ref["y"], ref["e_ln"]
    if route == "fused":
        ea = e_ln + hulp(np.abs(y) + e_ln, dt)
        gamma = (d + 9) * U32
    else:
        ea = e_ln
        gamma = (d + 7) * U32 / (1 - (d + 7) * U32)
    e_logit = mm64(ea, W64) + gamma * mm64(np.abs(y) + ea, W64)
    p, m, L = ref["p"], ref["m"], ref["L"]
    eps = U32 * (3 * n_chain + 2 * (m[:, None] - ref["logits"]))
    e_L = (p * (e_logit + 2 * eps)).sum(1) + (eot + n_chain) * U32 + 5 * U32 * (np.abs(L) + np.abs(m))
    ids = np.asarray(ids, dtype=np.int64)
    return e_logit[np.arange(len(ids)), ids] + e_L + U32 * np.abs(ref["lp"])


def chain(route, d, rows, eot):
    if route == "rows":
        return 2
    _, n_splits, split_cols = plan(d, rows, eot)
    return 4 * (split_cols // CHUNK) + 5 + n_splits


def emulate(x, g, b, W, ids, eot, dt, variant=None):
    """The fused route's arithmetic in numpy float32: the two-pass LayerNorm in fp32, the row narrowed to the 16-bit type, fp32
    products and sums, a (max, sum) per vocabulary split merged in split order. variant "include_eot": column eot enters the sum;
    "drop_ragged": the columns of the last, ragged 16-column tile are left out (two ways to get the edge wrong)."""
    x = np.asarray(x, dtype=np.float32)
    R, d = x.shape
    mean = (x.sum(1, dtype=np.float32) / np.float32(d))[:, None]
    a = x - mean
    var = (a * a).sum(1, dtype=np.float32) / np.float32(d)
    r = (np.float32(1) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)[:, None]
    y = a * r * np.asarray(g, dtype=np.float32) + np.asarray(b, dtype=np.float32)
    a16 = round16(y, dt)
    hi = eot + 1 if variant == "include_eot" else (eot // 16 * 16 if variant == "drop_ragged" else eot)
    logits = a16 @ np.asarray(W, dtype=np.float32)[:hi].T
    _, n_splits, split_cols = plan(d, R, eot)
    m = np.full(R, -np.inf, dtype=np.float32)
    s = np.zeros(R, dtype=np.float32)
    for sp in range(n_splits):
        part = logits[:, sp * split_cols: min((sp + 1) * split_cols, hi)]
        if part.shape[1] == 0:
            continue
        m2 = part.max(1)
        s2 = np.exp(part - m2[:, None], dtype=np.float32).sum(1, dtype=np.float32)
        mn = np.maximum(m, m2)
        s = s * np.exp(m - mn, dtype=np.float32) + s2 * np.exp(m2 - mn, dtype=np.float32)
        m = mn
    ids = np.asarray(ids, dtype=np.int64)
    tgt = np.where(ids < hi, logits[np.arange(R), np.minimum(ids, hi - 1)], -np.inf).astype(np.float32)
    return (tgt - (m + np.log(s, dtype=np.float32))).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the inputs of the GPU test
def _steer(W64, g, b, col, eot):
    """a row whose LayerNorm output points along W[col] so that column `col` holds more than 0.99 of the softmax over [0, eot] (the
    column itself may be eot: the mass the contract must leave out)"""
    g64 = np.asarray(g, dtype=np.float64)
    gs = np.where(g64 < 0, -1.0, 1.0) * np.maximum(np.abs(g64), 0.5)
    base = W64[col] / gs
    for k in range(40):
        x = (base * 2.0 ** k).astype(np.float32)
        y, _, _ = ln_expect(x[None].astype(np.float64), np.asarray(g, dtype=np.float32), np.asarray(b, dtype=np.float32), onepass=False)
        lg = (W64[: eot + 1] @ y[0])
        e = np.exp(lg - lg.max())
        if e[col] / e.sum() > 0.99:
            return x
    raise AssertionError("no row steers the softmax to column %d" % col)


def case(weights, cfg, rows, seed):
    """-> (x float32 [rows][d], ids int32 [rows], roles {name: row}). Seeded N(0, 3) rows with one outlier channel off channel 0 (as
    decode_kernel_reference.realistic_stream); ids at 0, at eot - 1, in the ragged tile, and at both ends of a vocabulary split of the
    plan for this row count; from 17 rows on: a row whose target dominates, in the ragged tile (lp ~ 0), a zero row (LayerNorm gives
    the bias alone), and a row whose mass sits on column eot, which the sum must leave out."""
    d, eot = int(cfg["n_text_state"]), int(cfg["eot"])
    W64 = np.asarray(weights["decoder.token_embedding.weight"], dtype=np.float64)
    g, b = weights["decoder.ln.weight"], weights["decoder.ln.bias"]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, d)) * 3.0
    oc = int(rng.integers(1, d))
    x[:, oc] += 0.75 * 14.0 * np.sqrt(d) * (1.0 + 0.2 * np.sin(np.arange(rows) / 7.0))
    x = x.astype(np.float32)
    _, n_splits, split_cols = plan(d, rows, eot)
    special = [0, eot - 1, eot // 16 * 16, split_cols - 1, min(split_cols, eot - 1), (n_splits - 1) * split_cols,
               min((n_splits - 1) * split_cols, eot) - 1]
    ids = rng.integers(0, eot, rows).astype(np.int32)
    ids[: min(rows, len(special))] = special[:rows]
    roles = {}
    if rows >= 17:
        roles = dict(dominant=8, zero=9, eot_heavy=10)
        ids[8] = eot // 16 * 16 + (eot % 16) // 2  # inside the ragged tile
        x[8] = _steer(W64, g, b, int(ids[8]), eot)
        x[9] = 0.0
        x[10] = _steer(W64, g, b, eot, eot)
    return x, ids, roles
