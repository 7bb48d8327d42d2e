"""Word-level timestamps, stated in float64 numpy (DESIGN.md "Word-level timestamps"): openai-whisper timing.py's find_alignment,
the word split of its tokenizer, merge_punctuations and add_word_timestamps for one window, plus the teacher-forced decoder
forward the alignment needs (the oracle exposes neither cross-attention weights nor per-layer residuals).

Where the set notation of the rules matters this file follows the project's statement of them: "is one ASCII punctuation
character", "is in the prepended / appended set" and "is a sentence-end mark" are tests of ONE character (openai-whisper tests
substrings of a string, which also accepts the empty string and runs such as "()")."""
import math
import string

import numpy as np

# The engine's matrix against the float64 one, and its token log-probabilities against the float64 ones, per model of MODELS below:
# twice the worst error measured on an MI355X over seeds 0 .. 7 of case_ids, on both clips of tests/test_gpu_words.py. The pass
# narrows its activations to 16 bits, so the bfloat16 build (micro) is an order of magnitude behind the half build (miniturbo).
# Measured over those 8 seeds: matrix 1.85e-2 (micro bf16), 2.03e-3 (miniturbo fp16) on entries of magnitude up to 3.4;
# log-probabilities 7.03e-2 and 1.04e-2. Over all MAX_SEEDS = 16 seeds the test runs: matrix 2.19e-2 and 2.34e-3, the
# log-probabilities unchanged (DESIGN.md "Word-level timestamps"); the constants stay at twice the 8-seed figures.
MATRIX_EPS = {"micro": 3.7e-2, "miniturbo": 4.1e-3}
LOGPROB_EPS = {"micro": 1.41e-1, "miniturbo": 2.1e-2}

NO_SPACE_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")
PREPENDED = "\"'“¿([{-"
APPENDED = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END = ".。!！?？"


# ---------------------------------------------------------------------------------------------- the decoder, teacher-forced
def _erf(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def _ln(x, w, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * w + b


def _softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def decoder_forward(cfg, weights, ck, cv, ctx):
    """All rows of the context `ctx` through the decoder in float64. ck, cv: [n_text_layer][n_audio_ctx][d] (the oracle's, or an
    engine's own cross cache). Returns (logits [L][n_vocab], cross-attention queries [n_layer][L][d])."""
    W = lambda k: np.asarray(weights[k], dtype=np.float64)
    d, H, nl = int(cfg["n_text_state"]), int(cfg["n_text_head"]), int(cfg["n_text_layer"])
    dh = d // H
    L = len(ctx)
    x = W("decoder.token_embedding.weight")[np.asarray(ctx)] + W("decoder.positional_embedding")[:L]
    causal = np.triu(np.full((L, L), -np.inf), 1)
    queries = np.zeros((nl, L, d))

    def heads(a):
        return a.reshape(a.shape[0], H, dh).transpose(1, 0, 2)

    def attend(q, k, v, mask):
        s = heads(q) @ heads(k).transpose(0, 2, 1) / math.sqrt(dh)
        if mask is not None:
            s = s + mask
        return (_softmax(s) @ heads(v)).transpose(1, 0, 2).reshape(q.shape[0], d)

    for l in range(nl):
        p = f"decoder.blocks.{l}."
        h = _ln(x, W(p + "attn_ln.weight"), W(p + "attn_ln.bias"))
        q = h @ W(p + "attn.query.weight").T + W(p + "attn.query.bias")
        k = h @ W(p + "attn.key.weight").T
        v = h @ W(p + "attn.value.weight").T + W(p + "attn.value.bias")
        x = x + attend(q, k, v, causal) @ W(p + "attn.out.weight").T + W(p + "attn.out.bias")
        h = _ln(x, W(p + "cross_attn_ln.weight"), W(p + "cross_attn_ln.bias"))
        q = h @ W(p + "cross_attn.query.weight").T + W(p + "cross_attn.query.bias")
        queries[l] = q
        x = x + attend(q, np.asarray(ck[l], dtype=np.float64), np.asarray(cv[l], dtype=np.float64), None) @ W(p + "cross_attn.out.weight").T \
            + W(p + "cross_attn.out.bias")
        h = _ln(x, W(p + "mlp_ln.weight"), W(p + "mlp_ln.bias"))
        h = h @ W(p + "mlp.0.weight").T + W(p + "mlp.0.bias")
        h = 0.5 * h * (1.0 + _erf(h / math.sqrt(2.0)))
        x = x + h @ W(p + "mlp.2.weight").T + W(p + "mlp.2.bias")
    x = _ln(x, W("decoder.ln.weight"), W("decoder.ln.bias"))
    return x @ W("decoder.token_embedding.weight").T, queries


# ---------------------------------------------------------------------------------------------- find_alignment
def default_heads(cfg):
    nl, H = int(cfg["n_text_layer"]), int(cfg["n_text_head"])
    return [(l, h) for l in range(nl) if 2 * l >= nl for h in range(H)]


def head_softmax(q, k, F):
    """q [L][64], k [>= F][64] -> softmax over keys [0, F) of q . k / 8"""
    return _softmax(np.asarray(q, dtype=np.float64) @ np.asarray(k[:F], dtype=np.float64).T / 8.0)


def median7(z):
    """width 7 along the last axis, reflect padding of 3; skipped when there are no more than 3 frames"""
    if z.shape[-1] <= 3:
        return z
    p = np.pad(z, [(0, 0)] * (z.ndim - 1) + [(3, 3)], mode="reflect")
    win = np.stack([p[..., k: k + z.shape[-1]] for k in range(7)], axis=-1)
    return np.sort(win, axis=-1)[..., 3]


def normalize(P):
    """P [heads][L][F] -> per head and frame the z-score over ALL L rows (population std), then the median filter"""
    mean = P.mean(axis=-2, keepdims=True)
    std = np.sqrt(((P - mean) ** 2).mean(axis=-2, keepdims=True))
    return median7((P - mean) / std)


def dtw(x, dtype=np.float32):
    """openai-whisper's dtw_cpu on x [N][F] (the cost, i.e. -matrix), accumulated in `dtype` -> trace [(N + 1)][(F + 1)]"""
    N, F = x.shape
    x = x.astype(dtype)
    cost = np.full((N + 1, F + 1), np.inf, dtype=dtype)
    trace = np.full((N + 1, F + 1), 2, dtype=np.uint8)
    cost[0, 0] = 0
    for i in range(1, N + 1):
        ci, cp, xi, ti = cost[i], cost[i - 1], x[i - 1], trace[i]
        for j in range(1, F + 1):
            c0, c1, c2 = cp[j - 1], cp[j], ci[j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            ci[j] = xi[j - 1] + c
            ti[j] = t
    return trace


def jumps_of(trace):
    """backtrace from (N, F); jump[i] = the frame of the first path point of row i"""
    N, F = trace.shape[0] - 1, trace.shape[1] - 1
    jump = np.zeros(N, dtype=np.int32)
    i, j = N, F
    while i > 0 or j > 0:
        if i >= 1 and j >= 1:
            jump[i - 1] = j - 1
        t = 2 if i == 0 else 1 if j == 0 else trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return jump


def align_path(matrix, dtype=np.float32):
    """matrix [N][F] -> jump [N]: DTW on -matrix"""
    return jumps_of(dtw(-np.asarray(matrix, dtype=dtype), dtype))


def context(cfg, text_ids, lang_tok, task_tok=None):
    return [int(cfg["sot"]), int(lang_tok), int(cfg["transcribe"] if task_tok is None else task_tok), int(cfg["no_timestamps"])] \
        + [int(t) for t in text_ids] + [int(cfg["eot"])]


def find_alignment(cfg, weights, ck, cv, text_ids, num_frames, lang_tok, heads=None, dtype=np.float64):
    """-> dict(matrix [L][F], jump [n + 1], token_logprob [n], logits [L][n_vocab]); n == 0: None"""
    n = len(text_ids)
    if n == 0:
        return None
    L = n + 5
    if L > int(cfg["n_text_ctx"]):
        raise ValueError("the context exceeds n_text_ctx")
    F = num_frames // 2
    heads = default_heads(cfg) if heads is None else heads
    logits, q = decoder_forward(cfg, weights, ck, cv, context(cfg, text_ids, lang_tok))
    P = np.stack([head_softmax(q[l][:, 64 * h: 64 * h + 64], np.asarray(ck[l])[:, 64 * h: 64 * h + 64], F) for l, h in heads])
    matrix = normalize(P).mean(axis=0)
    eot = int(cfg["eot"])
    rows = logits[3: L - 2, :eot]
    lse = rows.max(-1) + np.log(np.exp(rows - rows.max(-1, keepdims=True)).sum(-1))
    lp = rows[np.arange(n), np.asarray(text_ids)] - lse
    return dict(matrix=matrix, jump=align_path(matrix[3: L - 1], dtype), token_logprob=lp, logits=logits)


def admissible(matrix, n, eps, seeds=8):
    """the float64 jumps of matrix[3 : n + 4] are unchanged under `seeds` perturbations by uniform noise of amplitude eps"""
    X = matrix[3: n + 4]
    ref = align_path(X, np.float64)
    for sd in range(seeds):
        noise = np.random.default_rng(1000 + sd).uniform(-eps, eps, X.shape)
        if not np.array_equal(align_path(X + noise, np.float64), ref):
            return False
    return True


# ---------------------------------------------------------------------------------------------- words
def load_table(path):
    """a .tiktoken / tokens file -> [bytes] by id; an entry ends at its first NUL byte, as the engine's table does"""
    import base64

    out = []
    for line in open(path, "rb").read().splitlines():
        b = base64.b64decode(line.split()[0]) if line.strip() else b""
        out.append(b.split(b"\0")[0])
    return out


def token_bytes(table, t, eot):
    return table[t] if 0 <= t < eot and t < len(table) else b""


def _utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def split_words(table, ids, eot, language):
    """-> [(bytes, [ids])]: the unicode split, and for a language written with spaces the merge into words"""
    groups, cur_b, cur_t = [], b"", []
    for t in ids:
        cur_t.append(int(t))
        cur_b += token_bytes(table, t, eot)
        if _utf8(cur_b):
            groups.append((cur_b, cur_t))
            cur_b, cur_t = b"", []
    if language in NO_SPACE_LANGUAGES:
        return groups
    words = []
    for b, toks in groups:
        s = b.decode("utf-8")
        st = s.strip()
        if toks[0] >= eot or s.startswith(" ") or (len(st) == 1 and st in string.punctuation) or not words:
            words.append((b, list(toks)))
        else:
            words[-1] = (words[-1][0] + b, words[-1][1] + list(toks))
    return words


def _one(s, chars):
    return len(s) == 1 and s in chars


def merge_punctuations(al):
    """al: list of dicts word (str), tokens, start, end, probability; text and tokens move, times do not"""
    i, j = len(al) - 2, len(al) - 1
    while i >= 0:
        prev, nxt = al[i], al[j]
        if prev["word"].startswith(" ") and _one(prev["word"].strip(), PREPENDED):
            nxt["word"] = prev["word"] + nxt["word"]
            nxt["tokens"] = prev["tokens"] + nxt["tokens"]
            prev["word"], prev["tokens"] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(al):
        prev, nxt = al[i], al[j]
        if not prev["word"].endswith(" ") and _one(nxt["word"], APPENDED):
            prev["word"] = prev["word"] + nxt["word"]
            prev["tokens"] = prev["tokens"] + nxt["tokens"]
            nxt["word"], nxt["tokens"] = "", []
        else:
            i = j
        j += 1


def words_from_alignment(table, ids, eot, language, seg_tokens, seg_start, seg_end, jump, token_logprob, last_speech_timestamp=0.0):
    """-> ([(segment, word bytes, start, end, probability)], seg_start, seg_end after the rule): find_alignment's words from the
    path and add_word_timestamps of one window"""
    seg_start, seg_end = [float(x) for x in seg_start], [float(x) for x in seg_end]
    if len(seg_tokens) == 0:
        return [], seg_start, seg_end
    ids = [int(t) for t in ids]
    al = []
    if ids:
        words = split_words(table, ids + [eot], eot, language)
        # the eot pseudo-word closes the list unless the ids end in an unfinished character: that group swallows eot and is dropped
        if words and words[-1][1][0] == eot:
            words = words[:-1]
        if words:
            b = 0
            for wb, toks in words:
                e = b + len(toks)
                probs = np.exp(np.asarray(token_logprob[b:e], dtype=np.float32).astype(np.float64))
                al.append(dict(word=wb.decode("utf-8"), tokens=toks, start=int(jump[b]) / 50.0, end=int(jump[e]) / 50.0, probability=float(np.mean(probs))))
                b = e
    dur = np.array([t["end"] - t["start"] for t in al])
    dur = dur[dur.nonzero()]
    median = min(0.7, float(np.median(dur)) if len(dur) else 0.0)
    max_duration = median * 2
    if len(dur):
        for i in range(1, len(al)):
            if al[i]["end"] - al[i]["start"] > max_duration:
                if _one(al[i]["word"], SENTENCE_END):
                    al[i]["end"] = al[i]["start"] + max_duration
                elif _one(al[i - 1]["word"], SENTENCE_END):
                    al[i]["start"] = al[i]["end"] - max_duration
    merge_punctuations(al)
    out, wi = [], 0
    for s, n_tok in enumerate(seg_tokens):
        saved, words = 0, []
        while wi < len(al) and saved < n_tok:
            t = al[wi]
            if t["word"]:
                words.append(dict(word=t["word"], start=round(t["start"], 2), end=round(t["end"], 2), probability=t["probability"]))
            saved += len(t["tokens"])
            wi += 1
        if words:
            if words[0]["end"] - last_speech_timestamp > median * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            if seg_start[s] < words[0]["end"] and seg_start[s] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median, seg_start[s]))
            else:
                seg_start[s] = words[0]["start"]
            if seg_end[s] > words[-1]["start"] and seg_end[s] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median, seg_end[s])
            else:
                seg_end[s] = words[-1]["end"]
            last_speech_timestamp = seg_end[s]
        out += [(s, w["word"].encode("utf-8"), float(w["start"]), float(w["end"]), w["probability"]) for w in words]
    return out, seg_start, seg_end


# ---------------------------------------------------------------------------------------------- the cases of the GPU word tests
# Seeded N(0, 0.02) weights give cross-attention that is flat to within 1e-6 of 1 / F: the z-scores of such a matrix are the
# 16-bit rounding of the activations and nothing else, and no path over them is stable. The word tests therefore run on
# modelgen.realistic_weights, whose heads include peaked and saturated ones.
MODELS = (("micro", 11, "BF16"), ("miniturbo", 21, "F16"))
N_TEXT = 14          # text ids of a case
MAX_SEEDS = 16


def case_ids(eot, seed, n=N_TEXT):
    return [int(t) for t in np.random.default_rng(4242 + seed).integers(0, eot, n)]


def find_case(cfg, weights, ck, cv, num_frames, lang_tok, eps, max_seeds=MAX_SEEDS):
    """the first seed whose float64 matrix is admissible at eps -> (seed, ids, reference) or None"""
    for sd in range(max_seeds):
        ids = case_ids(int(cfg["eot"]), sd)
        ref = find_alignment(cfg, weights, ck, cv, ids, num_frames, lang_tok)
        if admissible(ref["matrix"], len(ids), eps):
            return sd, ids, ref
    return None
