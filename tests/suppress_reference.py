"""Python restatement of the token-suppression contract (DESIGN.md "Token suppression"): byte-level BPE over one piece, the list
that openai-whisper's suppress_tokens = -1 stands for, which ids a suppress set may hold, the layout of the mask the rules kernels
read, and what suppression means for a row: the ids of the set hold -inf before any rule looks.

csrc/suppress.hpp (through AX_WHISPER_NonSpeechTokens, AX_WHISPER_ConfigSuppressTokens and AX_WHISPER_SetSuppressTokens) and the
rules kernels under a set are checked against these."""
import base64

import numpy as np

SYMBOLS = list('"#()*+/:;<=>@[\\]^_`{|}~「」『』') + \
    "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split()
MUSIC = list("♩♪♫♬♭♮♯")


def load_ranks(path):
    """{bytes: rank} of a tokens file of "<base64> <rank>" lines (tests/golden/multilingual.tiktoken, {type}-tokens.txt)"""
    ranks = {}
    with open(path) as f:
        for line in f:
            if line.strip():
                tok, rank = line.split()
                ranks.setdefault(base64.b64decode(tok), int(rank))
    return ranks


def bpe_one_piece(ranks, piece: bytes):
    """The ids of ONE piece of the GPT-2 split: single bytes, then the adjacent pair whose concatenation has the lowest rank is
    merged (the leftmost of equal ranks) until no pair has one. KeyError where a part has no rank."""
    parts = [bytes([b]) for b in piece]
    while len(parts) > 1:
        cands = [(ranks[parts[i] + parts[i + 1]], i) for i in range(len(parts) - 1) if parts[i] + parts[i + 1] in ranks]
        if not cands:
            break
        _, i = min(cands)
        parts[i:i + 2] = [parts[i] + parts[i + 1]]
    return [ranks[p] for p in parts]


def non_speech_tokens(ranks):
    """openai-whisper's Tokenizer.non_speech_tokens. Every string encoded here is a single piece under the GPT-2 pattern: an optional
    space followed by characters that are neither letters, digits nor white space."""
    enc = lambda s: bpe_one_piece(ranks, s.encode("utf-8"))
    out = {enc(" -")[0], enc(" '")[0]}
    for sym in SYMBOLS + MUSIC:
        for ids in (enc(sym), enc(" " + sym)):
            if len(ids) == 1 or sym in MUSIC:
                out.add(ids[0])
    return sorted(out)


def check_ids(ids, n_vocab, eot, ts_begin):
    """The validity rule: the sorted set, or ValueError. Ids of (eot, ts_begin) are accepted (and have no effect)."""
    ids = [int(i) for i in ids]
    if len(ids) > n_vocab:
        raise ValueError("more entries than the vocabulary has ids")
    for i in ids:
        if i < 0 or i >= n_vocab:
            raise ValueError(f"id {i} outside the vocabulary")
        if i == eot:
            raise ValueError("eot cannot be suppressed")
        if i >= ts_begin:
            raise ValueError(f"timestamp id {i} cannot be suppressed")
    return sorted(set(ids))


def mask_words(ids, n_vocab, eot):
    """uint32 words of the device mask: bit i & 31 of word i >> 5 set iff id i < eot is in the set; whole groups of four words"""
    m = np.zeros((n_vocab + 127) // 128 * 4, dtype=np.uint32)
    for i in ids:
        if 0 <= i < eot:
            m[i >> 5] |= np.uint32(1 << (i & 31))
    return m


def suppress_rows(rows, ids):
    """a copy of the rows with -inf at the ids of the set"""
    out = np.array(rows, dtype=np.float32, copy=True)
    if len(ids):
        out[..., np.asarray(sorted(set(int(i) for i in ids)), dtype=np.int64)] = -np.inf
    return out
