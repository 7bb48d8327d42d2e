"""CPU: the host side of word-level timestamps (csrc/words.hpp through AX_WHISPER_AlignPath, AX_WHISPER_SplitWords and
AX_WHISPER_WordsFromAlignment) against tests/word_reference.py. No GPU and no model: the tokens file is
tests/golden/multilingual.tiktoken."""
import os

import numpy as np
import pytest

import word_reference as wr
from conftest import GOLDEN

TABLE_PATH = os.path.join(GOLDEN, "multilingual.tiktoken")
EOT = 50257
SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (64, 65), (65, 64), (130, 750), (445, 1500))


@pytest.fixture(scope="module")
def table():
    return wr.load_table(TABLE_PATH)


def grid_matrix(shape, seed):
    """entries are multiples of 2^-6 in [-8, 8]: every fp32 sum of a path is exact"""
    return (np.random.default_rng(seed).integers(-512, 513, shape) / 64.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------- AlignPath
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_align_path_equals_the_python_dtw(built_lib, shape):
    m = grid_matrix(shape, shape[0] * 10007 + shape[1])
    got = built_lib.align_path(m)
    ref = wr.align_path(m, np.float32)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert got[0] == 0 and np.all(np.diff(got) >= 0) and got[-1] < shape[1]


@pytest.mark.parametrize("shape", ((1, 9), (9, 1), (7, 5), (65, 64), (130, 750)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_align_path_ties_go_left(built_lib, shape):
    """an all-equal matrix and a two-valued one: the tie rule alone decides the path"""
    flat = np.full(shape, 0.5, dtype=np.float32)
    two = np.where(np.random.default_rng(shape[1]).integers(0, 2, shape) == 1, 1.0, -1.0).astype(np.float32)
    for m in (flat, two):
        assert np.array_equal(built_lib.align_path(m), wr.align_path(m, np.float32))
    # all equal: every interior cell has three equal predecessors or a cheaper left one, so the walk back goes left along the last
    # row and then up the first column: every row but the last begins at frame 0
    j = built_lib.align_path(flat)
    assert np.all(j[:-1] == 0) or shape[0] == 1


def test_align_path_refuses_an_empty_matrix(built_lib):
    with pytest.raises((RuntimeError, ValueError)):
        built_lib.align_path(np.zeros((0, 4), dtype=np.float32))


# ---------------------------------------------------------------------------------------------- SplitWords
def ids_of(table, *pieces):
    """the id of every piece (bytes); a piece must be one entry of the table"""
    index = {b: i for i, b in enumerate(table) if b}
    return [index[p] for p in pieces]


def multi_token_cjk(table):
    """a CJK character the table has no single entry for: its UTF-8 bytes as two or three entries"""
    index = {b: i for i, b in enumerate(table) if b}
    for cp in range(0x4E00, 0x9FFF):
        b = chr(cp).encode("utf-8")
        if b not in index and b[:2] in index and b[2:] in index:
            return chr(cp), [index[b[:2]], index[b[2:]]]
    raise AssertionError("every CJK character is one entry")


def test_split_words_crafted_ids(built_lib, table):
    ch, cjk = multi_token_cjk(table)
    ids = ids_of(table, b" Hello", b" wor", b"ld", b",", b" it", b"'s", b" (", b"ok", b")", b".") + cjk + [EOT + 3] + ids_of(table, b" x") + [EOT]
    for lang in ("en", "zh", "ja", "de"):
        got = built_lib.split_words(TABLE_PATH, ids, EOT, lang)
        ref = wr.split_words(table, ids, EOT, lang)
        assert got == ref, lang
    en = built_lib.split_words(TABLE_PATH, ids, EOT, "en")
    words = [w for w, _ in en]
    # a leading space and a lone punctuation mark start words; "'s" and "ok" join the word before them
    # (so does the CJK character, in a language written with spaces)
    assert words[:7] == [b" Hello", b" world", b",", b" it's", b" (ok", b")", b"." + ch.encode("utf-8")]
    zh = built_lib.split_words(TABLE_PATH, ids, EOT, "zh")
    assert len(zh) > len(en)  # zh keeps the unicode groups: " wor" and "ld" stay apart
    assert (ch.encode("utf-8"), cjk) in zh  # the two ids of one character are one group
    assert (b"", [EOT + 3]) in en and en[-1] == (b"", [EOT])  # an id >= eot is a word of its own, without text
    assert sum(len(t) for _, t in en) == len(ids)


def test_split_words_drops_an_unfinished_character(built_lib, table):
    _, cjk = multi_token_cjk(table)
    ids = ids_of(table, b" a") + cjk[:1]
    assert built_lib.split_words(TABLE_PATH, ids, EOT, "en") == wr.split_words(table, ids, EOT, "en") == [(b" a", ids[:1])]


# ---------------------------------------------------------------------------------------------- WordsFromAlignment
def check_words(built_lib, table, ids, lang, seg_tokens, seg_start, seg_end, jump, lp=None, last=0.0):
    lp = np.log(np.linspace(0.3, 0.9, max(len(ids), 1))[: len(ids)]).astype(np.float32) if lp is None else lp
    got, gs, ge = built_lib.words_from_alignment(TABLE_PATH, ids, EOT, lang, seg_tokens, seg_start, seg_end, jump, lp, last)
    ref, rs, re_ = wr.words_from_alignment(table, ids, EOT, lang, seg_tokens, seg_start, seg_end, jump, lp, last)
    assert [(g[0], g[1], g[2], g[3]) for g in got] == [(r[0], r[1], r[2], r[3]) for r in ref]
    # the mean of exp(float32 log-probability) in float64, narrowed to float32: two libms' exp differ by an ulp of float64 at most
    assert np.allclose([g[4] for g in got], [r[4] for r in ref], rtol=2e-7, atol=0)
    assert list(gs) == list(rs) and list(ge) == list(re_)
    return got, list(gs), list(ge)


def test_words_both_merge_sweeps(built_lib, table):
    ids = ids_of(table, b" He", b" said", b" \"", b" hi", b" there", b",", b" (", b" yes", b")", b".")
    jump = [0, 10, 20, 25, 30, 40, 50, 55, 60, 70, 75]
    got, _, _ = check_words(built_lib, table, ids, "en", [len(ids)], [0.0], [1.5], jump)
    words = [g[1] for g in got]
    assert words == [b" He", b" said", b" \" hi", b" there,", b" ( yes)."]  # prepended onto the next word, appended onto the one before
    # times are not merged: ' " hi' keeps the times of ' hi', ' there,' those of ' there'
    assert (got[2][2], got[2][3]) == (0.5, 0.6) and (got[3][2], got[3][3]) == (0.6, 0.8)


def test_words_long_word_at_and_after_a_sentence_end(built_lib, table):
    ids = ids_of(table, b" One", b" two", b".", b" Three", b" four", b"?", b" five")
    #        One   two   .     Three  four  ?     five   eot
    jump = [0, 10, 20, 120, 320, 330, 340, 440]
    got, _, _ = check_words(built_lib, table, ids, "en", [len(ids)], [0.0], [8.8], jump)
    by = {g[1]: g for g in got}
    assert by[b" two."][3] == 0.4  # merged text, the times of ' two' itself
    # the median duration is 0.2 s, so max_duration 0.4 s: '.' (2 s long) is cut to 0.4 s before it is merged away, and ' Three'
    # (4 s long, behind a sentence end) starts at its end - 0.4 s
    assert (by[b" Three"][2], by[b" Three"][3]) == (6.0, 6.4)


def test_words_pause_rule_and_segment_boundaries(built_lib, table):
    ids = ids_of(table, b" a", b" b", b" c", b" d", b" e", b" f")
    # segment 0: a first word after a pause that is far too long, and a long second word; segment 1: a last word that overshoots
    jump = [0, 200, 400, 410, 420, 430, 700]
    for last in (0.0, 7.9):
        got, ss, se = check_words(built_lib, table, ids, "en", [3, 3], [3.0, 8.4], [8.4, 9.0], jump, last=last)
    got, ss, se = check_words(built_lib, table, ids, "en", [3, 3], [3.0, 8.4], [8.4, 9.0], jump)
    assert [g[0] for g in got] == [0, 0, 0, 1, 1, 1]
    # median 0.7 s (capped), max_duration 1.4 s. ' a' ends 4 s after the last speech and is 4 s long, ' b' too: they meet at
    # max(8 / 2, 8 - 1.4) and ' a' keeps 1.4 s
    assert (got[0][2], got[0][3], got[1][2]) == (pytest.approx(5.2), 6.6, 6.6)
    assert ss[0] == got[0][2] and se[0] == 8.2  # the segment follows its first and its last word
    # ' f' runs 5 s past its segment's end: start + median, and the segment keeps its end
    assert got[-1][3] == pytest.approx(9.3) and se[1] == 9.0


def test_words_prefer_the_segment_start(built_lib, table):
    ids = ids_of(table, b" a", b" b", b" c")
    got, ss, _ = check_words(built_lib, table, ids, "en", [3], [2.0], [2.8], [0, 120, 130, 140], last=2.0)
    assert got[0][2] == 2.0 and ss[0] == 2.0  # a first word that begins 2 s before its segment is moved to the segment's start


def test_words_zero_durations_and_a_segment_without_text(built_lib, table):
    ids = ids_of(table, b" a", b" b", b" c", b" d")
    jump = [0, 0, 0, 30, 30]  # ' a' and ' b' have no duration: they do not enter the median
    got, ss, se = check_words(built_lib, table, ids, "en", [2, 0, 2], [0.0, 0.5, 0.6], [0.5, 0.6, 1.0], jump)
    assert [g[0] for g in got] == [0, 0, 2, 2]
    assert (ss[1], se[1]) == (0.5, 0.6)  # untouched
    # no ids at all, and no segments at all
    assert check_words(built_lib, table, [], "en", [0], [0.0], [1.0], [0])[0] == []
    assert check_words(built_lib, table, [], "en", [], [], [], [0])[0] == []


def test_words_zh_groups_and_fullwidth_marks(built_lib, table):
    ch, cjk = multi_token_cjk(table)
    index = {b: i for i, b in enumerate(table) if b}
    single = [index[c.encode("utf-8")] for c in "你好" if c.encode("utf-8") in index]
    mark = index.get("。".encode("utf-8"))
    ids = single + cjk + ([mark] if mark is not None else [])
    jump = list(range(0, 10 * (len(ids) + 1), 10))
    got, _, _ = check_words(built_lib, table, ids, "zh", [len(ids)], [0.0], [2.0], jump)
    assert any(ch.encode("utf-8") in g[1] for g in got)


def test_words_survive_an_unfinished_last_character(built_lib, table):
    """ids that end inside a character (a decode cut at the context limit): the unfinished group takes the closing eot with it
    and is dropped; the words in front of it stay, a single one too"""
    _, cjk = multi_token_cjk(table)
    for pieces in ((b" a",), (b" a", b" b")):
        ids = ids_of(table, *pieces) + cjk[:1]
        jump = list(range(0, 10 * (len(ids) + 1), 10))
        got, _, _ = check_words(built_lib, table, ids, "en", [len(ids)], [0.0], [1.0], jump)
        assert [g[1] for g in got] == list(pieces)
        got, _, _ = check_words(built_lib, table, ids, "zh", [len(ids)], [0.0], [1.0], jump)
        assert [g[1] for g in got] == list(pieces)


# ---------------------------------------------------------------------------------------------- alignment heads of a config file
def _config(tmp_path, heads, n_layer=4, n_state=384):
    import json

    cfg = {"n_text_layer": n_layer, "n_text_state": n_state, "n_text_head": n_state // 64}
    if heads is not None:
        cfg["alignment_heads"] = heads
    f = tmp_path / "x_config.json"
    f.write_text(json.dumps(cfg))
    return str(f)


def test_config_alignment_heads(built_lib, tmp_path):
    """the optional key of {type}_config.json: the handle's list; without it every head of the upper half of the layers"""
    assert built_lib.config_alignment_heads(_config(tmp_path, None)) == [(l, h) for l in (2, 3) for h in range(6)]
    assert built_lib.config_alignment_heads(_config(tmp_path, [])) == [(l, h) for l in (2, 3) for h in range(6)]
    assert built_lib.config_alignment_heads(_config(tmp_path, [[3, 1], [2, 5], [2, 0]])) == [(2, 0), (2, 5), (3, 1)]  # sorted
    assert built_lib.config_alignment_heads(_config(tmp_path, None, n_layer=5)) == [(l, h) for l in (3, 4) for h in range(6)]
    for bad in ([[4, 0]], [[0, 6]], [[-1, 0]], [[1, 1], [1, 1]], [[1]], [1, 2], "x", [[1, "2"]]):
        with pytest.raises(RuntimeError):
            built_lib.config_alignment_heads(_config(tmp_path, bad))


def test_convert_weights_copies_the_alignment_heads(built_lib, tmp_path):
    """tools/convert_weights.py --hf: generation_config.json's alignment_heads arrive in the model's config file, and the engine's
    reader takes them from there"""
    import json

    import convert_weights
    import modelgen

    hf = tmp_path / "hf"
    hf.mkdir()
    assert convert_weights.hf_alignment_heads(str(hf)) is None  # no generation_config.json
    (hf / "generation_config.json").write_text(json.dumps({"max_length": 448}))
    assert convert_weights.hf_alignment_heads(str(hf)) is None  # no key
    (hf / "generation_config.json").write_text(json.dumps({"alignment_heads": [[1, 0], [1, 1], [0, 1]]}))
    assert convert_weights.hf_alignment_heads(str(hf)) == [[1, 0], [1, 1], [0, 1]]
    assert convert_weights.hf_alignment_heads(str(hf / "model.safetensors")) == [[1, 0], [1, 1], [0, 1]]  # beside a weights file
    dims = modelgen.DIMS["micro"]
    d = convert_weights.write_model(modelgen.synth_weights(dims, 3), "micro", str(tmp_path / "m"), "BF16", TABLE_PATH,
                                    alignment_heads=convert_weights.hf_alignment_heads(str(hf)))
    cfg = json.load(open(os.path.join(d, "micro_config.json")))
    assert cfg["alignment_heads"] == [[1, 0], [1, 1], [0, 1]]
    assert built_lib.config_alignment_heads(os.path.join(d, "micro_config.json")) == [(0, 1), (1, 0), (1, 1)]
    d = convert_weights.write_model(modelgen.synth_weights(dims, 3), "micro", str(tmp_path / "n"), "BF16", TABLE_PATH)
    assert "alignment_heads" not in json.load(open(os.path.join(d, "micro_config.json")))
    (hf / "generation_config.json").write_text(json.dumps({"alignment_heads": [[1, 0, 2]]}))
    with pytest.raises(ValueError):
        convert_weights.hf_alignment_heads(str(hf))


def test_words_refuse_bad_arguments(built_lib, table):
    ids = ids_of(table, b" a", b" b")
    with pytest.raises(RuntimeError):
        built_lib.words_from_alignment(TABLE_PATH, ids, EOT, "en", [1], [0.0], [1.0], [0, 1, 2], [0.0, 0.0])  # counts do not add up
    with pytest.raises(RuntimeError):
        built_lib.words_from_alignment(TABLE_PATH, [EOT], EOT, "en", [1], [0.0], [1.0], [0, 1], [0.0])  # not a text id


def test_admissibility_is_a_property_of_the_matrix():
    """what tests/test_gpu_words.py relies on: a matrix with a clear diagonal is admissible at a small amplitude, a flat one is not"""
    n, F = 6, 40
    m = np.full((n + 5, F), -1.0)
    for i in range(n + 1):
        m[3 + i, 5 * i: 5 * i + 5] = 2.0
    assert wr.admissible(m, n, 1e-3)
    assert not wr.admissible(np.zeros((n + 5, F)), n, 1e-3)
