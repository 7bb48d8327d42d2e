"""CPU: the host rules of long-form word timestamps (csrc/longform.hpp long_word_advance and csrc/words.hpp words_from_alignment with
a time offset, through AX_WHISPER_LongWordAdvance and AX_WHISPER_WordsFromAlignmentAt) against tests/long_words_reference.py on
hand-built windows. No GPU and no model: the tokens file is tests/golden/multilingual.tiktoken."""
import os

import numpy as np
import pytest

import long_words_reference as lw
import word_reference as wr
from conftest import GOLDEN

TABLE_PATH = os.path.join(GOLDEN, "multilingual.tiktoken")
EOT = 50257
T = 50364  # <|0.00|> of the multilingual vocabulary


@pytest.fixture(scope="module")
def table():
    return wr.load_table(TABLE_PATH)


def ids_of(table, *pieces):
    index = {b: i for i, b in enumerate(table) if b}
    return [index[p] for p in pieces]


def both(built_lib, ids, seek, window_frames, split_advance, last_word_end):
    got = built_lib.long_word_advance(ids, T, seek, window_frames, split_advance, last_word_end)
    assert got == lw.long_word_advance(ids, T, seek, window_frames, split_advance, last_word_end)
    return got


# ---------------------------------------------------------------------------------------------- the seek rule
def test_single_timestamp_ending_keeps_split_windows_advance(built_lib):
    ids = [T, 11, 12, T + 100, T + 100, 13, T + 250]  # ... text, one timestamp: the window is used up
    assert both(built_lib, ids, 6000, 3000, 3000, 62.5) == (3000, False)
    # two closing timestamps are a pair, not a single ending: the rule applies
    assert both(built_lib, ids + [T + 250], 6000, 3000, 500, 62.5) == (250, True)
    # a lone timestamp (one id) is no single ending either, as in openai-whisper, whose test needs two ids
    assert both(built_lib, [T + 3], 0, 3000, 3000, 1.0) == (100, True)


def test_last_word_before_the_windows_end_moves_the_seek(built_lib):
    ids = [T, 11, 12, T + 100, T + 100, 13, 14]  # ends in text: split_window stops at the closed pair (200 frames)
    assert both(built_lib, ids, 3000, 3000, 200, 41.26) == (1126, True)
    assert both(built_lib, ids, 0, 3000, 200, 0.02) == (2, True)
    # to the nearest frame, ties to even (Python's round on the double product)
    for end in (10.005, 10.015, 10.025, 7.125, 29.995):
        adv, by = both(built_lib, ids, 0, 3000, 200, end)
        assert by and adv == round(end * 100)


def test_no_words_keeps_split_windows_advance(built_lib):
    ids = [T, 11, 12, T + 100, T + 100, 13]
    assert both(built_lib, ids, 3000, 3000, 200, None) == (200, False)
    assert both(built_lib, [], 3000, 3000, 3000, None) == (3000, False)


def test_guards(built_lib):
    ids = [T, 11, 12, T + 100, T + 100, 13]
    # a last word that ends at the window's start, or before it: no move
    assert both(built_lib, ids, 3000, 3000, 200, 30.0) == (200, False)
    assert both(built_lib, ids, 3000, 3000, 200, 29.5) == (200, False)
    # ends behind the start but rounds to it: an advance of 0 keeps split_window's
    assert both(built_lib, ids, 3000, 3000, 200, 30.004) == (200, False)
    # an end beyond the window: kept too; exactly the window's end is allowed
    assert both(built_lib, ids, 3000, 1200, 200, 42.01) == (200, False)
    assert both(built_lib, ids, 3000, 1200, 200, 42.0) == (1200, True)


# ---------------------------------------------------------------------------------------------- the word rule in file time
def at(built_lib, table, ids, lang, seg_tokens, seg_start, seg_end, jump, last, offset):
    lp = np.log(np.linspace(0.3, 0.9, max(len(ids), 1))[: len(ids)]).astype(np.float32)
    got, gs, ge = built_lib.words_from_alignment(TABLE_PATH, ids, EOT, lang, seg_tokens, seg_start, seg_end, jump, lp, last, time_offset=offset)
    ref, rs, re_ = lw.words_from_alignment_at(table, ids, EOT, lang, seg_tokens, seg_start, seg_end, jump, lp, last, offset)
    assert [g[:4] for g in got] == [r[:4] for r in ref]
    assert np.allclose([g[4] for g in got], [r[4] for r in ref], rtol=2e-7, atol=0)
    assert list(gs) == list(rs) and list(ge) == list(re_)
    return got, list(gs), list(ge)


def test_offset_zero_is_the_existing_rule_to_the_bit(built_lib, table):
    ids = ids_of(table, b" a", b" b", b" c", b" d", b" e", b" f")
    jump = [0, 200, 400, 410, 420, 430, 700]
    lp = np.log(np.linspace(0.3, 0.9, len(ids))).astype(np.float32)
    for last in (0.0, 7.9):
        args = (TABLE_PATH, ids, EOT, "en", [3, 3], [3.0, 8.4], [8.4, 9.0], jump, lp, last)
        old, os_, oe = built_lib.words_from_alignment(*args)
        new, ns, ne = built_lib.words_from_alignment(*args, time_offset=0.0)
        assert [(w[0], w[1], w[2].hex(), w[3].hex(), np.float32(w[4]).tobytes()) for w in old] == \
               [(w[0], w[1], w[2].hex(), w[3].hex(), np.float32(w[4]).tobytes()) for w in new]
        assert [x.hex() for x in os_] == [x.hex() for x in ns] and [x.hex() for x in oe] == [x.hex() for x in ne]
        ref, rs, re_ = wr.words_from_alignment(table, *args[1:])
        assert [w[:4] for w in new] == [w[:4] for w in ref] and list(ns) == rs and list(ne) == re_
        assert lw.words_from_alignment_at(table, *args[1:], 0.0)[0] == ref


def test_clamp_at_zero_is_in_file_time(built_lib, table):
    """time_offset > 0 where a max(0, .) of the rule puts a word start BEFORE the window's start (the case a window-relative clamp
    gets wrong). The segment opens 0.56 s into a window that starts at 30 s; its first word begins at the window's start, more than
    0.5 s before the segment, and ends 0.6 s in: the rule moves its start to max(0, min(end - median, segment start)) with the median
    capped at 0.7 s: 30.6 - 0.7 = 29.9 s. In window time that is max(0, -0.1) = 0, i.e. 30.0 s."""
    ids = ids_of(table, b" a", b" b", b" c", b" d")
    jump = [0, 30, 130, 230, 330]  # ' a' 0.6 s, then three words of 2 s: the median is capped at 0.7 s
    got, ss, se = at(built_lib, table, ids, "en", [4], [30.56], [36.6], jump, last=29.5, offset=30.0)
    assert got[0][3] == 30.6 and got[0][2] == pytest.approx(29.9) and got[0][2] < 30.0
    assert ss[0] == 30.56  # the segment keeps its start: the word was moved instead
    # the same window at the file's start: there the clamp at 0 holds
    got0, _, _ = at(built_lib, table, ids, "en", [4], [0.56], [6.6], jump, last=-0.5, offset=0.0)
    assert got0[0][2] == 0.0 and got0[0][3] == 0.6


def test_offsets_rounding_and_segment_boundaries(built_lib, table):
    ids = ids_of(table, b" One", b" two", b".", b" Three", b" four", b"?", b" five")
    jump = [0, 10, 20, 120, 320, 330, 340, 440]
    for offset in (0.0, 0.01, 12.34, 29.99, 30.0, 1234.56, 3599.98):
        for last in (0.0, offset - 1.0, offset + 0.2):
            got, ss, se = at(built_lib, table, ids, "en", [3, 4], [offset + 0.0, offset + 2.4], [offset + 2.4, offset + 8.8], jump, last, offset)
            assert all(round(w[2], 2) == w[2] and round(w[3], 2) == w[3] for w in got)
    # pause rule on the second segment depends on last_speech_timestamp in file time: near and far give different first words
    ids = ids_of(table, b" a", b" b", b" c", b" d", b" e", b" f")
    jump = [0, 200, 400, 410, 420, 430, 700]
    near, _, _ = at(built_lib, table, ids, "en", [3, 3], [63.0, 68.4], [68.4, 69.0], jump, 63.9, 60.0)
    far, _, _ = at(built_lib, table, ids, "en", [3, 3], [63.0, 68.4], [68.4, 69.0], jump, 3.9, 60.0)
    assert near != far


def test_replay_of_a_hand_built_log(built_lib, table):
    """replay_window (what the GPU test replays the engine's log with) against the library's two calls chained by hand"""
    text = ids_of(table, b" He", b" said", b" hi", b".")
    ids = [T + 10] + text[:2] + [T + 60, T + 60] + text[2:] + [T + 200, T + 200, text[0]]
    jump = [5, 20, 30, 60, 95, 100]
    lp = np.log(np.linspace(0.4, 0.8, 4)).astype(np.float32)
    r = lw.replay_window(table, "en", T, EOT, 448, 4500, 3000, ids, jump, lp, 44.0)
    assert r["text_ids"] == text and r["seg_tokens"] == [2, 2]
    segs, adv = built_lib.split_window(ids, T, EOT, 3000)
    assert adv == 400
    got, gs, ge = built_lib.words_from_alignment(TABLE_PATH, text, EOT, "en", [2, 2], [45.0 + np.float32(s[0]) for s in segs],
                                                 [45.0 + np.float32(s[1]) for s in segs], jump, lp, 44.0, time_offset=45.0)
    assert [g[:4] for g in got] == [w[:4] for w in r["words"]] and list(gs) == r["seg_start"] and list(ge) == r["seg_end"]
    assert built_lib.long_word_advance(ids, T, 4500, 3000, adv, got[-1][3]) == (r["advance"], r["by_word_end"])
    assert r["by_word_end"] and r["advance"] == round(got[-1][3] * 100) - 4500 and r["last_speech_timestamp"] == got[-1][3]


# ---------------------------------------------------------------------------------------------- the path a jump list stands for
def test_jump_path_excess_is_zero_on_the_optimum_and_positive_off_it():
    """what test b of tests/test_gpu_long_words.py relies on: the jumps of the float64 DTW cost nothing extra, other jumps do, and the
    unconstrained cost is the cost of word_reference's own path"""
    rng = np.random.default_rng(7)
    for n, F in ((1, 1), (3, 5), (6, 40), (20, 150)):
        m = rng.standard_normal((n, F))
        jump = wr.align_path(m, np.float64)
        excess, cells = lw.jump_path_excess(m, jump)
        assert cells == n + F and abs(excess) < 1e-9
        # the path's own cost, walked cell by cell along word_reference's trace, is the optimum dtw_cost finds
        trace = wr.dtw(-m, np.float64)
        i, j, cost = n, F, 0.0
        while i > 0 and j > 0:
            cost += -m[i - 1, j - 1]
            t = trace[i, j]
            i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
        assert abs(cost - lw.dtw_cost(-m)) < 1e-9
        if F >= 2 * n and n > 1:
            ramp = [r * (F - 1) // n for r in range(n)]
            if list(jump) != ramp:
                assert lw.jump_path_excess(m, ramp)[0] > 0
    assert lw.jump_path_excess(np.zeros((2, 4)), [1, 2])[0] == np.inf  # a path has to begin at frame 0
