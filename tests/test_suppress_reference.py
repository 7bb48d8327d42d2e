"""CPU, no library: tests/suppress_reference.py on tests/golden/multilingual.tiktoken against the published multilingual non-speech
list (tests/golden/non_speech_multilingual.json), and the reference's own mask layout, validity rule and row filter."""
import json
import os

import numpy as np
import pytest

import suppress_reference as sup
from conftest import GOLDEN

NV, EOT, T = 51865, 50257, 50364


@pytest.fixture(scope="module")
def ranks():
    return sup.load_ranks(os.path.join(GOLDEN, "multilingual.tiktoken"))


@pytest.fixture(scope="module")
def fixture_ids():
    return json.load(open(os.path.join(GOLDEN, "non_speech_multilingual.json")))


def test_non_speech_tokens_equal_the_published_list(ranks, fixture_ids):
    got = sup.non_speech_tokens(ranks)
    assert got == fixture_ids
    assert len(got) == 82 and got == sorted(set(got)) and got[-1] < EOT


def test_one_piece_bpe(ranks):
    assert sup.bpe_one_piece(ranks, b" ") == [220]
    # a piece that is one entry, and a musical sign that is not: its first id is what the list takes
    assert sup.bpe_one_piece(ranks, b" (") == [ranks[b" ("]]
    ids = sup.bpe_one_piece(ranks, "♩".encode())
    assert len(ids) > 1 and ids[0] in sup.non_speech_tokens(ranks)
    inv = {v: k for k, v in ranks.items()}
    for piece in (" ♪♪♪", "(((", " 『", "--"):
        assert b"".join(inv[i] for i in sup.bpe_one_piece(ranks, piece.encode())) == piece.encode()
    with pytest.raises(KeyError):
        sup.bpe_one_piece({b"a": 0}, b"ab")


@pytest.mark.parametrize("ids", ([0], [3, 4], [31, 32, 33], [1023, 1024], [EOT - 1], [EOT + 1, T - 1, 5, 5, 5], list(range(EOT))),
                         ids=["0", "3_4", "31_32_33", "1023_1024", "eot-1", "special_and_duplicates", "all_text"])
def test_mask_sets_the_bits_below_eot_and_none_above(ids):
    for nv in (NV, NV + 1):
        m = sup.mask_words(ids, nv, EOT)
        assert m.dtype == np.uint32 and len(m) % 4 == 0 and len(m) * 32 >= nv and len(m) * 32 < nv + 128
        bits = np.unpackbits(m.view(np.uint8), bitorder="little")
        want = np.zeros(len(m) * 32, dtype=np.uint8)
        want[[i for i in ids if i < EOT]] = 1
        assert np.array_equal(bits, want)
        assert not bits[EOT:].any()
    assert len(sup.mask_words([], NV, EOT)) == 1624


def test_validity_rule():
    assert sup.check_ids([5, 3, 5, EOT + 1, T - 1], NV, EOT, T) == [3, 5, EOT + 1, T - 1]
    assert sup.check_ids([], NV, EOT, T) == []
    for bad in ([EOT], [T], [NV - 1], [NV], [-1], [0] * (NV + 1)):
        with pytest.raises(ValueError):
            sup.check_ids(bad, NV, EOT, T)


def test_suppress_rows_is_a_copy_with_minus_inf():
    x = np.arange(24, dtype=np.float32).reshape(2, 12)
    y = sup.suppress_rows(x, [3, 3, 7])
    assert y is not x and x[0, 3] == 3.0
    assert np.isneginf(y[:, [3, 7]]).all() and np.array_equal(np.delete(y, [3, 7], axis=1), np.delete(x, [3, 7], axis=1))
    assert np.array_equal(sup.suppress_rows(x, []), x)
