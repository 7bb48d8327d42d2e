"""Host: tests/repetition_reference.py against a brute-force loop; the two new calls without a handle (refusals of values need one)."""
import ctypes as C
import math

import numpy as np
import pytest

import repetition_reference as rr

E = 40


def _brute(row, seq, p, g):
    """position by position, no sets: the row after both rules"""
    x = [float(v) for v in row]
    done = []
    for c in seq:
        if c < E and c not in done:
            done.append(c)
            x[c] = x[c] * p if x[c] < 0 else x[c] / p
    n = len(seq)
    for i in range(0, n - g + 1 if g >= 2 else 0):
        if all(seq[i + j] == seq[n - g + 1 + j] for j in range(g - 1)) and seq[i + g - 1] < E:
            x[seq[i + g - 1]] = -math.inf
    return x


@pytest.mark.parametrize("g", [0, 2, 3, 16])
def test_reference_equals_the_brute_force_loop(g):
    rng = np.random.default_rng(100 + g)
    for trial in range(60):
        n = int(rng.integers(0, 45))
        seq = [int(v) for v in rng.integers(0, 6 if trial % 2 else 50, size=n)]  # (few distinct ids: many repeats; ids >= E: timestamps)
        if trial % 3 == 0 and n >= 2 * max(g, 2):  # a planted repeat of the tail
            k = max(g, 2) - 1
            seq[2:2 + k] = seq[n - k:]
        row = rng.standard_normal(50) * 3
        row[rng.integers(0, 50, size=5)] = 0.0
        p = float(np.float32((1.0, 1.3, 0.5)[trial % 3]))
        assert rr.edit_row(row, seq, E, p, g).tolist() == _brute(row, seq, p, g)


def test_the_two_symbols_resolve_and_refuse_no_handle(built_lib):
    L = built_lib.load_library()  # (tests/test_abi.py holds the header's declarations to the binding's SYMBOLS)
    p, g = C.c_float(), C.c_int()
    assert L.AX_WHISPER_SetRepetitionRules(None, 1.1, 3) == -1
    assert L.AX_WHISPER_GetRepetitionRules(None, C.byref(p), C.byref(g)) == -1
