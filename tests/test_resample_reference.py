"""CPU: the sample-rate conversion's definition, host side. The library's filter table (AX_WHISPER_ResampleFilter, csrc/resample.hpp)
against the float64 formula of tests/resample_reference.py (its own table, from np.i0), the length rule and the refusals
(AX_WHISPER_ResampledLength), the quality of the float32 table as a filter, and the checker the GPU tests use: a float32 emulation of
the sum passes every clip of resample_reference.CASES under the per-element bound, six seeded defects do not.

Filter quality, measured with numpy on the library's float32 table in float64 (0.5 s unit sinusoids, interior samples): worst
passband error up to 7000 Hz 5.6e-8, worst stopband amplitude from 8500 Hz 5.6e-8, DC gain of every phase within 6.2e-8 of 1 (the
thresholds below are 1e-6)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def wa():
    import __graft_entry__  # noqa: F401  (the package's import path)
    import whisper_axera_amd as wa

    wa.build()
    wa.load_library()
    return wa


@pytest.fixture(scope="module")
def lib_tables(wa):
    return {rate: wa.resample_filter(rate) for rate in R.RATES}


@pytest.mark.parametrize("rate", list(R.RATES))
def test_table_is_the_float64_formula_rounded_once(lib_tables, rate):
    L, M, K, table = lib_tables[rate]
    assert (L, M, K) == R.RATES[rate] == R.plan(rate)
    ref = R.table64(rate)
    assert table.shape == ref.shape == (L, 2 * K) and table.dtype == np.float32
    # one float32 ulp of the float64 value (the two libraries' sin and I0 differ by a few float64 ulps, far below that)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(table.astype(np.float64) - ref) <= ulp).all()
    assert np.array_equal(table == 0, ref == 0)  # outside |t| < W: exactly zero, inside: never


def test_length_follows_the_ceil_rule(wa):
    for rate, (L, M, _) in R.RATES.items():
        for n in (1, 2, 7, M, M + 1, 3 * M, 3 * M + 1, 479999, 480000, 1 << 20):
            assert wa.resampled_length(n, rate) == -((-n * L) // M) == R.n_out_of(n, rate), (rate, n)
    assert (441 * 160) % 441 == 0 and wa.resampled_length(441, 44100) == 160     # n L mod M = 0
    n1 = next(n for n in range(1, 2000) if (n * 160) % 441 == 1)                # n L mod M = 1: one output more than n L / M
    assert wa.resampled_length(n1, 44100) == (n1 * 160) // 441 + 1
    assert wa.resampled_length(12345, 16000) == 12345


@pytest.mark.parametrize("rate", [0, -1, 999, 384001, 44101])
def test_refused_rates(wa, rate):
    L = wa.load_library()
    assert L.AX_WHISPER_ResampledLength(1000, rate) == -1
    assert str(rate).encode() in L.AX_WHISPER_LastError(None)
    import ctypes as C
    l, m, k = C.c_int(), C.c_int(), C.c_int()
    assert L.AX_WHISPER_ResampleFilter(rate, C.byref(l), C.byref(m), C.byref(k), None, 0) == -1
    with pytest.raises(ValueError):
        wa.resample_filter(rate)


def test_refused_lengths(wa):
    L = wa.load_library()
    assert L.AX_WHISPER_ResampledLength((1 << 29) // 2 + 1, 8000) == -1   # the output exceeds 2^29
    assert L.AX_WHISPER_ResampledLength((1 << 29) // 2, 8000) == 1 << 29
    assert L.AX_WHISPER_ResampledLength((1 << 29) + 1, 48000) == -1       # the input does
    assert L.AX_WHISPER_ResampledLength(-1, 48000) == -1
    for rate in (88200, 1000, 384000):
        assert L.AX_WHISPER_ResampledLength(rate, rate) == 16000


# ------------------------------------------------------------------ filter quality, float64 on the library's float32 table
def _sinusoid_through(table, rate, f):
    n = rate // 2
    x = np.sin(2 * np.pi * f * np.arange(n, dtype=np.float64) / rate)
    y, _ = R.reference(x, rate, table)
    L, M, K = R.plan(rate)
    edge = -(-K * L // M) + 2
    j = np.arange(len(y))[edge + 1: len(y) - edge - 1]
    return y[j], np.sin(2 * np.pi * f * j / 16000.0)


@pytest.mark.parametrize("rate,freqs", [(44100, (100, 1000, 3000, 3700, 7000)), (48000, (100, 1000, 3000, 3700, 7000)), (8000, (100, 1000, 3000))])
def test_passband(lib_tables, rate, freqs):
    for f in freqs:
        y, want = _sinusoid_through(lib_tables[rate][3], rate, f)
        err = float(np.abs(y - want).max())
        print(f"{rate} Hz, {f} Hz: passband error {err:.2e}")
        assert err <= 1e-6, (rate, f, err)


@pytest.mark.parametrize("rate", [44100, 48000])
def test_stopband(lib_tables, rate):
    for f in (8500, 9000, 12000, 20000):
        y, _ = _sinusoid_through(lib_tables[rate][3], rate, f)
        amp = float(np.abs(y).max())
        print(f"{rate} Hz, {f} Hz: stopband amplitude {amp:.2e}")
        assert amp <= 1e-6, (rate, f, amp)


def test_dc_gain_of_every_phase(lib_tables):
    for rate, (_, _, _, table) in lib_tables.items():
        gain = table.astype(np.float64).sum(axis=1)
        assert np.abs(gain - 1.0).max() <= 1e-6, (rate, float(np.abs(gain - 1.0).max()))


# ------------------------------------------------------------------ the checker
HOST_CASES = list(R.host_cases())


def test_emulation_passes_every_case():
    worst = 0.0
    for label, rate, x in HOST_CASES:
        worst = max(worst, R.check(R.emulate32(x, rate), x, rate, label))
    print(f"float32 emulation, {len(HOST_CASES)} clips: worst error / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0


def _fails(y, x, rate):
    try:
        R.check(y, x, rate)
        n = np.flatnonzero(x)
        if n.size == 1 and x[n[0]] == 1.0:
            assert np.array_equal(y, R.impulse_expect(len(x), int(n[0]), rate))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_do_not_pass(defect):
    """Every defect is caught on the clips of CASES whose rate has more than one phase (the phase defects are no-ops at L == 1)."""
    caught = [label for label, rate, x in HOST_CASES if R.plan(rate)[0] > 1 and len(x) > 2 and _fails(R.emulate32(x, rate, defect), x, rate)]
    assert len(caught) >= 4, (defect, caught)


def test_impulse_comes_back_as_the_table_values():
    for rate in R.KERNEL_RATES:
        L, M, K = R.plan(rate)
        for n, p in ((2 * K + 1, K), (3 * K, 0), (3 * K, 3 * K - 1)):
            x = np.zeros(n, dtype=np.float32)
            x[p] = 1.0
            want = R.impulse_expect(n, p, rate)
            assert np.array_equal(R.emulate32(x, rate), want)
            assert np.count_nonzero(want) > 0
            R.check(want, x, rate)
