"""CPU: chunked long-form without a GPU (DESIGN.md "Chunked long-form") — the host cut rule (AX_WHISPER_LongCutPlanHost) against the
Python rule on crafted and random levels, the invariants of every plan, a window's segments in file time (AX_WHISPER_ChunkedSegments)
against Python, the refusals, the float64 levels reference on a hand-computed case, the derived fp32 bound, and the ABI additions."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import long_cuts_reference as lcr

T, E = 50364, 50257  # timestamp_begin and eot of the multilingual vocabulary

NEW = ("AX_WHISPER_LongCutPlanHost", "AX_WHISPER_ChunkedSegments", "AX_WHISPER_LongFrameLevels", "AX_WHISPER_LongCutPlanFromLevels",
       "AX_WHISPER_LongCutPlan", "AX_WHISPER_ComputeMelWindowCut", "AX_WHISPER_RunPCMLongChunkedWindows", "AX_WHISPER_RunPCMLongChunked",
       "AX_WHISPER_RunFileLongChunked")


@pytest.mark.parametrize("name", sorted(lcr.crafted_levels()))
def test_host_rule_on_crafted_levels(built_lib, name):
    s, w_min, w_max = lcr.crafted_levels()[name]
    want = lcr.cut_plan(s, w_min, w_max)
    got = built_lib.long_cut_plan_host(s, w_min, w_max)
    assert got == want, (name, got, want)
    lcr.check_plan(got, len(s), w_min, w_max)
    if name == "one_clear_minimum":
        assert got[0] == (0, 260)
    if name == "exact_ties":
        assert got[0] == (0, 290) and got[1] == (290, 300)  # the latest of equal minima; then a flat stretch: the latest frame
    if name == "odd_minimum_not_taken":
        assert got[0] == (0, 240) and all(seek != 251 for seek, _ in got)
    if name == "signed_zero_tie":
        assert got[0] == (0, 300)  # -0.0 == 0.0 as float32: a tie
    if name in ("one_window", "one_window_short"):
        assert got == [(0, len(s))]
    if name == "content_wmax_plus_1":
        assert len(got) == 2 and got[1][1] >= 1
    if name == "content_wmax_plus_wmin":
        assert len(got) == 2


def test_host_rule_on_random_levels(built_lib):
    n_ties = 0
    for k in range(50):
        s = lcr.random_levels(k)
        want = lcr.cut_plan(s, 200, 300)
        assert built_lib.long_cut_plan_host(s, 200, 300) == want, k
        lcr.check_plan(want, len(s), 200, 300)
        for seek, ln in want[:-1]:
            cand = s[seek + 200: seek + 301: 2]
            n_ties += int((cand == cand.min()).sum() > 1)
    assert n_ties > 100  # the quantised levels do exercise the tie rule


def test_content_below_the_levels_and_empty_files(built_lib):
    s = lcr.random_levels(0)
    assert built_lib.long_cut_plan_host(s, 200, 300, content=1234) == lcr.cut_plan(s, 200, 300, content=1234)
    assert built_lib.long_cut_plan_host(s, 200, 300, content=0) == [] == lcr.cut_plan(s, 200, 300, content=0)


def test_refusals_of_the_host_rule(built_lib):
    s = np.zeros(4000, dtype=np.float32)
    for w_min, w_max in ((201, 300), (200, 301), (300, 200), (2000, 3002), (0, 300), (3002, 3002)):
        with pytest.raises(ValueError, match="chunk_m"):
            built_lib.long_cut_plan_host(s, w_min, w_max)
        with pytest.raises(ValueError):
            lcr.cut_plan(s, w_min, w_max)
    bad = s.copy()
    bad[17] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        built_lib.long_cut_plan_host(bad, 200, 300)
    # a win_cap too small: -1, nothing written
    L = built_lib.load_library()
    seek, ln, n = (C.c_int * 2)(-7, -7), (C.c_int * 2)(-7, -7), C.c_int(-7)
    assert L.AX_WHISPER_LongCutPlanHost(s.ctypes.data_as(built_lib.fp), 4000, 200, 300, 2, seek, ln, C.byref(n)) == -1
    assert b"windows were planned, win_cap is 2" in L.AX_WHISPER_LastError(None)
    assert list(seek) == [-7, -7] and list(ln) == [-7, -7] and n.value == 0
    with pytest.raises(ValueError):
        lcr.check_params(2000, 3000, 65)  # R > 64 (the library refuses it where it takes R: tests/test_gpu_long_chunked.py)


def test_smooth_frames_above_64_is_refused_by_the_shared_check(tmp_path):
    """cut_params_error is the one check every entry point uses (host only): R = 65 is refused, R = 64 and R = 0 are taken."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include "long_cuts.hpp"\n#include <cstdio>\nint main() { printf("%d %d %d %d\\n", (int)axw::cut_params_error(2000, 3000, 65).empty(), '
                   '(int)axw::cut_params_error(2000, 3000, 64).empty(), (int)axw::cut_params_error(2000, 3000, 0).empty(), '
                   '(int)axw::cut_params_error(2000, 3000, -1).empty()); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "whisper.axera_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split() == ["0", "1", "1", "0"]


SEGMENT_CASES = {
    "cuts": ([T, 5, 6, T + 100, T + 100, 7, T + 250, T + 250, 8, T + 400, T + 400], 1000, 900),
    "trailing_open_segment": ([T, 5, T + 100, T + 100, 6, 7], 2000, 500),
    "trailing_after_text_only": ([T, 5, T + 100, T + 100, 6, T + 180], 0, 400),
    "timestamp_beyond_len_is_clamped": ([T, 5, T + 1400, T + 1400, 6, T + 1500], 4000, 2200),
    "no_pairs": ([T + 10, 5, 6, 7], 300, 640),
    "no_pairs_closing_timestamp": ([T, 5, 6, T + 77], 300, 640),
    "no_text": ([T, T + 50, T + 50, T + 60], 0, 3000),
    "empty": ([], 100, 100),
}


@pytest.mark.parametrize("name", sorted(SEGMENT_CASES))
def test_chunked_segments_against_python(built_lib, name):
    ids, seek, ln = SEGMENT_CASES[name]
    want = lcr.chunked_segments(ids, T, E, seek, ln)
    got = built_lib.chunked_segments(ids, T, E, seek, ln)
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g[2:] == w[2:] and abs(g[0] - w[0]) < 1e-9 and abs(g[1] - w[1]) < 1e-9, (g, w)
    if name == "trailing_open_segment":
        assert len(got) == 2 and got[1][2:] == (4, 6) and abs(got[1][0] - 22.0) < 1e-9 and abs(got[1][1] - 25.0) < 1e-9  # kept, to the window's end
    if name == "timestamp_beyond_len_is_clamped":
        assert abs(got[0][1] - 62.0) < 1e-9 and abs(got[1][0] - 62.0) < 1e-9 and abs(got[1][1] - 62.0) < 1e-9  # 28 s and 30 s -> len = 22 s
    if name == "cuts":
        assert [round(g[0], 6) for g in got] == [10.0, 12.0, 15.0] and got[-1][1] == pytest.approx(18.0)
    if name in ("no_text", "empty"):
        assert got == []
    for g in got:
        assert seek * 0.01 - 1e-9 <= g[0] <= g[1] <= (seek + ln) * 0.01 + 1e-9


@pytest.mark.parametrize("name", sorted(SEGMENT_CASES))
def test_chunked_segments_are_split_segments_in_file_time(built_lib, name):
    """The contract the mode names: AX_WHISPER_ChunkedSegments(ids, seek, len) is AX_WHISPER_SplitSegments(ids, clip_seconds = len / 100)
    with every time t mapped to seek / 100 + min(t, len / 100). SplitSegments returns float32 seconds: times below 60 s, rounded once
    at 2^-24 relative, so 1e-5 s covers the difference."""
    ids, seek, ln = SEGMENT_CASES[name]
    clip = ln / 100.0
    want = [(seek / 100.0 + min(s, clip), seek / 100.0 + min(e, clip), tb, te) for s, e, tb, te in built_lib.split_segments(ids, T, E, clip)]
    got = built_lib.chunked_segments(ids, T, E, seek, ln)
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g[2:] == w[2:] and abs(g[0] - w[0]) < 1e-5 and abs(g[1] - w[1]) < 1e-5, (g, w)


def test_levels_reference_on_a_hand_computed_case():
    """5 frames of 8 mels, R = 7 > the frame count: every box reaches both ends, so the index clamp decides the weights."""
    x = np.array([[1.0] * 8, [0.0, 2.0] * 4, [3.0] * 8, [0.5] * 4 + [1.5] * 4, [2.0] * 8])
    e, s = lcr.frame_levels(x, 7)
    assert np.array_equal(e, [1.0, 1.0, 3.0, 1.0, 2.0])
    # frame f: offsets -7 .. 7 hit index 0 for f + j <= 0 (8 - f times), 4 for f + j >= 4 (4 + f times), 1, 2, 3 once each
    want = [((8 - f) * 1.0 + 1.0 + 3.0 + 1.0 + (4 + f) * 2.0) / 15.0 for f in range(5)]
    assert np.allclose(s, want, rtol=0, atol=1e-15)
    e0, s0 = lcr.frame_levels(x, 0)
    assert np.array_equal(e0, s0)
    e1, s1 = lcr.frame_levels(x, 1)
    assert np.allclose(s1, [(1 + 1 + 1) / 3, (1 + 1 + 3) / 3, (1 + 3 + 1) / 3, (3 + 1 + 2) / 3, (1 + 2 + 2) / 3], rtol=0, atol=1e-15)


def test_the_derived_bound_covers_fp32_sums_in_any_order():
    """The bound of levels_bounds against fp32 sums taken in three different orders (sequential, reversed, pairwise) on values of the
    size the encoder sees: every order stays inside, and the bound is not slack by more than the term count."""
    rng = np.random.default_rng(7)
    for nm, R in ((80, 25), (128, 64), (8, 0)):
        x = rng.uniform(-1.0, 1.5, (400, nm)).astype(np.float32)
        e_ref, s_ref = lcr.frame_levels(x, R)

        def mean32(a, order):
            a = a[:, ::-1] if order == "reversed" else a
            if order == "pairwise":
                v = a.astype(np.float32)
                while v.shape[1] > 1:
                    if v.shape[1] % 2:
                        v = np.concatenate([v, np.zeros((v.shape[0], 1), np.float32)], axis=1)
                    v = (v[:, 0::2] + v[:, 1::2]).astype(np.float32)
                acc = v[:, 0]
            else:
                acc = np.zeros(a.shape[0], dtype=np.float32)
                for j in range(a.shape[1]):
                    acc = (acc + a[:, j]).astype(np.float32)
            return (acc / np.float32(a.shape[1])).astype(np.float32)

        for order in ("sequential", "reversed", "pairwise"):
            e = mean32(x, order)
            idx = np.clip(np.arange(400)[:, None] + np.arange(-R, R + 1)[None, :], 0, 399)
            s = mean32(e[idx], order)
            be, bs = lcr.levels_bounds(x, e, R)
            assert (np.abs(e - e_ref) <= be).all() and (np.abs(s - s_ref) <= bs).all(), (nm, R, order)
        assert be.max() < 1.02 * nm * lcr.U32 * 1.5 and bs.max() < 1.02 * (nm + 2 * R + 1) * lcr.U32 * 1.5


def test_new_symbols_are_declared_exported_and_bound(built_lib):
    header = open(built_lib.HEADER_PATH).read()
    lib = C.CDLL(built_lib.LIB_PATH)
    for n in NEW:
        assert n + "(" in header and hasattr(lib, n) and n in built_lib.SYMBOLS, n
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    assert exported and all(s.startswith("AX_WHISPER_") for s in exported)  # nothing else leaks


def test_null_handle_and_null_pointers_return_minus_one(built_lib):
    L = built_lib.load_library()
    fp = built_lib.fp
    x = np.zeros(1600, dtype=np.float32)
    out = np.full(16, 7.0, dtype=np.float32)
    ptr = (fp * 1)(x.ctypes.data_as(fp))
    optr = (fp * 1)(out.ctypes.data_as(fp))
    one = (C.c_int * 1)(1600)
    n = (C.c_int * 1)(-5)
    ids = np.zeros(448, dtype=np.int32)
    text = C.c_void_p(123)
    assert L.AX_WHISPER_LongFrameLevels(None, ptr, one, 1, 25, optr, optr) == -1
    assert L.AX_WHISPER_LongCutPlanFromLevels(None, x.ctypes.data_as(fp), 1600, 200, 300, 16, n, n, n) == -1
    assert L.AX_WHISPER_LongCutPlan(None, ptr, one, 1, None, 16, n, n, n, n, None) == -1
    assert L.AX_WHISPER_ComputeMelWindowCut(None, x.ctypes.data_as(fp), 1600, 0, 5, out.ctypes.data_as(fp)) == -1
    assert L.AX_WHISPER_RunPCMLongChunkedWindows(None, ptr, one, 1, 4, 0, None, None, 1, n, ids.ctypes.data_as(built_lib.ip), None, n) == -1
    assert L.AX_WHISPER_RunPCMLongChunked(None, x.ctypes.data_as(fp), 1600, None, None, C.byref(text)) == -1
    assert L.AX_WHISPER_RunFileLongChunked(None, b"x.wav", None, None, C.byref(text)) == -1
    assert (out == 7.0).all() and n[0] == -5 and not ids.any()
    # host only: NULL outputs
    assert L.AX_WHISPER_LongCutPlanHost(x.ctypes.data_as(fp), 1600, 200, 300, 16, None, None, n) == -1
    assert L.AX_WHISPER_LongCutPlanHost(None, 1600, 200, 300, 16, n, n, n) == -1
    assert L.AX_WHISPER_ChunkedSegments(ids.ctypes.data_as(built_lib.ip), 4, T, E, 0, 100, 4, None, None, None, None, n) == -1
    assert L.AX_WHISPER_ChunkedSegments(ids.ctypes.data_as(built_lib.ip), 4, T, E, 0, 3001, 0, None, None, None, None, n) == -1
    assert n[0] == -5
