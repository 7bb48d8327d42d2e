"""CPU: the long-form contract off the GPU — the numpy whole-file log-mel pinned against the oracle below frame 3000,
AX_WHISPER_SplitWindow against the Python window rule (one hand-built case per branch + seeded sequences that obey the timestamp
rules), the seek loop's termination, the two new kernels' resources in both builds, and the new exports."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import longform_reference as lfr
import ts_reference as tsr
from conftest import load_demo_pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["AX_WHISPER_SplitWindow", "AX_WHISPER_ComputeMelWindow", "AX_WHISPER_RunPCMLongWindows", "AX_WHISPER_RunPCMLong",
               "AX_WHISPER_RunFileLong"]
T, E, NV = 50364, 50257, 51865


@pytest.mark.parametrize("seconds", [0, 75], ids=["demo", "tiled_75s"])
def test_numpy_log_mel_is_pinned_to_the_oracle(oracle_mod, seconds):
    """The numpy log-mel is only trusted beyond frame 3000 because it agrees with oracle.log_mel below it: first 3000 frames and
    the maximum, to 5e-5."""
    pcm = load_demo_pcm()
    if seconds:
        pcm = np.tile(pcm, seconds * 16000 // len(pcm) + 1)[: seconds * 16000]
    want, n_frames, mmax = oracle_mod.log_mel(pcm, 80)
    norm, nf, mx = lfr.file_log_mel(pcm, 80)
    assert nf == n_frames == 1 + len(pcm) // 160
    assert abs(mx - mmax) < 5e-5, (mx, mmax)
    got = lfr.window_of(norm, 0)
    err = float(np.abs(got - want).max())
    print("numpy log-mel against oracle.log_mel: max |d| = %.3g, maximum %.7f / %.7f" % (err, mx, mmax))
    assert err < 5e-5
    if nf < 3000:
        assert (got[:, nf:] == 0).all()


def test_make_file_lengths_and_difference():
    demo = load_demo_pcm()
    files = {k: lfr.make_file(demo, k) for k in range(1, 6)}
    assert [len(files[k]) for k in range(1, 6)] == [192000, 480000, 720000, 1200000, 1600000]
    for a in range(1, 6):
        for b in range(a + 1, 6):
            assert not np.array_equal(files[a][:192000], files[b][:192000])


def _assert_same(built_lib, ids, window_frames):
    want, adv, branch = lfr.split_window(ids, T, E, window_frames)
    got, gadv = built_lib.split_window(ids, T, E, window_frames)
    assert gadv == adv, (ids, window_frames, gadv, adv)
    assert len(got) == len(want), (ids, got, want)
    for (s, e, b, f), (ws, we, wb, wf) in zip(got, want):
        # exact: the library rounds the double product pos * 0.02 to float once
        assert (np.float32(s), np.float32(e), b, f) == (np.float32(ws), np.float32(we), wb, wf), (ids, got, want)
    return want, adv, branch


def test_split_window_hand_built_cases(built_lib):
    x, y, z = 11, 12, 13
    # no timestamps at all: one segment over the window, full advance
    assert _assert_same(built_lib, [x, y, z], 3000) == ([(0.0, 30.0, 0, 3)], 3000, "none")
    # no cuts, the last timestamp is T itself: the window's end
    assert _assert_same(built_lib, [T, x], 1234) == ([(0.0, 12.34, 1, 2)], 1234, "none")
    # no cuts, a later single timestamp ends the segment
    assert _assert_same(built_lib, [T + 5, x, T + 100], 3000) == ([(0.0, 2.0, 1, 2)], 3000, "none")
    # cuts, not single_end: ids after the last pair belong to no segment, advance stops at the pair
    want, adv, br = _assert_same(built_lib, [T, x, T + 50, T + 50, y, z], 3000)
    assert (want, adv, br) == ([(0.0, 1.0, 1, 2)], 100, "cuts")
    # cuts + single_end: the trailing single timestamp closes the last segment, the window is used up
    want, adv, br = _assert_same(built_lib, [T, x, T + 50, T + 50, y, T + 80], 3000)
    assert (adv, br) == (3000, "single_end") and [(b, f) for _, _, b, f in want] == [(1, 2), (4, 5)]
    assert abs(want[1][0] - 1.0) < 1e-12 and abs(want[1][1] - 1.6) < 1e-12
    # a pair closing at 0.00 s: advance 0 -> the progress guard
    want, adv, br = _assert_same(built_lib, [T, T, x, y], 777)
    assert (want, adv, br) == ([], 777, "cuts")
    # advance beyond the window (a 10-frame window, a pair at 1.00 s) is capped
    assert _assert_same(built_lib, [T, x, T + 50, T + 50], 10)[1] == 10
    # empty input, and ids without eot / timestamps of length one
    assert _assert_same(built_lib, [], 3000) == ([], 3000, "none")
    assert _assert_same(built_lib, [x], 1) == ([(0.0, 0.01, 0, 1)], 1, "none")
    # a segment without text is not emitted
    want, adv, br = _assert_same(built_lib, [T, T + 10, T + 10, x, T + 20, T + 20], 3000)
    assert [(b, f) for _, _, b, f in want] == [(3, 4)] and adv == 40
    # ids in (E, T) are not text
    want, _, _ = _assert_same(built_lib, [T, E + 3, T + 9, T + 9], 3000)
    assert want == []


def _ruled_ids(rng):
    """A sequence every step of which is allowed by the timestamp rules (ts_reference.allowed); stops where eot would be taken."""
    seq = []
    n = rng.randrange(0, 48)
    p_ts = rng.choice([0.2, 0.4, 0.7])
    while len(seq) < n:
        ok = tsr.allowed(seq, T, E, NV)
        ts_ok = np.flatnonzero(ok[T:])
        text_ok = bool(ok[0])
        r = rng.random()
        if ts_ok.size and (r < p_ts or not text_ok):
            c = T + int(ts_ok[min(rng.choice([0, 0, 1, 3, 17, 400]), ts_ok.size - 1)])
        elif text_ok and r < 0.97:
            c = rng.randrange(0, E)
        else:
            assert ok[E] or not text_ok
            break  # eot (excluded from the ids)
        assert ok[c]
        seq.append(c)
    return seq


def test_split_window_matches_the_python_rule_on_ruled_sequences(built_lib):
    rng = random.Random(20240611)
    branches = {"none": 0, "cuts": 0, "single_end": 0}
    capped = 0  # (a pair closing at 0.00 s cannot follow the rules: the progress guard has its hand-built case)
    for it in range(2500):
        ids = _ruled_ids(rng)
        wf = rng.choice([3000, 3000, 1500, 200, 10, 1])
        want, adv, br = _assert_same(built_lib, ids, wf)
        branches[br] += 1
        assert 1 <= adv <= wf
        cuts = [i for i in range(1, len(ids)) if ids[i - 1] >= T and ids[i] >= T]
        if cuts and br == "cuts" and 2 * (ids[cuts[-1] - 1] - T) > wf:
            capped += 1
        assert all(ids[i] < T for _, _, b, f in want for i in range(b, f) if ids[i] < E)
    print("branches", branches, "advances capped at the window", capped)
    assert min(branches.values()) > 50 and capped > 0


def test_split_window_rejects_bad_arguments_and_respects_n_max(built_lib):
    import ctypes as C

    L = built_lib.load_library()
    n, adv = C.c_int(), C.c_int()
    assert L.AX_WHISPER_SplitWindow(None, 3, T, E, 3000, 0, None, None, None, None, C.byref(n), C.byref(adv)) == -1
    assert L.AX_WHISPER_SplitWindow(None, 0, T, E, 3000, 0, None, None, None, None, C.byref(n), C.byref(adv)) == 0
    assert (n.value, adv.value) == (0, 3000)
    ids = np.array([T, 1, T + 5, T + 5, 2, T + 9, T + 9, 3, T + 12], dtype=np.int32)
    st, en = np.full(4, -7.0, dtype=np.float32), np.full(4, -7.0, dtype=np.float32)
    tb, te = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
    pi = C.POINTER(C.c_int)
    rc = L.AX_WHISPER_SplitWindow(ids.ctypes.data_as(built_lib.ip), len(ids), T, E, 3000, 2, st.ctypes.data_as(built_lib.fp),
                                  en.ctypes.data_as(built_lib.fp), tb.ctypes.data_as(pi), te.ctypes.data_as(pi), C.byref(n), C.byref(adv))
    assert rc == 0 and n.value == 2 and adv.value == 3000
    assert (st[2:] == -7.0).all() and (tb[2:] == -7).all() and (te[2:] == -7).all()  # canaries past n_max


def test_python_loop_terminates_and_covers_the_file():
    # a decoder that always closes a pair at 0.00 s would never move without the progress guard
    log = lfr.loop(100 * 16000 + 7, lambda seek, wf: [T, T, 5], T, E)
    assert [w[0] for w in log] == [0, 3000, 6000, 9000] and log[-1][1] == 1000 and log[-1][0] + log[-1][2] == 10000
    # a pair at 20.00 s: the windows overlap by 10 s until the rest fits
    log = lfr.loop(75 * 16000, lambda seek, wf: [T, 5, T + 1000, T + 1000, 6], T, E)
    seeks = [w[0] for w in log]
    assert seeks == sorted(set(seeks)) and seeks[:3] == [0, 2000, 4000] and log[-1][0] + log[-1][2] == 7500
    assert lfr.loop(159, lambda seek, wf: [], T, E) == []  # below one frame: no window


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_long_form_kernels_compile_without_scratch_or_spills(f16, tmp_path):
    out = tmp_path / "frontend.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out),
                        os.path.join(ROOT, "whisper.axera_amd", "csrc", "frontend.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    for k in ("stft_mel_long_kernel", "mel_window_kernel", "stft_mel_kernel", "mel_normalize_kernel"):
        assert any(k in n for n in names), (k, names)
    assert re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M) == ["0"] * len(names)
    assert all(int(x) == 0 for x in re.findall(r"^\s+\.(?:vgpr|sgpr)_spill_count:\s+(\d+)", text, re.M))
    # the window kernel moves 16 bytes per access on both sides
    body = text[text.index("mel_window_kernel"):]
    body = body[: body.index(".end_amdhsa_kernel")]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body


def test_new_symbols_are_exported_and_declared(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    header = open(built_lib.HEADER_PATH).read()
    for s in NEW_SYMBOLS:
        assert s in header and s in built_lib.SYMBOLS
