"""GPU: handle lifecycle, threading and failure behaviour of the C ABI."""
import os
import threading

import numpy as np
import pytest
import torch  # noqa: F401

from conftest import load_demo_pcm

pytestmark = pytest.mark.gpu


def test_one_handle_from_many_threads(built_lib, micro_case):
    """The reference's handle is not re-entrant yet its server calls it from a thread pool; here a handle
    is mutex-serialised: concurrent callers all get the single-threaded answer."""
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0)
    pcm = load_demo_pcm()
    want = e.run_tokens(pcm, max_new=10)
    out = [None] * 8
    th = [threading.Thread(target=lambda i=i: out.__setitem__(i, e.run_tokens(pcm, max_new=10))) for i in range(8)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert all(o == want for o in out)
    e.close()


def test_two_handles_are_independent(built_lib, micro_case):
    a = built_lib.Whisper("micro", micro_case.root, "zh", device=0)
    b = built_lib.Whisper("micro", micro_case.root, "en", device=0)
    pcm = load_demo_pcm()
    ra, rb = a.run_tokens(pcm, max_new=8), b.run_tokens(pcm, max_new=8)
    assert a.sot_seq != b.sot_seq
    assert a.run_tokens(pcm, max_new=8) == ra and b.run_tokens(pcm, max_new=8) == rb
    a.close()
    b.close()


def test_init_uninit_cycles_do_not_leak_device_memory(built_lib, micro_case):
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=3)
        e.run_tokens(load_demo_pcm(), max_new=4)
        e.close()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 << 20, (free0, free1)


def test_capacity_grows_on_demand(built_lib, micro_case):
    import modelgen

    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=1)
    clips = [modelgen.synth_clip(i, 100000) for i in range(7)]
    one = [e.run_tokens(c, max_new=6) for c in clips]
    assert e.run_tokens_batch(clips, max_new=6) == one  # 1 slot -> 7 slots, VALU path -> MFMA path
    e.close()


def test_corrupt_model_directories_fail_with_a_message(built_lib, micro_case, tmp_path):
    import shutil

    L = built_lib.load_library()
    src = os.path.join(micro_case.root, "micro")
    # 1. weights file truncated
    d1 = tmp_path / "a" / "micro"
    shutil.copytree(src, d1)
    p = d1 / "micro.safetensors"
    p.write_bytes(p.read_bytes()[: 4096])
    assert L.AX_WHISPER_Init(b"micro", str(tmp_path / "a").encode(), b"zh") is None
    assert L.AX_WHISPER_LastError(None)
    # 2. config is not JSON (the reference would throw through the C ABI)
    d2 = tmp_path / "b" / "micro"
    shutil.copytree(src, d2)
    (d2 / "micro_config.json").write_text("{ not json")
    assert L.AX_WHISPER_Init(b"micro", str(tmp_path / "b").encode(), b"zh") is None
    assert b"json" in L.AX_WHISPER_LastError(None)
    # 3. a tensor with the wrong shape
    import modelgen

    d3 = tmp_path / "c"
    w = dict(micro_case.weights)
    w["decoder.ln.weight"] = np.ones(64, dtype=np.float32)
    modelgen.write_model_dir(str(d3), "micro", micro_case.dims, weights=w)
    assert L.AX_WHISPER_Init(b"micro", str(d3).encode(), b"zh") is None
    assert b"decoder.ln.weight" in L.AX_WHISPER_LastError(None)


def _write_wav(path, data, rate=16000, fmt="int16"):
    """data: float array [n] or [n, ch] in [-1, 1)."""
    import struct

    a = np.atleast_2d(np.asarray(data, dtype=np.float64).T).T  # [n, ch]
    n, ch = a.shape
    if fmt == "int16":
        raw, bits, tag = (np.round(a * 32768).clip(-32768, 32767).astype("<i2")).tobytes(), 16, 1
    elif fmt == "int24":
        v = np.round(a * 8388608).clip(-8388608, 8388607).astype(np.int32).reshape(-1)
        raw, bits, tag = b"".join(int(x).to_bytes(3, "little", signed=True) for x in v), 24, 1
    elif fmt == "int32":
        raw, bits, tag = (np.round(a * 2147483648).clip(-2147483648, 2147483647).astype("<i4")).tobytes(), 32, 1
    elif fmt == "float32":
        raw, bits, tag = a.astype("<f4").tobytes(), 32, 3
    else:
        raise ValueError(fmt)
    blk = ch * bits // 8
    hdr = b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, tag, ch, rate, rate * blk, blk, bits)
    # an extra chunk before "data" must be skipped by the reader
    hdr += b"LIST" + struct.pack("<I", 4) + b"abcd"
    with open(path, "wb") as f:
        f.write(hdr + b"data" + struct.pack("<I", len(raw)) + raw)


def test_wav_ingest_formats(built_lib, micro_case, tmp_path):
    """AX_WHISPER_RunFile: int16 -> /32768 (AudioFile.h:1241-1243), stereo -> (L+R)/2 (ax_whisper_api.cpp:105-113); plus the
    int24 / int32 / float32 encodings AudioFile also reads."""
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0)
    pcm = load_demo_pcm()[:40000].astype(np.float64)
    q16 = np.round(pcm * 32768) / 32768  # exactly representable in every format below
    want = e.run(q16.astype(np.float32))
    for fmt in ("int16", "int24", "int32", "float32"):
        p = str(tmp_path / f"mono_{fmt}.wav")
        _write_wav(p, q16, fmt=fmt)
        assert e.run(p) == want, fmt
    # stereo: L = x + d, R = x - d  -> (L+R)/2 == x
    d = 0.25 * np.sin(np.arange(len(q16)) * 0.01)
    d = np.round(d * 32768) / 32768
    st = np.stack([np.clip(q16 + d, -1, 1 - 2 ** -15), np.clip(q16 - d, -1, 1 - 2 ** -15)], axis=1)
    mono = ((st[:, 0].astype(np.float32) + st[:, 1].astype(np.float32)) / 2).astype(np.float32)
    p = str(tmp_path / "stereo.wav")
    _write_wav(p, st, fmt="int16")
    assert e.run(p) == e.run(mono)
    # AIFF (the reference's AudioFile reads it as well, AudioFile.h:643-776): big-endian, COMM + SSND chunks
    import aifc

    for width in (2, 3):
        p = str(tmp_path / f"mono_{width * 8}.aiff")
        with aifc.open(p, "wb") as a:
            a.setnchannels(1); a.setsampwidth(width); a.setframerate(16000)
            v = np.round(q16 * (1 << (8 * width - 1))).astype(np.int64)
            a.writeframes(b"".join(int(x).to_bytes(width, "big", signed=True) for x in v))
        assert e.run(p) == want, width
    p = str(tmp_path / "stereo.aiff")
    with aifc.open(p, "wb") as a:
        a.setnchannels(2); a.setsampwidth(2); a.setframerate(16000)
        a.writeframes(np.round(st * 32768).clip(-32768, 32767).astype(">i2").tobytes())
    assert e.run(p) == e.run(mono)
    (tmp_path / "bad.aiff").write_bytes(b"FORM\x00\x00\x00\x04AIFF")
    with pytest.raises(RuntimeError):
        e.run(str(tmp_path / "bad.aiff"))
    cli = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_cli")
    import subprocess

    r = subprocess.run([cli, "-w", str(tmp_path / "mono_16.aiff"), "-t", "micro", "-p", micro_case.root, "--language", "zh"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"Result: {want}" in r.stdout, r.stdout + r.stderr
    e.close()


@pytest.mark.parametrize("batch", [1, 3, 6])
def test_non_finite_and_huge_audio_never_faults(built_lib, micro_case, batch):
    """an all-NaN logits row left the argmax at its 'no candidate' index, which was then fed back as a token
    and indexed the embedding table far out of bounds. Batch 1 = the persistent launch, 3 = the VALU GEMV path,
    6 = the MFMA path. NaN / Inf samples are refused at the ABI (-1); a finite 1e20-amplitude tone overflows the power
    spectrum on the device and must decode to SOMETHING (ids inside the vocabulary), not fault."""
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=batch)
    n = 48000
    t = np.arange(n, dtype=np.float32) / 16000
    good = load_demo_pcm()[:n]
    want_good = e.run_tokens(good, max_new=6)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[1234] = bad_value
        clips = [bad if b == batch - 1 else good for b in range(batch)]
        with pytest.raises(RuntimeError, match="non-finite"):
            e.run_tokens_batch(clips, max_new=6)
    huge = (1e20 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)
    clips = [huge if b == batch - 1 else good for b in range(batch)]
    out = e.run_tokens_batch(clips, max_new=6)
    assert all(0 <= i < e.n_vocab for row in out for i in row)
    for b in range(batch - 1):
        assert out[b] == want_good  # the poisoned clip does not leak into its neighbours
    # device-resident PCM bypasses the host check: NaN audio must still decode without a fault (an all-NaN logits row
    # gives id 0, what std::max_element returns, Whisper.cpp:42-45)
    nanclip = np.full(n, np.nan, dtype=np.float32)
    d = torch.from_numpy(np.stack([nanclip if b == batch - 1 else good for b in range(batch)])).cuda()
    out = e.run_device_tokens(d.data_ptr(), n, [n] * batch, max_new=6)
    assert all(0 <= i < e.n_vocab for i in out[batch - 1])
    for b in range(batch - 1):
        assert out[b] == want_good
    # the handle is still healthy
    assert e.run_tokens(good, max_new=6) == want_good
    e.close()


def test_failed_inits_do_not_leak_device_memory(built_lib, micro_case, tmp_path):
    """A constructor that throws half way (weights uploaded, then a bad tensor) must free what it allocated."""
    import modelgen

    w = dict(micro_case.weights)
    w["decoder.ln.bias"] = np.ones(64, dtype=np.float32)  # loaded last: everything before it is already on the device
    modelgen.write_model_dir(str(tmp_path), "micro", micro_case.dims, weights=w)
    L = built_lib.load_library()
    assert L.AX_WHISPER_Init(b"micro", str(tmp_path).encode(), b"zh") is None
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        assert L.AX_WHISPER_Init(b"micro", str(tmp_path).encode(), b"zh") is None
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 16 << 20, (free0, free1)


def _touch_every_lazily_created_object(e, tmp_path, monkeypatch):
    """Everything a handle creates on demand, once each (csrc/engine.hpp: the four owner groups)."""
    import modelgen

    clips = [modelgen.synth_clip(i, 40000 + 1000 * i) for i in range(24)]
    e.run_tokens(clips[0], max_new=4)  # one clip: the persistent launch
    e.run_timestamp_scores_batch(clips[:4], max_new=4)  # the timestamp logits and the score arrays
    assert len(e.run_tokens_batch(clips, max_new=4)) == 24  # capacity growth, a two-branch step graph, branch and pad streams, the queue probe
    assert e.get_config_int("decode_branches") >= 2
    e.run_tokens(modelgen.synth_clip(30, 65 * 16000), max_new=4)  # beyond a 60 s staging row: the overflow tail buffer
    e.stream_open(4)
    e.stream_admit_batch([0, 1], clips[:2], [4, 4])
    left = {0, 1}
    for _ in range(64):
        for sl in e.stream_step(4):
            e.stream_collect(sl)
            left.discard(sl)
        if not left:
            break
    assert not left
    e.stream_close()
    e.stream_open(6)  # regrows the ring and the admit events
    e.stream_close()
    e.run_long(modelgen.synth_clip(31, 70 * 16000), max_new=4)  # the arena and the pinned window table
    assert e.scan_stored16(1)
    assert e.bench("decode_step_ts_scored", 4, 0, 2) > 0
    stamps = tmp_path / "attn_stamps.csv"
    monkeypatch.setenv("AX_WHISPER_ATTN_STAMP", str(stamps))
    assert e.bench("attn_stamp", 4, 0, 1) > 0 and stamps.exists()
    with pytest.raises(RuntimeError, match="unknown target"):
        e.bench("no_such_target", 4, 0, 1)


def test_every_lazily_created_object_is_released(built_lib, micro_case, tmp_path, monkeypatch):
    """Exact, where the two memory-bound tests are thresholded: "live_hip_objects" counts every device and pinned buffer,
    stream, event and graph the handles of this process own (csrc/owned.hpp). A second handle that has touched everything
    created on demand leaves the count where it was, twice."""
    import gc

    gc.collect()  # (a handle an earlier test left to the collector would change the count under this test)
    a = built_lib.Whisper("micro", micro_case.root, "zh", device=0)
    try:
        base = a.get_config_int("live_hip_objects")
        assert base > 0
        for _ in range(2):
            b = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=1)
            try:
                _touch_every_lazily_created_object(b, tmp_path, monkeypatch)
                assert b.get_config_int("live_hip_objects") > 2 * base  # (it counts what b grew)
            finally:
                b.close()
            assert a.get_config_int("live_hip_objects") == base
    finally:
        a.close()


def test_failed_init_releases_every_object(built_lib, micro_case, tmp_path):
    """The constructor that throws half way (test_failed_inits_do_not_leak_device_memory), counted exactly: streams, events,
    the staging buffer and every weight uploaded before the bad tensor are given back."""
    import gc
    import modelgen

    w = dict(micro_case.weights)
    w["decoder.ln.bias"] = np.ones(64, dtype=np.float32)  # loaded last: everything before it is already on the device
    modelgen.write_model_dir(str(tmp_path), "micro", micro_case.dims, weights=w)
    L = built_lib.load_library()
    gc.collect()
    a = built_lib.Whisper("micro", micro_case.root, "zh", device=0)
    try:
        base = a.get_config_int("live_hip_objects")
        for _ in range(3):
            assert L.AX_WHISPER_Init(b"micro", str(tmp_path).encode(), b"zh") is None
            assert a.get_config_int("live_hip_objects") == base
    finally:
        a.close()


def test_multi_device_handle_shards_a_batch(built_lib, micro_case, monkeypatch):
    """AX_WHISPER_InitMulti: one engine per listed device behind one handle, RunPCMBatch* split into contiguous blocks
    (csrc/multi_device.hpp). A one-GPU box lists its device twice (test hook) so that two real engines, two worker
    threads and the join run for real; the sharding rule itself is covered on the CPU by tests/test_multi_device.py."""
    import modelgen

    L = built_lib.load_library()
    assert L.AX_WHISPER_VisibleDeviceCount() >= 1
    one = built_lib.Whisper("micro", micro_case.root, "zh", devices=[0], max_batch=3)
    assert one.n_devices == 1
    clips = [load_demo_pcm()] + [modelgen.synth_clip(i, 60000 + 7000 * i) for i in range(1, 7)]
    # the reference runs use the block shapes the 3-engine handle will use (3 + 3 + 1 clips; 1 + 1; 1 + 1 + 1), so both
    # sides take the same decode path per block (the paths differ in fp32 summation order, i.e. on numerical ties)
    want = one.run_tokens_batch(clips[:3], max_new=8) + one.run_tokens_batch(clips[3:6], max_new=8) + [one.run_tokens(clips[6], max_new=8)]
    want2 = [one.run_tokens(c, max_new=8) for c in clips[:2]]
    want_text = [one.run(c) for c in clips[:3]]
    one.close()
    with pytest.raises(RuntimeError, match="listed twice"):
        built_lib.Whisper("micro", micro_case.root, "zh", devices=[0, 0])
    with pytest.raises(RuntimeError, match="not visible|out of range"):
        built_lib.Whisper("micro", micro_case.root, "zh", devices=[0, 99])
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    e = built_lib.Whisper("micro", micro_case.root, "zh", devices=[0, 0, 0], max_batch=3)
    try:
        assert e.n_devices == 3 and e.L.AX_WHISPER_GetConfigInt(e.h, b"n_devices") == 3
        assert e.run_tokens_batch(clips, max_new=8) == want            # 7 clips -> blocks of 3, 3, 1
        assert e.run_tokens_batch(clips[:2], max_new=8) == want2       # fewer clips than devices: one clip each
        assert e.run_tokens(clips[1], max_new=8) == want2[1]
        got_text = e.run_batch(clips[:3])
        giveups = e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_giveups")  # summed over the three engines
        if got_text != want_text:
            # three one-clip decodes share ONE GPU here: an engine whose one-launch decoder could not get every CU in
            # time falls back to the launch-per-phase path, whose fp32 summation order differs (numerical ties over
            # 444 ids of a random-weight model). What this test is about — every clip's result in its own slot, in
            # order — shows in the head of each transcript; ids are compared exactly above (8 ids per clip).
            print("text differs past the head; persistent give-ups:", giveups)
            assert [t[:24] for t in got_text] == [t[:24] for t in want_text]
        bad = [c.copy() for c in clips]
        bad[5][100] = np.nan                                            # lives in the second device's block
        with pytest.raises(RuntimeError, match="device worker 1.*non-finite"):
            e.run_tokens_batch(bad, max_new=8)
        assert e.run_tokens_batch(clips, max_new=8) == want            # every worker was joined; the handle is intact
    finally:
        e.close()


def test_per_device_capture_mutex_switch(built_lib, micro_case, tmp_path):
    """AX_WHISPER_CAPTURE_MUTEX=device (csrc/api.cpp device_capture_mutex: one mutex per device instead of one per process; read
    once per process, so this runs in a child). Two handles on device 0, driven from two threads at once through the paths that
    take that mutex — capacity growth, first-time capture of a 5-clip step graph, StreamOpen — give the ids of the same calls made
    one after the other in the same process."""
    import subprocess
    import sys
    import textwrap

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "child.py"
    script.write_text(textwrap.dedent(f"""
        import sys, threading
        sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'whisper.axera_amd', 'tools')!r})
        import numpy as np, torch
        import modelgen, whisper_axera_amd as wa
        clips = [modelgen.synth_clip(i, 50000 + 9000 * i) for i in range(6)]
        def work(e, out):
            out.append(e.run_tokens_batch(clips[:5], max_new=10))          # grows the capacity 1 -> 5, captures the 5-clip step graph
            got, _ = e.run_stream(clips, 3, max_new=6, steps_per_call=2)  # StreamOpen + slot buffers
            out.append(got)
        a = wa.Whisper("micro", {micro_case.root!r}, "zh", device=0, max_batch=1)
        want = []
        work(a, want)
        a.close()
        hs = [wa.Whisper("micro", {micro_case.root!r}, "zh", device=0, max_batch=1) for _ in range(2)]
        outs = [[], []]
        ts = [threading.Thread(target=work, args=(h, o)) for h, o in zip(hs, outs)]
        [t.start() for t in ts]; [t.join() for t in ts]
        for h in hs: h.close()
        assert outs[0] == want and outs[1] == want, "concurrent handles differ from the sequential run"
        print("OK", len(want[0]), len(want[1]))
    """))
    env = dict(os.environ, AX_WHISPER_CAPTURE_MUTEX="device")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK 5 6" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
