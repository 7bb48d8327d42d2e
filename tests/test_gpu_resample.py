"""GPU: audio at any sample rate through the C ABI (DESIGN.md "Sample rates"), with the micro model and the suite's fixtures.

The stage-level call (AX_WHISPER_ResampleBatch) against the float64 reference under the per-element bound of
tests/resample_reference.py; a band-limited signal against its own analytic samples at 16 kHz; the fused upload path
(AX_WHISPER_ComputeMelRate: upload, resample kernel into the staging row and the overflow buffer, front-end) bit-equal to the staged
one; the decode entry points with a rate per clip (AX_WHISPER_RunPCMBatchRate on one engine and sharded over two engines of one GPU,
AX_WHISPER_StreamAdmitBatchRate with a second admission pass right behind the first) giving the ids of the resampled clips; the file
calls; a refused rate.
"""
import os
import wave

import numpy as np
import pytest

import resample_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    import modelgen

    td = str(tmp_path_factory.mktemp("resample_micro"))
    dims = modelgen.DIMS["micro"]
    modelgen.write_model_dir(td, "micro", dims, weights=modelgen.synth_weights(dims, seed=7))
    return td


@pytest.fixture(scope="module")
def eng(built_lib, model_dir):
    e = built_lib.Whisper("micro", model_dir, "zh", device=0, max_batch=4)
    yield e
    e.close()


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


@pytest.fixture(scope="module")
def clips(demo_pcm):
    """Three clips for the decode tests: speech samples declared to be at 8000 and 44100 Hz (what they sound like does not matter
    here), and one at 16000 Hz."""
    return [demo_pcm[: 8000 * 3].copy(), demo_pcm[: 44100].copy(), demo_pcm[16000: 16000 * 3].copy()], [8000, 44100, 16000]


SECOND = {rate: noise(rate, 100 + rate) for rate in (8000, 44100, 48000)}


def test_16000_is_the_identity(eng):
    x = noise(12345, 1)
    y = eng.resample(x, 16000)
    assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("rate", list(SECOND))
def test_one_second_of_noise_stays_within_the_bound(eng, rate):
    y = eng.resample(SECOND[rate], rate)
    w = R.check(y, SECOND[rate], rate, f"{rate} Hz")
    print(f"{rate} Hz: worst error / bound {w:.3f}")


def test_batch_equals_the_single_calls(eng):
    rates = list(SECOND)
    single = [eng.resample(SECOND[r], r) for r in rates]
    batch = eng.resample_batch([SECOND[r] for r in rates], rates)
    for a, b in zip(single, batch):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_band_limited_signal_against_its_own_16_khz_samples(eng):
    freqs = np.array([100.0, 1000.0, 3000.0, 3700.0, 7000.0])
    amps = np.array([0.3, 0.25, 0.2, 0.15, 0.1])  # sum 1: the signal stays inside [-1, 1]
    phase = np.array([0.1, 0.7, 1.3, 2.1, 2.9])
    sig = lambda rate, n: (amps[:, None] * np.sin(2 * np.pi * freqs[:, None] * np.arange(n)[None, :] / rate + phase[:, None])).sum(axis=0)
    x48 = sig(48000, 24000).astype(np.float32)
    y = eng.resample(x48, 48000)
    assert len(y) == 8000
    _, bound = R.reference(x48, 48000)
    L, M, K = R.plan(48000)
    edge = -(-K * L // M) + 2
    j = np.arange(len(y))[edge + 1: len(y) - edge - 1]
    err = np.abs(y.astype(np.float64) - sig(16000, 8000))[j]
    tol = (1e-6 + bound[j]) * amps.sum()
    print(f"band-limited: worst error {err.max():.2e}, worst error / tolerance {(err / tol).max():.3f}")
    assert (err <= tol).all()


@pytest.mark.parametrize("rate,n", [(44100, 44100), (16000, 20000), (8000, 488000)], ids=["44100", "16000", "8000 into the overflow buffer"])
def test_fused_upload_equals_staged(eng, rate, n):
    x = noise(n, 7 + rate) * np.float32(0.5)
    staged = eng.resample(x, rate)
    if rate == 8000:
        assert len(staged) == 976000 > 960000  # beyond the 960000-sample staging row: the tail lands in the overflow buffer
    a = eng.compute_mel(x, rate=rate)
    b = eng.compute_mel(staged)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(a).all()


def _resampled(eng, clips, rates):
    return [eng.resample(c, r) for c, r in zip(clips, rates)]


@pytest.mark.parametrize("timestamps", [False, True], ids=["plain", "timestamps"])
def test_run_tokens_batch_rate_gives_the_ids_of_the_resampled_clips(eng, clips, timestamps):
    cl, rates = clips
    got = eng.run_tokens_batch_rate(cl, rates, max_new=6, timestamps=timestamps)
    res = _resampled(eng, cl, rates)
    want = eng.run_timestamp_tokens_batch(res, max_new=6) if timestamps else eng.run_tokens_batch(res, max_new=6)
    assert got == want and all(len(g) > 0 for g in got)


def test_sharded_over_two_engines_of_one_gpu(built_lib, model_dir, eng, clips, monkeypatch):
    cl, rates = clips
    want = eng.run_tokens_batch(_resampled(eng, cl, rates), max_new=6)
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    two = built_lib.Whisper("micro", model_dir, "zh", max_batch=4, devices=[0, 0])
    try:
        assert two.n_devices == 2
        assert two.run_tokens_batch_rate(cl, rates, max_new=6) == want  # (blocks of two clips and one: the rates travel with them)
    finally:
        two.close()


def _stream(eng, passes, rated):
    """Two admission passes right behind each other into four slots, then steps until every slot has finished."""
    eng.stream_open(4)
    try:
        for slots, cl, rates in passes:
            if rated:
                eng.stream_admit_batch(slots, cl, max_new=[6] * len(cl), rates=rates)
            else:
                eng.stream_admit_batch(slots, cl, max_new=[6] * len(cl))
        done, out = set(), {}
        for _ in range(200):
            done |= set(eng.stream_step(4))
            if len(done) == 4:
                break
        assert len(done) == 4
        for s in sorted(done):
            out[s] = eng.stream_collect(s)
        return out
    finally:
        eng.stream_close()


def test_stream_admit_with_rates(eng, demo_pcm):
    raw = [(demo_pcm[:16000].copy(), 8000), (demo_pcm[:48000].copy(), 48000), (demo_pcm[8000:30050].copy(), 44100), (demo_pcm[4000:12000].copy(), 8000)]
    res = [eng.resample(c, r) for c, r in raw]
    rated = _stream(eng, [([0, 1], [raw[0][0], raw[1][0]], [8000, 48000]), ([2, 3], [raw[2][0], raw[3][0]], [44100, 8000])], True)
    plain = _stream(eng, [([0, 1], res[:2], None), ([2, 3], res[2:], None)], False)
    assert rated == plain and all(len(v) > 0 for v in rated.values())


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(pcm, -1, 1) * 32767).astype(np.int16).tobytes())


def test_file_calls(built_lib, eng, demo_pcm, tmp_path):
    p8, p16 = tmp_path / "a8k.wav", tmp_path / "a16k.wav"
    _write_wav(p8, demo_pcm[::2][:40000], 8000)
    _write_wav(p16, demo_pcm[:80000], 16000)
    samples, rate, ch = built_lib.load_audio_file(str(p8))
    assert rate == 8000 and ch == 1
    staged = eng.resample(samples, 8000)
    assert eng.run(str(p8), resample=True) == eng.run(staged)
    assert eng.run(str(p16), resample=True) == eng.run(str(p16))
    got, r, c, n = eng.load_audio_file_16k(str(p8))
    assert (r, c, n) == (8000, 1, len(samples)) and np.array_equal(got.view(np.uint32), staged.view(np.uint32))
    got16, r16, _, _ = eng.load_audio_file_16k(str(p16))
    assert r16 == 16000 and np.array_equal(got16, built_lib.load_audio_file(str(p16))[0])


def test_a_refused_rate_fails_the_call_and_leaves_the_handle_usable(eng, clips):
    cl, rates = clips
    with pytest.raises(RuntimeError, match="44101"):
        eng.run_tokens_batch_rate(cl, [8000, 44101, 16000], max_new=6)
    with pytest.raises(RuntimeError, match="999"):
        eng.compute_mel(cl[0], rate=999)
    assert eng.run_tokens_batch_rate(cl, rates, max_new=6) == eng.run_tokens_batch(_resampled(eng, cl, rates), max_new=6)
