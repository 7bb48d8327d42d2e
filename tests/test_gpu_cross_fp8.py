"""GPU: the FP8 cross K/V mode of a handle (AX_WHISPER_CROSS_KV=fp8; DESIGN.md "FP8 cross K/V") through the engine.

What is compared with what:
  codes and scales   get_cross_kv_fp8(slot) == tests/cross_fp8_reference.quantize(get_cross_kv(slot)), bit for bit (the power-of-two
                     scale makes x * 2^-e exact, the code is one round-to-nearest-even)
  logits             decode_forced on the fp8 handle against the bf16-policy oracle fed the DEQUANTISED K/V (code * scale, exactly
                     representable in the oracle's storage type): the bar of tests/test_gpu_parity.py, 1e-3 abs — the fp8 kernel
                     adds no rounding of its own kind to the step (fp32 accumulation over exact code values) — and at least 8x
                     closer than to the oracle on the original K/V, which shows the step read the codes
  ids                equal to that oracle's argmax, or a tie by the rule of conftest.assert_ids_equal_or_tie: the oracle's top-2
                     margin at the step below twice the logit error measured at that step + 1e-4 (the slot stream too)
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

import cross_fp8_reference as R
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3  # tests/test_gpu_parity.py: logits against the bf16-policy oracle


def _mels(n, n_mels=80):
    """n distinct mels: the three of persist_cache_reference.mels (offsets of +-5 that move the cross K/V a lot), then seeded ones."""
    from make_model_goldens_inputs import synth_mel
    from persist_cache_reference import mels

    out = mels(n_mels)
    return (out + [synth_mel(40 + i, n_mels, 3000 - 97 * i) + np.float32(0.5 * (i % 5)) for i in range(n)])[:n]


def _dequantised(e, slot):
    """(k, v) float32 [L][1500][d] of the slot's stored codes and scales."""
    kc, vc, sc = e.get_cross_kv_fp8(slot)
    L, T, d = kc.shape
    return (R.dequantize(kc, sc[:, :, 0, :].reshape(L, d)).astype(np.float32), R.dequantize(vc, sc[:, :, 1, :].reshape(L, d)).astype(np.float32))


@pytest.fixture(scope="module")
def fp8_engine(built_lib, micro_case):
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=24, cross_kv="fp8")
    yield e
    e.close()


@pytest.fixture(scope="module")
def h16_engine(built_lib, micro_case):
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=4)
    yield e
    e.close()


def test_switch(built_lib, micro_case, fp8_engine, h16_engine, monkeypatch):
    assert fp8_engine.get_config_int("cross_kv_fp8") == 1 and h16_engine.get_config_int("cross_kv_fp8") == 0
    assert h16_engine.get_config_int("cross_kv_fp8_launches") == 0
    assert "AX_WHISPER_CROSS_KV" not in os.environ  # the constructor put the variable back
    with pytest.raises(RuntimeError, match="fp8"):
        h16_engine.get_cross_kv_fp8(0)
    with pytest.raises(RuntimeError, match="fp8"):
        h16_engine.cross_kv_quantize()
    monkeypatch.setenv("AX_WHISPER_CROSS_KV", "int4")
    with pytest.raises(RuntimeError, match="AX_WHISPER_CROSS_KV=int4"):
        built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=1)
    monkeypatch.setenv("AX_WHISPER_CROSS_KV", "h16")
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=1)
    assert e.get_config_int("cross_kv_fp8") == 0
    e.close()


def test_codes_and_scales_are_the_reference_quantisation(fp8_engine, h16_engine):
    mels = _mels(3)
    fp8_engine.encode_mel(np.stack(mels))
    h16_engine.encode_mel(np.stack(mels))
    for slot in range(3):
        k, v = fp8_engine.get_cross_kv(slot)
        k0, v0 = h16_engine.get_cross_kv(slot)
        assert np.array_equal(k.view(np.uint32), k0.view(np.uint32)) and np.array_equal(v.view(np.uint32), v0.view(np.uint32))  # the h16 images stay
        kc, vc, sc = fp8_engine.get_cross_kv_fp8(slot)
        L, T, d = k.shape
        for name, x, codes, scales in (("K", k, kc, sc[:, :, 0, :]), ("V", v, vc, sc[:, :, 1, :])):
            want, e = R.quantize(x)
            assert np.array_equal(scales.reshape(L, d).view(np.uint32), R.scales_of(e).view(np.uint32)), (slot, name)
            assert np.array_equal(codes, want), (slot, name, int((codes != want).sum()))
    # the kernel alone, again, over every slot: the same bytes
    before = fp8_engine.get_cross_kv_fp8(1)
    fp8_engine.cross_kv_quantize()
    after = fp8_engine.get_cross_kv_fp8(1)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def _forced_against_oracle(e, case, mels, lang, n_forced, check_slots, branches, what):
    """decode_forced of len(mels) clips on the fp8 handle e; the clips of check_slots against the oracle on their dequantised and on
    their original K/V. Returns (worst error to the dequantised oracle, to the original one, ties)."""
    B, L = len(mels), e.n_text_layer
    e.encode_mel(np.stack(mels))
    forced = np.array([[1000 + 37 * b + 11 * i for i in range(n_forced)] for b in range(B)], dtype=np.int32)
    n0 = e.get_config_int("cross_kv_fp8_launches")
    logits, am = e.decode_forced(B, forced)
    steps = 4 + n_forced
    assert e.get_config_int("cross_kv_fp8_launches") - n0 == L * branches * steps, (what, e.get_config_int("cross_kv_fp8_launches") - n0, L, branches, steps)
    worst_deq, worst_orig, ties = 0.0, 0.0, 0
    for b in check_slots:
        kd, vd = _dequantised(e, b)
        k, v = e.get_cross_kv(b)
        _, lg = case.oracle_bf16.greedy(kd, vd, lang, max_new=n_forced, forced=forced[b].tolist(), want_logits=True)
        _, lg0 = case.oracle_bf16.greedy(k, v, lang, max_new=n_forced, forced=forced[b].tolist(), want_logits=True)
        err = np.abs(logits[b] - lg).max(axis=1)
        err0 = np.abs(logits[b] - lg0).max()
        worst_deq, worst_orig = max(worst_deq, float(err.max())), max(worst_orig, float(err0))
        srt = np.sort(lg, axis=1)
        margin = srt[:, -1] - srt[:, -2]
        for s in range(lg.shape[0]):
            if am[b, s] != int(lg[s].argmax()):
                ties += 1
                assert margin[s] < 2 * err[s] + 1e-4, (what, b, s, float(margin[s]), float(err[s]))
    print(f"{what}: logits err to the oracle on dequantised K/V {worst_deq:.3e}, on the original K/V {worst_orig:.3e} "
          f"(x{worst_orig / max(worst_deq, 1e-30):.0f}), ties {ties}")
    assert worst_deq < LOGIT_TOL, what
    assert worst_orig >= 8 * worst_deq, what
    return worst_deq, worst_orig, ties


def test_forced_5_clips_one_branch_folded_query(fp8_engine, micro_case):
    _forced_against_oracle(fp8_engine, micro_case, _mels(5), "zh", 6, range(5), 1, "5 clips")


def test_forced_24_clips_two_branches_fused_query(fp8_engine, micro_case):
    _forced_against_oracle(fp8_engine, micro_case, _mels(24), "zh", 5, (0, 1, 15, 16, 23), 2, "24 clips")


def test_forced_miniturbo_split_k_query_from_a_buffer(built_lib, oracle_mod, tmp_path, monkeypatch):
    """AX_WHISPER_BATCHED_LN=0: the split-K sequence, whose cross-attention reads q from a buffer (in splits at 4 clips)."""
    case = ModelCase(tmp_path, "miniturbo", 21)
    monkeypatch.setenv("AX_WHISPER_BATCHED_LN", "0")
    e = built_lib.Whisper("miniturbo", case.root, "yue", device=0, max_batch=4, cross_kv="fp8")
    try:
        assert e.get_config_int("batched_ln") == 0 and e.get_config_int("cross_kv_fp8") == 1
        _forced_against_oracle(e, case, _mels(4, 128), "yue", 5, range(4), 1, "miniturbo, 4 clips")
    finally:
        e.close()


def test_one_and_two_clips_are_unchanged(fp8_engine, h16_engine):
    mels = _mels(2)
    for B in (1, 2):
        fp8_engine.encode_mel(np.stack(mels[:B]))
        h16_engine.encode_mel(np.stack(mels[:B]))
        n0 = fp8_engine.get_config_int("cross_kv_fp8_launches")
        got, want = fp8_engine.decode_greedy(B, max_new=12), h16_engine.decode_greedy(B, max_new=12)
        assert [list(x) for x in got] == [list(x) for x in want]
        assert fp8_engine.get_config_int("cross_kv_fp8_launches") == n0  # the persistent launches and the GEMV family read h16


def test_slot_stream_reads_each_slots_codes(fp8_engine, micro_case):
    """4 slots, 6 clips: every clip's ids against the oracle on the K/V its slot held when it finished."""
    import modelgen

    pcm = load_demo_pcm()
    clips = [pcm, pcm[8000:], 0.5 * pcm] + [modelgen.synth_clip(i, 160000 + 20000 * i) for i in range(1, 4)]
    max_new = 10
    e = fp8_engine
    n0 = e.get_config_int("cross_kv_fp8_launches")
    e.stream_open(4)
    got, kv, where = {}, {}, {}
    try:
        pending = list(range(len(clips)))
        idle = [0, 1, 2, 3]
        while len(got) < len(clips):
            while pending and idle:
                sl, c = idle.pop(0), pending.pop(0)
                e.stream_admit(sl, clips[c], max_new)
                where[sl] = c
            for sl in e.stream_step(4):
                kv[where[sl]] = _dequantised(e, sl)
                got[where[sl]] = e.stream_collect(sl)
                idle.append(sl)
    finally:
        e.stream_close()
    assert e.get_config_int("cross_kv_fp8_launches") > n0
    ties = 0
    for c in range(len(clips)):
        ids, lg = micro_case.oracle_bf16.greedy(kv[c][0], kv[c][1], "zh", max_new=max_new, want_logits=True)
        if got[c] == ids:
            continue
        # the first divergence as a tie, by the rule of conftest.assert_ids_equal_or_tie: the oracle's margin at that step against
        # twice the logit error MEASURED at that step — the clip encoded again into four slots of this handle (the batched fp8 step)
        # and teacher-forced with the oracle's ids, its row compared with the oracle's row on the stream slot's K/V
        n = min(len(got[c]), len(ids))
        i = next((i for i in range(n) if got[c][i] != ids[i]), n)
        assert i < n, (c, got[c], ids)
        e.encode_mel(np.stack([e.compute_mel(clips[c])] * 4))
        logits, _ = e.decode_forced(4, np.array([list(ids[:i])] * 4, dtype=np.int32).reshape(4, i))
        err = float(np.abs(logits[0, i] - lg[i]).max())
        srt = np.sort(lg[i])
        ties += 1
        assert srt[-1] - srt[-2] < 2 * err + 1e-4, (c, i, float(srt[-1] - srt[-2]), err, got[c], ids)
    print(f"slot stream: {len(clips)} clips, ties {ties}")
