"""GPU: resident vocabulary rows of the one-clip persistent launch (decode_persistent.hip, round 7).

The poller waves of every workgroup keep the tail of the workgroup's vocabulary rows in registers for the whole launch and
compute those logits themselves; the compute waves stream the rest. The design keeps the summation order of every row
(rows_dot<LD, CD>, group_sum<LD>), so the bar is BIT equality with the launch that streams every row
(AX_WHISPER_VOCAB_RESIDENT=0): a tolerance would hide a row computed twice, or by nobody."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

from conftest import ModelCase

pytestmark = pytest.mark.gpu


def _engine(wa, case, monkeypatch, resident):
    if resident:
        monkeypatch.delenv("AX_WHISPER_VOCAB_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("AX_WHISPER_VOCAB_RESIDENT", "0")
    try:
        return wa.Whisper(case.model_type, case.root, "zh", device=0, max_batch=1)  # the switch is read at construction
    finally:
        monkeypatch.delenv("AX_WHISPER_VOCAB_RESIDENT", raising=False)


def _rows(e):
    return e.L.AX_WHISPER_GetConfigInt(e.h, b"vocab_resident_rows")


# resident rows per workgroup: 6 passes of 512 / LD rows (LD = lanes per row: 16 at d_model 128 and 384, 32 at 256 and 768)
@pytest.mark.parametrize("model_type,seed,dtype,want_rows", [("micro", 41, "BF16", 192), ("mini", 42, "BF16", 96), ("tiny", 43, "BF16", 192),
                                                             ("small", 44, "BF16", 96), ("tiny", 45, "F16", 192)])
def test_forced_logits_bit_equal_with_and_without_resident_rows(built_lib, oracle_mod, tmp_path, monkeypatch, model_type, seed, dtype, want_rows):
    import modelgen

    case = ModelCase(tmp_path, model_type, seed, dtype=dtype)
    on, off = _engine(built_lib, case, monkeypatch, True), _engine(built_lib, case, monkeypatch, False)
    try:
        for e in (on, off):
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_decode") == 1
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"fp16") == (1 if dtype == "F16" else 0)
        assert _rows(on) == want_rows and _rows(off) == 0
        clip = modelgen.synth_clip(seed, 160000)
        # the teacher-forced history: the streaming launch's own greedy ids (28 steps; any ids would do)
        forced = off.run_tokens(clip, max_new=28)
        assert on.run_tokens(clip, max_new=28) == forced
        if len(forced) < 24:  # an early eot: pad with ordinary text ids, teacher forcing does not care
            forced = forced + [1000 + 7 * i for i in range(28 - len(forced))]
        mel, _, _ = oracle_mod.log_mel(clip, case.dims["n_mels"])
        res = []
        for e in (on, off):
            e.encode_mel(mel[None])
            res.append(e.decode_forced(1, np.array([forced])))
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_decode") == 1  # no give-up on the way
        (lg_on, am_on), (lg_off, am_off) = res
        assert lg_on.shape == (1, len(forced) + 1, case.dims["n_vocab"]) and len(forced) + 1 >= 24
        # every id of the vocabulary is covered: an entry that neither role wrote keeps what the buffer held before the launch
        # and cannot equal the streaming launch's logit in every one of 25+ steps
        assert np.isfinite(lg_on).all()
        diff = np.flatnonzero(lg_on.view(np.uint32) != lg_off.view(np.uint32))
        print(model_type, dtype, "resident rows", _rows(on), "entries that differ:", diff.size, "of", lg_on.size)
        assert np.array_equal(lg_on, lg_off)
        assert np.array_equal(am_on, am_off)
        assert np.array_equal(am_on[0], lg_on[0].argmax(axis=1))  # first max wins: np.argmax's rule
    finally:
        on.close()
        off.close()


def test_full_context_greedy_ids_equal_at_small(built_lib, oracle_mod, tmp_path, monkeypatch):
    import modelgen

    case = ModelCase(tmp_path, "small", 0)
    clip = modelgen.synth_clip(3, 160000)
    ids = []
    for resident in (True, False):
        e = _engine(built_lib, case, monkeypatch, resident)
        try:
            assert (_rows(e) > 0) == resident
            ids.append(e.run_tokens(clip))
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_decode") == 1
        finally:
            e.close()
    assert len(ids[0]) == 444, len(ids[0])  # synthetic weights never emit eot: the context limit ends the run
    assert ids[0] == ids[1]


def test_wide_model_keeps_no_resident_rows(built_lib, oracle_mod, tmp_path, monkeypatch):
    """d_model 1280: five chunks per lane and pass do not fit the poller waves' registers; the key says so and the launch is today's."""
    case = ModelCase(tmp_path, "w1280", 46)
    e = _engine(built_lib, case, monkeypatch, True)
    try:
        assert _rows(e) == 0
    finally:
        e.close()
