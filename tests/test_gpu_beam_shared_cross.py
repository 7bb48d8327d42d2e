"""GPU: beam search over ONE cross K/V copy per clip (DESIGN.md "Shared cross K/V"). decode_beam(trace=True) runs on a beam_cross="shared"
handle and is checked by tests/test_gpu_beam.py's own _check_reorder: candidates and selection exact against tests/beam_reference.py on
the traced rows, every record teacher-forced on a DEFAULT handle under the copy path's bars (rows 5e-3, log-probabilities 2 err + 1e-4)."""
import numpy as np
import pytest

import test_gpu_beam as tb

pytestmark = pytest.mark.gpu


class SharedModel(tb.Model):
    """tb.Model (its engine `e` is a default handle: the teacher-forced side) whose traced beam calls run on a shared-cross handle."""

    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        super().__init__(built_lib, tmp, model_type, seed, dtype)
        self.shared = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=25, beam_cross="shared")
        self.launches = {}

    def traced(self, clips, K, max_new=tb.MAX_NEW):
        key = (clips, K, max_new)
        if key not in self._traced:
            self.shared.encode_mel(np.stack(self.mels[:clips]))
            before = self.shared.get_config_int("beam_cross_shared_launches")
            self._traced[key] = self.shared.decode_beam(clips, K, max_new, trace=True)
            self.launches[key] = self.shared.get_config_int("beam_cross_shared_launches") - before
        return self._traced[key]


@pytest.fixture(scope="module")
def micro(built_lib, oracle_mod, tmp_path_factory):
    m = SharedModel(built_lib, tmp_path_factory.mktemp("beam_shared_micro"), "micro", 11, "BF16")
    yield m
    m.shared.close(), m.e.close()


# 5, 10 slots: one branch, folded query; 24, 25: branches of 16 + rest, fused query; at 5 x 5 the boundary cuts clip 3 (slots 15 .. 19)
@pytest.mark.parametrize("clips,K,branches", [(1, 5, 1), (2, 5, 1), (3, 8, 2), (5, 5, 2)], ids=["1x5", "2x5", "3x8_branches", "5x5_cut_group"])
def test_shared_beam_is_the_default_handles_teacher_forced_decode(micro, clips, K, branches):
    assert micro.shared.get_config_int("beam_cross_shared") == 1 and micro.e.get_config_int("beam_cross_shared") == 0
    tb._check_reorder(micro, clips, K, tb.MAX_NEW, "shared cross %d x %d" % (clips, K))
    assert micro.launches[clips, K, tb.MAX_NEW] == micro.e.n_text_layer * (tb.MAX_NEW + 2) * branches


def test_split_k_sequence_on_miniturbo(built_lib, oracle_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("AX_WHISPER_BATCHED_LN", "0")  # the split-K sequence, whose cross-attention reads q from a buffer
    m = SharedModel(built_lib, tmp_path, "miniturbo", 21, "F16")
    try:
        assert m.shared.get_config_int("batched_ln") == 0
        tb._check_reorder(m, 2, 5, tb.MAX_NEW, "shared cross, split-K sequence, 2 x 5")
        assert m.launches[2, 5, tb.MAX_NEW] == m.e.n_text_layer * (tb.MAX_NEW + 2)
    finally:
        m.shared.close(), m.e.close()


def test_counters_the_default_handle_and_a_bad_value(micro, built_lib, monkeypatch):
    micro.traced(1, 2)  # the GEMV family: a copy per slot as ever
    assert micro.launches[1, 2, tb.MAX_NEW] == 0
    with pytest.raises(RuntimeError, match="AX_WHISPER_BEAM_CROSS=both: expected copy or shared"):
        built_lib.Whisper("micro", micro.case.root, "zh", device=0, max_batch=1, beam_cross="both")
    # a default handle launches no grouped kernel, and says what a handle opened under =copy says, bit for bit
    monkeypatch.setenv("AX_WHISPER_BEAM_CROSS", "copy")
    other = built_lib.Whisper("micro", micro.case.root, "zh", device=0, max_batch=24)
    try:
        got = []
        for e in (micro.e, other):
            e.encode_mel(np.stack(micro.mels[:2]))
            got.append(e.decode_beam(2, 5, tb.MAX_NEW, trace=True))
            assert e.get_config_int("beam_cross_shared") == 0 and e.get_config_int("beam_cross_shared_launches") == 0
        assert np.array_equal(got[0][1]["rows"], got[1][1]["rows"]) and [r["ids"] for r in got[0][0]] == [r["ids"] for r in got[1][0]]
    finally:
        other.close()
