"""GPU: beam search on a handle with cross_kv="fp8" AND beam_cross="shared" (DESIGN.md "Shared cross K/V over FP8 codes"), checked by
test_gpu_beam._check_reorder: candidates and selection exact against beam_reference.py, every record teacher-forced on the SAME handle
in a batch of at least three clips (the existing FP8 step, same codes) under the copy path's bars. Both launch counters rise."""
import numpy as np
import pytest

import test_gpu_beam as tb

pytestmark = pytest.mark.gpu
COUNTERS = ("beam_cross_shared_launches", "cross_kv_fp8_launches")


class AtLeastThree:
    """A handle whose encode and teacher-forced decode are padded to three clips: a batch the FP8 step serves (two keep the GEMV family)."""

    def __init__(self, e):
        self._e = e

    def __getattr__(self, name):
        return getattr(self._e, name)

    def encode_mel(self, mels):
        return self._e.encode_mel(np.concatenate([mels, np.repeat(mels[-1:], max(0, 3 - len(mels)), axis=0)]))

    def decode_forced_timestamp_scores(self, clips, forced, **kw):
        n = max(clips, 3)
        return self._e.decode_forced_timestamp_scores(n, np.concatenate([forced, np.repeat(forced[-1:], n - clips, axis=0)]), **kw)


class BothModel(tb.Model):
    """tb.Model whose one engine is a handle with both modes: the traced beam calls and the teacher-forced side run on it."""

    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        super().__init__(built_lib, tmp, model_type, seed, dtype)
        self.e.close()
        self.e = AtLeastThree(built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=25, cross_kv="fp8", beam_cross="shared"))
        self.launches = {}

    def traced(self, clips, K, max_new=tb.MAX_NEW):
        key = (clips, K, max_new)
        if key not in self._traced:
            self.e.encode_mel(np.stack(self.mels[:clips]))
            before = [self.e.get_config_int(c) for c in COUNTERS]
            self._traced[key] = self.e.decode_beam(clips, K, max_new, trace=True)
            self.launches[key] = [self.e.get_config_int(c) - b for c, b in zip(COUNTERS, before)]
        return self._traced[key]


@pytest.fixture(scope="module")
def micro(built_lib, oracle_mod, tmp_path_factory):
    m = BothModel(built_lib, tmp_path_factory.mktemp("beam_shared_fp8_micro"), "micro", 11, "BF16")
    yield m
    m.e.close()


# test_gpu_beam_shared_cross.py's sizes: 5, 10 slots one branch (folded query); 24, 25 two (fused); at 5 x 5 the boundary cuts clip 3
@pytest.mark.parametrize("clips,K,branches", [(1, 5, 1), (2, 5, 1), (3, 8, 2), (5, 5, 2)], ids=["1x5", "2x5", "3x8_branches", "5x5_cut_group"])
def test_shared_fp8_beam_is_the_same_handles_teacher_forced_decode(micro, clips, K, branches):
    assert micro.e.get_config_int("beam_cross_shared") == 1 and micro.e.get_config_int("cross_kv_fp8") == 1
    tb._check_reorder(micro, clips, K, tb.MAX_NEW, "shared fp8 cross %d x %d" % (clips, K))
    assert micro.launches[clips, K, tb.MAX_NEW] == [micro.e.n_text_layer * (tb.MAX_NEW + 2) * branches] * 2


def test_split_k_sequence_on_miniturbo(built_lib, oracle_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("AX_WHISPER_BATCHED_LN", "0")  # the split-K sequence, whose cross-attention reads q from a buffer
    m = BothModel(built_lib, tmp_path, "miniturbo", 21, "F16")
    try:
        assert m.e.get_config_int("batched_ln") == 0
        tb._check_reorder(m, 2, 5, tb.MAX_NEW, "shared fp8 cross, split-K sequence, 2 x 5")
        assert m.launches[2, 5, tb.MAX_NEW] == [m.e.n_text_layer * (tb.MAX_NEW + 2)] * 2
    finally:
        m.e.close()


@pytest.mark.parametrize("modes", [dict(cross_kv="fp8"), dict(beam_cross="shared")], ids=["fp8_only", "shared_only"])
def test_one_mode_alone_keeps_its_own_route(micro, built_lib, modes):
    e = built_lib.Whisper("micro", micro.case.root, "zh", device=0, max_batch=10, **modes)
    try:
        e.encode_mel(np.stack(micro.mels[:2]))
        e.decode_beam(2, 5, tb.MAX_NEW)
        got = [e.get_config_int(c) for c in COUNTERS]
        # an FP8 handle's beam call keeps h16 copies (neither counter moves); a shared handle's takes the h16 grouped kernel
        assert got == ([0, 0] if "cross_kv" in modes else [e.n_text_layer * (tb.MAX_NEW + 2), 0])
    finally:
        e.close()
