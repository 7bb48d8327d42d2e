"""GPU: beam search over an ancestry table (DESIGN.md "Tree self-attention"). decode_beam(trace=True) runs on a beam_self="tree" handle
and is checked by tests/test_gpu_beam.py's own _check_reorder: candidates and selection exact against tests/beam_reference.py on the
traced rows, every record teacher-forced on a DEFAULT handle under the copy path's bars (rows 5e-3, log-probabilities 2 err + 1e-4).
A wrong origin entry reads another hypothesis' key and moves these models' logits by about 0.1."""
import numpy as np
import pytest

import test_gpu_beam as tb
from test_gpu_beam_shared_fp8 import AtLeastThree

pytestmark = pytest.mark.gpu
COUNTER = "beam_self_tree_launches"


class TreeModel(tb.Model):
    """tb.Model (its engine `e` is a default handle: the teacher-forced side) whose traced beam calls run on a tree handle; with `modes`
    the one engine is a handle with those modes too, padded to three clips, and both sides run on it."""

    def __init__(self, built_lib, tmp, model_type, seed, dtype, **modes):
        super().__init__(built_lib, tmp, model_type, seed, dtype)
        self.tree = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=25, beam_self="tree", **modes)
        if modes:
            self.e.close()
            self.e = self.tree = AtLeastThree(self.tree)
        self.launches = {}

    def traced(self, clips, K, max_new=tb.MAX_NEW):
        key = (clips, K, max_new)
        if key not in self._traced:
            self.tree.encode_mel(np.stack(self.mels[:clips]))
            before = self.tree.get_config_int(COUNTER)
            self._traced[key] = self.tree.decode_beam(clips, K, max_new, trace=True)
            self.launches[key] = self.tree.get_config_int(COUNTER) - before
        return self._traced[key]

    def close(self):
        self.tree.close()
        if self.e is not self.tree:
            self.e.close()


@pytest.fixture(scope="module")
def micro(built_lib, oracle_mod, tmp_path_factory):
    m = TreeModel(built_lib, tmp_path_factory.mktemp("beam_tree_micro"), "micro", 11, "BF16")
    yield m
    m.close()


# 5, 10 slots: one branch; 24, 25: branches of 16 + rest; at 5 x 5 the boundary cuts clip 3 (slots 15 .. 19), which both branches serve
@pytest.mark.parametrize("clips,K,branches", [(1, 5, 1), (2, 5, 1), (3, 8, 2), (5, 5, 2)], ids=["1x5", "2x5", "3x8_branches", "5x5_cut_group"])
def test_tree_beam_is_the_default_handles_teacher_forced_decode(micro, clips, K, branches):
    assert micro.tree.get_config_int("beam_self_tree") == 1 and micro.e.get_config_int("beam_self_tree") == 0
    tb._check_reorder(micro, clips, K, tb.MAX_NEW, "tree self %d x %d" % (clips, K))
    assert micro.launches[clips, K, tb.MAX_NEW] == micro.e.n_text_layer * (tb.MAX_NEW + 2) * branches


def test_slots_move_beyond_the_first_key_block(micro):
    trace = tb._check_reorder(micro, 1, 3, 70, "tree self 1 x 3, 70 ids")
    moved = [n for n in range(trace["n_steps"]) if (trace["src"][n] != np.arange(3)).any()]
    assert trace["n_steps"] == 70 and any(n + 2 > 64 for n in moved), moved  # decode offset = n + 2: origin rows of two key blocks


def test_split_k_sequence_on_miniturbo(built_lib, oracle_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("AX_WHISPER_BATCHED_LN", "0")
    m = TreeModel(built_lib, tmp_path, "miniturbo", 21, "F16")
    try:
        assert m.tree.get_config_int("batched_ln") == 0
        tb._check_reorder(m, 2, 5, tb.MAX_NEW, "tree self, split-K sequence, 2 x 5")
        assert m.launches[2, 5, tb.MAX_NEW] == m.e.n_text_layer * (tb.MAX_NEW + 2)
    finally:
        m.close()


def test_all_three_modes_on_one_handle(built_lib, oracle_mod, tmp_path):
    m = TreeModel(built_lib, tmp_path, "micro", 11, "BF16", cross_kv="fp8", beam_cross="shared")
    try:
        before = [m.e.get_config_int(c) for c in ("beam_cross_shared_launches", "cross_kv_fp8_launches")]
        tb._check_reorder(m, 5, 5, tb.MAX_NEW, "tree self + shared fp8 cross 5 x 5")
        n = m.e.n_text_layer * (tb.MAX_NEW + 2) * 2
        assert m.launches[5, 5, tb.MAX_NEW] == n and m.e.get_config_int("beam_cross_shared_launches") - before[0] == n
    finally:
        m.close()


def test_counters_the_default_handle_and_a_bad_value(micro, built_lib, monkeypatch):
    micro.traced(1, 2)  # the GEMV family: the copy path as ever, reorder included
    assert micro.launches[1, 2, tb.MAX_NEW] == 0
    with pytest.raises(RuntimeError, match="AX_WHISPER_BEAM_SELF=graph: expected copy or tree"):
        built_lib.Whisper("micro", micro.case.root, "zh", device=0, max_batch=1, beam_self="graph")
    # a default handle launches no tree kernel, and says what a handle opened under =copy says, bit for bit
    monkeypatch.setenv("AX_WHISPER_BEAM_SELF", "copy")
    other = built_lib.Whisper("micro", micro.case.root, "zh", device=0, max_batch=24)
    try:
        got = []
        for e in (micro.e, other):
            e.encode_mel(np.stack(micro.mels[:2]))
            got.append(e.decode_beam(2, 5, tb.MAX_NEW, trace=True))
            assert e.get_config_int("beam_self_tree") == 0 and e.get_config_int(COUNTER) == 0
        assert np.array_equal(got[0][1]["rows"], got[1][1]["rows"]) and [r["ids"] for r in got[0][0]] == [r["ids"] for r in got[1][0]]
    finally:
        other.close()
