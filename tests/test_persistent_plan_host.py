"""CPU: which decode path a decoder shape gets, and who runs which cross-attention unit in a persistent launch.

Init decides silently, from the model's shape and the device's CU count, between the one-clip persistent launch, the two- and
three-clip launches and the launch-per-phase paths (decode_persistent.hip: decode_persistent_grid / _supported / _max_clips),
and the kernels deal the cross-attention units of every layer to the workgroups without a self-attention head with ca_unit_of
(decode_persistent_common.hpp). AX_WHISPER_PersistentDecodePlan hands exactly those functions to the host, so this file checks
the product's own code, not a restatement: the depth edges of DESIGN.md "Which decode path a model shape gets" as literals,
the assignment's invariants for every supported (d_model, layers, clips) on 64 / 128 / 256 / 304 CUs, and which launches have
a workgroup with units in CONSECUTIVE layers (the K tiles of the next unit are then staged behind this layer's attention
block, decode_persistent2.hip) — tests/test_gpu_model_depths.py must run one such model per width."""
import numpy as np
import pytest

WIDTHS = {128: 2, 256: 4, 384: 6, 512: 8, 768: 12, 1280: 20}   # persist_dispatch: d_model -> heads (head_dim 64)
CUS = (64, 128, 256, 304)
# 256 CUs: d_model -> (deepest decoder with 3 clips per launch, deepest with the persistent launch, first that falls back)
EDGES_256 = {128: (55, 58, 59), 256: (55, 58, 59), 384: (33, 36, 37), 512: (23, 26, 27), 768: (12, 15, 16), 1280: (None, 6, 7)}
# 256 CUs: the shallowest decoder whose launch has a workgroup with units in consecutive layers: d_model -> {clips: layers}
CONSECUTIVE_FROM_256 = {128: {2: 53, 3: 47}, 256: {2: 53, 3: 47}, 384: {2: 31, 3: 25}, 512: {2: 21, 3: 15}, 768: {2: 10, 3: 4}}


@pytest.fixture(scope="module")
def plan(built_lib):
    return built_lib.persistent_decode_plan


def test_depth_edges_on_256_cus(plan):
    for n_cu in (256, 304):   # the launch never has more than 256 workgroups
        for d, H in WIDTHS.items():
            deep3, deep, first_off = EDGES_256[d]
            for L in range(1, 65):
                p = plan(d, H, L, n_cu)
                assert p["grid"] == min(256, d) and p["free_workgroups"] == p["grid"] - L * H
                want_clips = 0 if L >= first_off else (1 if d > 768 else (3 if L <= deep3 else 2))
                assert (p["supported"], p["max_clips"]) == (L <= deep, want_clips), (n_cu, d, L, p)
            assert first_off == deep + 1
    assert not plan(1024, 16, 2, 256)["supported"]      # no instantiation at this width
    assert not plan(768, 6, 2, 256)["supported"]        # head_dim 128


def _consecutive(units):
    owned = units >= 0
    return bool((owned[:-1] & owned[1:]).any())


def test_every_unit_has_one_owner_per_layer(plan):
    n_launches = 0
    for n_cu in CUS:
        for d, H in WIDTHS.items():
            for L in range(1, 65):
                p = plan(d, H, L, n_cu)
                if not p["supported"]:
                    assert p["max_clips"] == 0
                    continue
                # the rule itself (out of scope to change; pinned so that a change shows up here)
                assert p["free_workgroups"] >= 2 * 3 * H and 1 <= p["max_clips"] <= 3
                assert p["max_clips"] == 1 or (d <= 768 and p["free_workgroups"] >= p["max_clips"] * 3 * H)
                for nc in range(1, p["max_clips"] + 1):
                    nu = nc * 3 * H
                    # 4 decode steps of L layers each: the assignment runs on over the step boundaries
                    u = plan(d, H, L, n_cu, n_clips=nc, t0=0, n_slots=4 * L)["units"]
                    assert u.shape == (4 * L, p["grid"])
                    assert (u[:, p["free_workgroups"]:] == -1).all()   # a self-attention owner takes no unit
                    assert u.min() >= -1 and u.max() == nu - 1
                    # every unit 0 .. nu-1 exactly once per layer slot (one value per workgroup and slot: nobody owns two)
                    assert (np.sort(np.where(u < 0, nu, u), axis=1)[:, :nu] == np.arange(nu)).all(), (n_cu, d, L, nc)
                    assert ((u >= 0).sum(axis=1) == nu).all()
                    if nc == 1:   # the one-clip launch stages the next unit's tiles a layer AHEAD: never in consecutive layers
                        assert not _consecutive(u), (n_cu, d, L)
                    # the window is part of one endless sequence: another offset gives the same rows
                    assert (plan(d, H, L, n_cu, n_clips=nc, t0=3 * L - 1, n_slots=2)["units"] == u[3 * L - 1:3 * L + 1]).all()
                    n_launches += 1
    assert n_launches > 1000
    with pytest.raises(RuntimeError):   # units of a launch the shape does not get
        plan(1280, 20, 6, 256, n_clips=2, t0=0, n_slots=4)
    with pytest.raises(RuntimeError):
        plan(768, 12, 16, 256, n_clips=1, t0=0, n_slots=4)


def test_which_launches_have_consecutive_layer_owners(plan):
    for d, H in WIDTHS.items():
        for L in range(1, 65):
            p = plan(d, H, L, 256)
            for nc in range(2, p["max_clips"] + 1):
                got = _consecutive(plan(d, H, L, 256, n_clips=nc, t0=0, n_slots=4 * L)["units"])
                assert got == (L >= CONSECUTIVE_FROM_256[d][nc]), (d, L, nc, got)


def test_the_gpu_suite_runs_a_consecutive_layer_launch_per_width(plan):
    """tests/test_gpu_model_depths.py names, per width with a multi-clip launch, the models whose two- and three-clip launches
    have consecutive-layer owners (the equality test of that file runs them): checked here against the product's assignment."""
    import test_gpu_model_depths as gpu

    assert set(gpu.CONSECUTIVE_LAYER_MODELS) == {128, 256, 384, 512, 768}
    specs = {s.name: s for s in gpu.DEPTH_EDGE_MODELS}
    for d, by_clips in gpu.CONSECUTIVE_LAYER_MODELS.items():
        assert set(by_clips) == {2, 3}
        for nc, name in by_clips.items():
            s = specs[name]
            assert s.d == d and s.persistent == 1 and s.max_clips >= nc
            assert _consecutive(plan(d, WIDTHS[d], s.layers, 256, n_clips=nc, t0=0, n_slots=4 * s.layers)["units"]), (name, nc)
    # and the literals of that file's dispatch table are the product's answers
    for s in gpu.DEPTH_EDGE_MODELS:
        p = plan(s.d, WIDTHS[s.d], s.layers, 256)
        assert (int(p["supported"]), max(p["max_clips"], 1)) == (s.persistent, s.max_clips), s.name
