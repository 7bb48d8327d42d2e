"""CPU: the reference side of tests/test_gpu_persistent_clips.py (tests/persist_cache_reference.py) on the oracle alone, micro/41.

What makes the GPU test bite is shown here without a GPU: the three mels give different ids, a neighbour's cross K/V moves every
layer >= 1 of a clip's cache by far more than the comparison's tolerance, and the comparison the GPU test uses refuses a cache
in which ONE row's K came from the neighbouring clip while it accepts the untouched cache and one that is a 16-bit spacing off."""
import numpy as np
import pytest

import persist_cache_reference as prc
from conftest import ModelCase

N_IDS = 70


@pytest.fixture(scope="module")
def clips(oracle_mod, tmp_path_factory):
    case = ModelCase(tmp_path_factory.mktemp("persist_cache_ref"), "micro", 41)
    orc = case.oracle_bf16
    kvs = [orc.encoder(m) for m in prc.mels(80)]
    idss = [orc.greedy(ck, cv, "zh", max_new=N_IDS) for ck, cv in kvs]
    own = [prc.forced_cache(orc, *kvs[i], idss[i]) for i in range(3)]
    return orc, kvs, idss, own


def test_mels_are_the_three_of_the_issue():
    demo, plus5, bins = prc.mels(80)
    assert all(m.shape == (80, 3000) and m.dtype == np.float32 for m in (demo, plus5, bins))
    assert (plus5 == 5.0).all()
    assert (bins[0::2] == 5.0).all() and (bins[1::2] == -5.0).all()
    assert float(demo.std()) > 0.1 and float(np.abs(demo).max()) < 5.0   # an ordinary log-mel, far from the two constants


def test_ulp16_at_and_around_powers_of_two():
    for dtype, m in (("BF16", 7), ("F16", 10)):
        for e in (-3, 0, 1, 4):
            p = 2.0 ** e
            assert prc.ulp16(p, dtype) == 2.0 ** (e - m)                                # at the power: the spacing ABOVE it
            assert prc.ulp16(-p, dtype) == 2.0 ** (e - m)
            assert prc.ulp16(np.nextafter(np.float32(p), np.float32(0)), dtype) == 2.0 ** (e - 1 - m)   # just below: half of it
            assert prc.ulp16(p * 1.999, dtype) == 2.0 ** (e - m)
            assert prc.ulp16(p * (1 + 2.0 ** -m), dtype) == 2.0 ** (e - m)               # the next representable value
        # zeros and subnormals: the floor, never 0
        assert prc.ulp16(0.0, dtype) == 2.0 ** (prc.FLOOR_EXP - m) == prc.ulp16(1e-30, dtype)
        r = np.array([[0.0, 1.0], [-2.5, 300.0]])
        assert prc.ulp16(r, dtype).shape == r.shape and (prc.ulp16(r, dtype) > 0).all()
    # against the types themselves: numpy's half, and bfloat16 as the upper half of a float32
    x = np.float16(1.7)
    assert prc.ulp16(float(x), "F16") == float(np.nextafter(x, np.float16(4))) - float(x)
    b = np.array([0x40490000], dtype=np.uint32)   # 3.140625 in bfloat16
    assert prc.ulp16(float(b.view(np.float32)[0]), "BF16") == float((b + 0x10000).view(np.float32)[0]) - float(b.view(np.float32)[0])


def test_forced_cache_rows_and_prefix(clips):
    orc, kvs, idss, own = clips
    k, v = own[0]
    assert k.shape == v.shape == (orc.m.n_text_layer, len(idss[0]) + 4, orc.m.n_text_state)
    # causal: the cache of a prefix of the ids is the prefix of the cache (the GPU test's unequal budgets rely on it)
    kp, vp = prc.forced_cache(orc, *kvs[0], idss[0][:9])
    assert np.array_equal(kp, k[:, :13]) and np.array_equal(vp, v[:, :13])
    # layer 0 depends on the ids only: the first four rows (the sot sequence) are common to all clips
    assert np.array_equal(own[0][0][0, :4], own[1][0][0, :4]) and np.array_equal(own[0][1][0, :4], own[2][1][0, :4])


def test_ids_differ_and_a_wrong_clip_moves_the_cache(clips):
    orc, kvs, idss, own = clips
    assert all(len(i) == N_IDS for i in idss)
    assert idss[0] != idss[1] and idss[1] != idss[2] and idss[0] != idss[2]
    sep_k, sep_v = prc.separation(orc, kvs, idss, own=own)
    print("micro/41: separation K %.3f, V %.3f" % (sep_k, sep_v))
    assert sep_k >= 0.5 and sep_v >= 0.5   # measured >= 0.7
    tol = max(prc.max_tolerance(own[i][j], "BF16", prc.A["BF16"]) for i in range(3) for j in range(2))
    assert min(sep_k, sep_v) >= 8 * tol, (sep_k, sep_v, tol)


def test_comparison_refuses_one_swapped_row(clips):
    orc, kvs, idss, own = clips
    a = prc.A["BF16"]
    ref_k, ref_v = own[0]
    assert prc.worst_ratio(ref_k, ref_k, "BF16", a) == 0.0
    # a cache one 16-bit spacing off everywhere (another rounding of nearly the same fp32 value) still passes
    off = ref_k + np.where(np.arange(ref_k.size).reshape(ref_k.shape) % 2 == 0, 1.0, -1.0) * prc.ulp16(ref_k, "BF16")
    assert prc.worst_ratio(off, ref_k, "BF16", a) <= 1.0
    # clip 0's ids decoded against the NEIGHBOURING clip's cross K/V: what a wrong cross_clip_stride would compute
    wrong_k, wrong_v = prc.forced_cache(orc, *kvs[1], idss[0])
    for layer in range(1, ref_k.shape[0]):
        row = 4 + int(np.abs(wrong_k[layer, 4:] - ref_k[layer, 4:]).max(axis=1).argmin())   # the LEAST telling row behind the sot sequence
        bad = ref_k.copy()
        bad[layer, row] = wrong_k[layer, row]
        r = prc.worst_ratio(bad, ref_k, "BF16", a)
        print("layer %d row %d: one swapped K row is %.1f x the tolerance" % (layer, row, r))
        assert r > 1.0, (layer, row, r)
        assert prc.worst_ratio(ref_v, ref_v, "BF16", a) == 0.0
    # a whole neighbour's cache (a wrong self_clip_stride would hand clip 1 clip 2's rows): its own ids, its own cross K/V
    assert prc.worst_ratio(own[1][0], ref_k, "BF16", a) > 1.0 and prc.worst_ratio(own[1][1], ref_v, "BF16", a) > 1.0
    # non-finite values never pass
    bad = ref_v.copy()
    bad[1, 5, 3] = np.nan
    assert prc.worst_ratio(bad, ref_v, "BF16", a) > 1.0
