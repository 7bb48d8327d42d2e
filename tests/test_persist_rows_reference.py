"""CPU: the references, bounds and lane maps of tests/persist_rows_reference.py are held against themselves before a GPU sees them.

Emulation: a numpy float32 emulation of rows_dot / run_ln / gelu_erf / the fold chain / the reductions in the kernels' association
order must stay within every derived bound on every family; a family that exceeded one would show a wrong derivation. Discrimination:
on every case of the GPU test each named defect moves the float64 reference by at least 8 x the largest bound used on that case, in
a row of every workgroup (a head of every fold): a bound loose enough to hide such a defect fails here, without a GPU. Row dealing:
the Python mirror of RowSet::prefetch partitions [0, N) for every (N, P, first) the GPU test launches. Build: the driver
cross-compiles for gfx950 in both dtype builds, so a drift of decode_persistent_common.hpp breaks on a CPU machine."""
import numpy as np
import pytest

import kernel_driver
import persist_rows_reference as PR

DTS = ("bf16", "f16")
_cases = {}


def rows_case(dt, shape, name, N, family):
    key = (dt, shape, name)
    if key not in _cases:
        _cases.clear()  # one at a time: the widest holds W [3840][5120] in float64 more than once
        _cases[key] = PR.RowsCase(dt, shape[0], shape[1], N, family, PR.rows_seed(shape[0], shape[1], name))
    return _cases[key]


def test_the_shape_table_is_the_dispatch_s():
    assert len(PR.ROW_SHAPES) == 11 and len(set(PR.ROW_SHAPES)) == 11
    assert set(PR.ROW_SHAPES_D) == {(16, 1), (32, 1), (16, 3), (32, 2), (32, 3), (32, 5)}
    assert set(PR.ROW_SHAPES_F) == {(64, 2), (64, 3), (64, 4), (64, 6), (64, 10)}
    for d, (LD, CD, LF, CF) in PR.SHAPES.items():
        assert 8 * LD * CD == d and 8 * LF * CF == 4 * d
    assert PR.LAY["PT"] == 1024 and PR.CT + PR.PL == PR.LAY["PT"] and PR.qfold_stride(128) == 128 * 128 + 17 * 128


def test_reductions_emulated():
    vs, kinds = PR.reduce_vectors()
    worst = PR.check_reduce(vs, kinds, PR.emu_reduce(vs))
    print("reductions, emulation: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    # a butterfly without its permlane16 step: caught by the integer vectors
    bad = PR.emu_reduce(vs)
    bad[:, 1] = PR.emu_group_sum(vs, 16)
    with pytest.raises(AssertionError):
        PR.check_reduce(vs, kinds, bad)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", PR.ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_emulation_within_every_bound(dt, shape):
    """96 rows per family: the bounds are per row, so fewer rows check no less."""
    for fi, family in enumerate(PR.FAMILIES):
        case = PR.RowsCase(dt, shape[0], shape[1], 96, family, 77 + fi)
        worst = PR.check_rows_values(case, case.emulate(), f"{dt} {shape} {family}")
        amp = case.amplification
        print(f"{dt} ({shape[0]}, {shape[1]}) {family}: emulation worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
              + f"; |mean s| rstd / |result| median {np.median(amp):.2f} max {amp.max():.1f}")


def test_erff_of_the_emulation():
    ulps = PR.erff_ulps()
    print(f"this machine's float32 erf against float64 on [-4, 4]: {ulps:.2f} u (the bound budgets {PR.ERFF_ULPS} u for the device library's)")
    assert ulps <= PR.ERFF_ULPS


@pytest.mark.parametrize("shape", PR.ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_dealing(shape, built_lib):
    LPR, CH = shape
    slots = PR.CT // LPR
    seen = set()
    for name, N, family, deal_list in PR.rows_plan(LPR, CH):
        for P, NS, first in deal_list:
            own = PR.deals(N, P, first, LPR, NS)
            n = own[:, 1] - own[:, 0]
            rows = np.concatenate([np.arange(a, b) for a, b in own])
            assert np.array_equal(np.sort(rows), np.arange(N)), (shape, N, P, first)
            assert (n <= 2 * slots).all() and (n <= 64).all() and PR.deal_allowed(N, P, first, LPR, NS)
            if first < 0:
                seen |= set(n.tolist())
            else:
                assert set(n.tolist()) <= {0, slots, N % slots or slots}  # a packed deal: full passes, one remainder, or nothing
    grids, want = PR.even_grids(3 * (8 * LPR * CH if shape in PR.ROW_SHAPES_D else 2 * LPR * CH), LPR)
    assert 1 <= len(grids) <= 3 and {w for w in want if w is not None} <= seen, (want, seen)
    assert any(slots < c < 2 * slots for c in seen) or want[1] is None  # a second pass that only some slots run
    if shape in PR.ROW_SHAPES_D:  # the launch's own grid and free workgroups (AX_WHISPER_PersistentDecodePlan exposes no producer counts)
        d = 8 * LPR * CH
        p = built_lib.persistent_decode_plan(d, d // 64, 2, 256)
        assert p["grid"] == PR.grid_of(d) and p["free_workgroups"] == p["grid"] - 2 * (d // 64)
        pk, counts = PR.producers(d, p["grid"])
        assert counts["NP_D"] * slots >= d and pk["qkv"][2] == p["grid"] - counts["NP_Q"]


def test_vocabulary_deal_and_refusals():
    for N, P in PR.VOCAB_DEALS:
        own = PR.deals(N, P, -1, 16)
        assert own[0, 0] == 0 and own[-1, 1] == N and (own[1:, 0] == own[:-1, 1]).all()
    assert not PR.deal_allowed(3 * 128, 4, -1, 16)       # 96 rows a workgroup: more than 2 * SLOTS = 64
    assert not PR.deal_allowed(3 * 768, 17, -1, 32)      # 135 rows
    assert not PR.deal_allowed(3 * 128, 8, 0, 16)        # a packed deal with fewer workgroups than passes
    assert PR.deal_allowed(3 * 128, 128, 116, 16)


def _moved(case, what, P, NS, first, scale=8.0):
    """Per phase the defect touches: does every workgroup (with rows the defect reaches) hold a row moved by scale x the largest bound?"""
    slots = PR.CT // case.LPR
    out = {}
    for p, ref2 in case.perturbed(what, P, first, NS).items():
        big = max(case.bound[p].max(), case.bound_b.max() if p == 2 else 0.0)
        move = np.abs(ref2 - (case.ref[p] if p != 3 else case.pre3))
        ok = []
        for r0, r1 in PR.deals(case.N, P, first, case.LPR, NS):
            lo = r0 + slots if what == "bias_of_first_pass" else r0
            if lo < r1:
                ok.append(move[lo:r1].max() >= scale * big)
        out[p] = (all(ok), len(ok), float(move.max() / big))
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", PR.ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_defects_move_the_reference(dt, shape):
    for name, N, family, deal_list in PR.rows_plan(*shape):
        case = rows_case(dt, shape, name, N, family)
        for P, NS, first in deal_list:
            for what in ("drop_mean_s", "bias_of_first_pass", "swap_chunks", "drop_last_lane"):
                for p, (ok, n, ratio) in _moved(case, what, P, NS, first).items():
                    assert ok, f"{dt} {shape} {name} {family} P {P} first {first}: {what} hides below 8 x the bound of phase {PR.PHASES[p]} in some workgroup (largest move {ratio:.1f} bounds)"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", PR.FOLD_WIDTHS)
def test_fold_emulation_and_defects(dt, d):
    for ci, (family, shift_kind) in enumerate(PR.FOLD_CASES):
        case = PR.FoldCase(dt, d, family, shift_kind, 300 + d + ci)
        qd = case.definition()[0]
        assert np.abs(PR.fold_perturbed(case) - qd).max() <= 1e-9 * np.abs(qd).max()  # the identity itself, in float64
        worst, info = PR.check_fold(case, case.emulate(), f"{dt} d {d} {family} {shift_kind}")
        print(f"{dt} fold d {d} {family} shift {shift_kind}: emulation worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items() if "/" not in k)
              + f"; median |mu s| r / |q| {worst['|mu s| / |q|']:.2f}")
        big = max(info["eq"].max(), info["eqd"].max())
        for what in ("drop_mean_s", "drop_d", "attn_g_in_M"):
            move = np.abs(PR.fold_perturbed(case, what) - qd).reshape(d // 64, 64).max(axis=1)
            assert (move >= 8 * big).all(), f"{dt} d {d} {family} {shift_kind}: {what} moves a head by only {move.min() / big:.1f} bounds"


def test_arena_reference_tells_the_roles_apart():
    """The LayerNorm vectors of the three roles are drawn independently: an arena built with the attention LayerNorm's gain in M, or
    with s_qkv from the MLP LayerNorm, is far outside the bound."""
    _, layers = PR.arena_case("bf16", 128, 2, 9)
    for l, (wl, fl) in enumerate(layers):
        ref, bound = PR.arena_layer_expect(wl, fl, 128)
        fl2 = fl.copy()
        fl2[[PR.LAY["F_CROSS_LN_W"], PR.LAY["F_ATTN_LN_W"]]] = fl[[PR.LAY["F_ATTN_LN_W"], PR.LAY["F_CROSS_LN_W"]]]
        ref2, _ = PR.arena_layer_expect(wl, fl2, 128)
        assert np.median(np.abs(ref2 - ref)[:128 * 128] / bound[:128 * 128]) > 1000
        good = ref.astype(np.float32)
        assert PR.check_arena([(wl, fl)], 128, good) <= 1
    with pytest.raises(AssertionError):
        PR.check_arena([(layers[0][0], layers[1][1])], 128, PR.arena_layer_expect(*layers[0], 128)[0].astype(np.float32))


@pytest.mark.parametrize("dt", DTS)
def test_driver_cross_compiles(dt, built_lib):
    exe = kernel_driver.driver_exe(dt, source="persist_rows_driver.cpp", linked=PR.LINKED, also=PR.ALSO)
    assert exe.endswith("persist_rows_driver." + dt)
