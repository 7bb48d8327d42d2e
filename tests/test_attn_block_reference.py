"""CPU: the operand maps and the bound of tests/attn_block_reference.py (the persistent launches' 64-key attention block on the
matrix pipe). The GPU side is tests/test_gpu_attn_block.py."""
import os
import subprocess

import numpy as np
import pytest

import attn_block_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """csrc/decode_layout.hpp's own index functions, printed by tests/cpp/decode_layout_tables.cpp built with g++."""
    exe = tmp_path_factory.mktemp("layout") / "decode_layout_tables"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "whisper.axera_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "decode_layout_tables.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in out.splitlines()}


def test_maps_agree_with_the_layout_header(tables):
    key, dim = np.arange(64)[:, None], np.arange(64)[None, :]
    k, v, vt = (tables[n].reshape(448, 64) for n in ("k", "v", "vt"))
    chunk = tables["kv_chunk"].reshape(7, 8, 64)
    for blk in (0, 3):  # block offsets are whole blocks: the in-block maps repeat
        assert np.array_equal(k[64 * blk:64 * blk + 64] - 4096 * blk, A.k_offset(key, dim))
        assert np.array_equal(vt[64 * blk:64 * blk + 64] - 4096 * blk, A.vt_offset(key, dim))
        assert np.array_equal(v[64 * blk:64 * blk + 64] - 4096 * blk, A.v_offset(key, dim))
    for b in range(4):
        for ks in range(2):
            row, kk, piece = A.b_piece(b, ks)
            # the piece is kv_chunk_offset(blk, 4 ks + lane / 16, 16 b + lane % 16) ...
            assert np.array_equal(piece, chunk[0, 4 * ks + A.LANES // 16, 16 * b + A.LANES % 16])
            at = piece[:, None] + np.arange(8)
            # ... and holds, of the blocked K, (key = row, dim = k); of the transposed V, (dim = row, key = k)
            assert np.array_equal(at, k[row, kk]) and np.array_equal(at, vt[kk, row])
            # row-major V through the two transposed reads: the same (key, dim) elements
            assert np.array_equal(A.b_rows(b, ks), v[kk, row])
            for a in A.b_rows_addresses(b, ks):
                assert (a % 4 == 0).all() and a.min() >= 0 and a.max() + 4 <= 4096  # 8-byte aligned, inside the block
    for ks in range(2):
        w = A.a_words(ks)
        assert w.min() >= 0 and w.max() < 64 and (w[:, 0] % 4 == 0).all()  # 16-byte aligned, inside the 64 packed dwords
        # element j of lane l is value 32 ks + 8 (l / 16) + j of the hi (even rows) or lo (odd rows) half
        val = 2 * (w % 32)[:, :, None] + np.arange(2)
        assert np.array_equal(val.reshape(64, 8), (32 * ks + 8 * (A.LANES // 16))[:, None] + np.arange(8))
        assert np.array_equal(w[:, 0] // 32, A.LANES % 2)


@pytest.mark.parametrize("form", ["vt", "rows"])
def test_every_pair_is_covered_exactly_once(form):
    """Over the four blocks and two k-steps, the sixteen (row, k) pairs of a lane's two fragments cover all 64 x 64 (key, dim)
    pairs once; within ONE (block, k-step) the 64 lanes' 8 elements are 512 distinct elements."""
    seen_k = np.zeros((64, 64), dtype=int)
    seen_v = np.zeros(4096, dtype=int)
    for b in range(4):
        for ks in range(2):
            row, kk, piece = A.b_piece(b, ks)
            np.add.at(seen_k, (row, kk), 1)
            at = A.b_rows(b, ks) if form == "rows" else piece[:, None] + np.arange(8)
            assert len(np.unique(at)) == 512
            np.add.at(seen_v, at.ravel(), 1)
    assert (seen_k == 1).all() and (seen_v == 1).all()
    # the result: lane l's two registers are rows 4 (l / 16), + 1 (hi and lo of ONE query) of column l % 16 of accumulator l / 16
    acc = np.zeros((4, 16, 16))
    for g in range(4):
        acc[g, 4 * g, :] = 16 * g + np.arange(16)
        acc[g, 4 * g + 1, :] = 1000
    assert np.array_equal(A.pick(acc), A.LANES + 1000)


@pytest.mark.parametrize("garbage", ["huge", "nan"])
@pytest.mark.parametrize("form", ["vt", "rows"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_emulation_with_exact_operands_stays_inside_the_bound(dt, form, garbage):
    worst = 0.0
    for seed, counts in ((1, A.VALID_COUNTS), (2, A.VALID_COUNTS[::-1])):
        case = A.make_case(dt, seed, counts, garbage)
        K, V = A.lds_images(case, form)
        for w, n in enumerate(counts):
            m, l, o = A.emulate(form, case["q_packed"], K[w], V[w], n, dt)
            r = A.block_expect(case["q_hi"], case["q_lo"], case["k"][w], case["v"][w], n)
            worst = max(worst, A.check_record(f"{dt} {form} wave {w} keys {n}", np.concatenate([[m, l], o]), r, dt))
    print(f"{dt} {form} {garbage}: emulation error / bound {worst:.3f}")
    assert worst > 0  # the bound is not vacuous: the emulation's roundings show


def test_a_wrong_map_fails():
    """The check can fail: the output read with the two transposed reads swapped (keys +4 first) leaves the bound."""
    dt = "bf16"
    case = A.make_case(dt, 3, A.VALID_COUNTS, "huge")
    K, V = A.lds_images(case, "rows")
    orig = A.b_rows
    try:
        A.b_rows = lambda nb, ks: orig(nb, ks)[:, [4, 5, 6, 7, 0, 1, 2, 3]]
        m, l, o = A.emulate("rows", case["q_packed"], K[7], V[7], 64, dt)
    finally:
        A.b_rows = orig
    r = A.block_expect(case["q_hi"], case["q_lo"], case["k"][7], case["v"][7], 64)
    with pytest.raises(AssertionError):
        A.check_record("swapped", np.concatenate([[m, l], o]), r, dt)
