"""CPU: the persistent launches' LDS image of a cross V block (csrc/decode_layout.hpp: cross_v_swizzle, cross_v_source_piece,
cross_v_read_base / cross_v_read_offset), printed by tests/cpp/cross_v_swizzle_table.cpp built with g++, against the map and the
LDS bank rule restated here.

The image: LDS slot (key row R, 16-byte chunk c) of the [64 keys][64 dims] block holds the block's chunk c ^ x(R),
x(R) = 2 (2 (R / 8 % 2) + R / 2 % 2). The reads: ds_read_b64_tr_b16, every lane supplies the address of 8 bytes = V[key][dim .. dim + 3]
with key = 32 ks + 8 (lane / 16) + lane / 4 % 4 + 4 half and dim = 16 nb + 4 (lane % 4). The bank rule of a 64-bit LDS read: the two
32-lane halves of a wave are served one after the other; inside a half every lane takes the two banks (a / 4) % 64 and + 1, and the
read costs as many passes as the most loaded bank has distinct addresses."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = np.arange(64)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = tmp_path_factory.mktemp("swizzle") / "cross_v_swizzle_table"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "whisper.axera_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "cross_v_swizzle_table.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    t = {}
    for ln in out.splitlines():
        w = ln.split()
        t[w[0], int(w[1])] = np.array(w[2:], dtype=np.int64)
    assert t["stage", 0].size == t["stage", 1].size == 512 and t["read", 0].size == t["read", 1].size == 16 * 64
    return t


def x_of(row):
    row = np.asarray(row)
    return 2 * (2 * ((row >> 3) & 1) + ((row >> 1) & 1))


def bank_passes(addr):
    """LDS passes of ONE 64-bit read of a wave: per 32-lane half, the most distinct 8-byte addresses on one bank."""
    worst = 0
    for half in (addr[:32], addr[32:]):
        on_bank = {}
        for a in half:
            for b in ((a // 4) % 64, (a // 4 + 1) % 64):
                on_bank.setdefault(int(b), set()).add(int(a))
        worst = max(worst, max(len(s) for s in on_bank.values()))
    return worst


@pytest.mark.parametrize("swz", [1, 0], ids=["swizzled", "plain"])
def test_staging_map_permutes_chunks_inside_a_row(tables, swz):
    src = tables["stage", swz]
    slot = np.arange(512)
    assert sorted(src) == list(range(512)), "not a bijection of the block's 512 pieces"
    assert np.array_equal(src >> 3, slot >> 3), "a piece left its 128-byte row"
    want = (slot & 7) ^ (x_of(slot >> 3) if swz else 0)
    assert np.array_equal(src & 7, want)
    if swz:
        assert set(x_of(np.arange(64))) == {0, 2, 4, 6}


@pytest.mark.parametrize("swz", [1, 0], ids=["swizzled", "plain"])
def test_reads_land_on_their_elements(tables, swz):
    """Every address is 8-byte aligned, inside the tile, and — through the staging map — holds V[key][dim .. dim + 3] of the key
    and dims the product's B operand wants from that lane."""
    src = tables["stage", swz]
    addr = tables["read", swz].reshape(4, 2, 2, 64)
    assert (addr % 8 == 0).all() and (addr >= 0).all() and (addr + 8 <= 8192).all()
    for nb in range(4):
        for ks in range(2):
            for half in range(2):
                a = addr[nb, ks, half]
                key = 32 * ks + 8 * (LANES // 16) + (LANES // 4) % 4 + 4 * half
                dim = 16 * nb + 4 * (LANES % 4)
                piece = src[a // 16]                              # the source piece the LDS piece at this address received
                got = piece * 8 + (a % 16) // 2                   # element of the row-major source block
                assert np.array_equal(got, key * 64 + dim), (nb, ks, half)


def test_swizzled_reads_are_conflict_free_and_plain_reads_are_four_way(tables):
    """32 LDS passes per block for the swizzled image (2 per read: the two halves), 128 for the plain one — the conflict this
    image is there for, seen by the same checker."""
    worst = {s: [bank_passes(a) for a in tables["read", s].reshape(16, 64)] for s in (0, 1)}
    assert max(worst[1]) == 1 and min(worst[1]) == 1, worst[1]
    assert max(worst[0]) == 4 and min(worst[0]) == 4, worst[0]
    cycles = {s: sum(2 * w for w in worst[s]) for s in (0, 1)}  # two halves per read
    assert cycles == {1: 32, 0: 128}
