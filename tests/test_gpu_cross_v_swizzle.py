"""GPU: the persistent launches' staging of cross K/V tiles through stage_cross_kv and the 64-key block on the swizzled V image
(tests/cpp/cross_tile_driver.cpp) — both dtype builds, both forms of the block (matrix pipe, and the vector-pipe form behind
AXW_ATTN_MFMA=0).

One workgroup of eight waves stages eight K/V blocks from global memory in the kernels' own piece splits (0,2) (2,8) (8,11) (11,13)
(13,16) and as one call, and runs the block on the image the helper leaves; the same inputs copied into LDS as they are run the
plain row-major block. The records of the two V homes must be the same bits (the same MFMAs / FMAs in the same order on the same
elements), and each within attn_block_reference.check_record's bound of the float64 block. Cases as in test_gpu_attn_block.py: every
valid-key count of VALID_COUNTS on every wave, K rows of masked keys "huge" or NaN patterns, the scratch area pre-filled with NaN."""
import os
import subprocess

import numpy as np
import pytest

import attn_block_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper.axera_amd")
BUILD = os.path.join(PKG, "build")
HIPCC = "/opt/rocm/bin/hipcc"
SENT = 0x7FC57FC5
MODES = {"plain": 0, "split": 1, "whole": 2}
pytestmark = pytest.mark.gpu


def driver_exe(dt, mfma):
    """build/cross_tile_driver.<dt>.<form of the block>, rebuilt whenever it is older than its sources."""
    exe = os.path.join(BUILD, f"cross_tile_driver.{dt}.{'mfma' if mfma else 'valu'}")
    srcs = [os.path.join(ROOT, "tests", "cpp", "cross_tile_driver.cpp")] + [os.path.join(PKG, "csrc", f) for f in
                                                                           ("decode_persistent_common.hpp", "common.hpp", "decode_layout.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(f) for f in srcs):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DAXW_F16=" + ("1" if dt == "f16" else "0"), f"-DAXW_ATTN_MFMA={int(mfma)}", "-DAXW_CROSS_V_SWIZZLE=1",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), srcs[0], "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module", params=["bf16", "f16"])
def cases(request):
    """The inputs of one dtype build, shared by both forms of the block: (dt, [(case, expected records)])."""
    dt, out = request.param, []
    for gi, garbage in enumerate(("huge", "nan")):
        for rot in range(8):
            counts = A.VALID_COUNTS[rot:] + A.VALID_COUNTS[:rot]
            case = A.make_case(dt, 300 + 8 * gi + rot, counts, garbage)
            out.append((case, [A.block_expect(case["q_hi"], case["q_lo"], case["k"][w], case["v"][w], n) for w, n in enumerate(counts)]))
    return dt, out


def run_driver(exe, cases, tmp_path):
    """[case][mode][8][66]: every case in every mode. The global images are the cross caches': blocked K, row-major V."""
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases) * len(MODES)).tobytes())
        for case, _ in cases:
            K, V = A.lds_images(case, "rows")
            for mode in MODES.values():
                f.write(np.array([mode, 8] + list(case["counts"]), dtype=np.int32).tobytes())
                f.write(np.uint32(SENT).tobytes())
                f.write(case["q_packed"].astype(np.uint32).tobytes())
                f.write(K.tobytes())
                f.write(V.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
    assert "swizzle=1" in r.stdout, r.stdout  # built with the swizzled image, whatever the library's default
    return np.fromfile(fout, dtype=np.float32).reshape(len(cases), len(MODES), 8, 66)


@pytest.mark.parametrize("mfma", [True, False], ids=["matrix-pipe", "vector-pipe"])
def test_swizzled_tile_gives_the_plain_tile_s_bits(cases, mfma, tmp_path):
    dt, cs = cases
    got = run_driver(driver_exe(dt, mfma), cs, tmp_path)
    worst = 0.0
    for ci, (case, exp) in enumerate(cs):
        for mode, mi in MODES.items():
            for w in range(8):
                name = f"{dt} {'mfma' if mfma else 'valu'} {mode} case {ci} wave {w} keys {case['counts'][w]}"
                worst = max(worst, A.check_record(name, got[ci, mi, w], exp[w], dt))
        for mode in ("split", "whole"):
            same = got[ci, MODES[mode]].view(np.uint32) == got[ci, MODES["plain"]].view(np.uint32)
            assert same.all(), f"{dt} case {ci}: staged {mode} and plain records differ in waves {sorted(set(np.nonzero(~same)[0]))}"
    print(f"{dt} {'matrix-pipe' if mfma else 'vector-pipe'}: worst error / bound {worst:.4f}")
