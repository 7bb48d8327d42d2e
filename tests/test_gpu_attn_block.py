"""GPU: the persistent launches' 64-key attention block alone (tests/cpp/attn_block_driver.cpp) against the float64 block and the
derived bound of tests/attn_block_reference.py — both dtype builds, both forms of the block (the matrix-pipe form and the
vector-pipe form behind AXW_ATTN_MFMA=0, held to the SAME bound), both V homes and the register-held block.

Every valid-key count of VALID_COUNTS runs on every wave (eight rotations over the eight waves, so each on wave 0 and on wave 7);
the scratch area is pre-filled with NaN; the query has a 30x outlier dim; K rows of masked keys hold +- the type's largest value
or NaN bit patterns, V rows of masked keys are finite."""
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
pytestmark = pytest.mark.gpu


def driver_exe(dt, mfma):
    """build/attn_block_driver.<dt>.<form of the block>, rebuilt whenever it is older than its sources."""
    exe = os.path.join(BUILD, f"attn_block_driver.{dt}.{'mfma' if mfma else 'valu'}")
    srcs = [os.path.join(ROOT, "tests", "cpp", "attn_block_driver.cpp")] + [os.path.join(PKG, "csrc", f) for f in
                                                                           ("decode_persistent_common.hpp", "common.hpp", "decode_layout.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(f) for f in srcs):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DAXW_F16=" + ("1" if dt == "f16" else "0"), f"-DAXW_ATTN_MFMA={int(mfma)}",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), srcs[0], "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module", params=["bf16", "f16"])
def cases(request):
    """The inputs of one dtype build, shared by both forms of the block: (dt, [(form, nw, case, expected records)])."""
    dt, out = request.param, []
    for gi, garbage in enumerate(("huge", "nan")):
        for rot in range(8):
            counts = A.VALID_COUNTS[rot:] + A.VALID_COUNTS[:rot]
            case = A.make_case(dt, 100 + 8 * gi + rot, counts, garbage)
            exp = [A.block_expect(case["q_hi"], case["q_lo"], case["k"][w], case["v"][w], n) for w, n in enumerate(counts)]
            for form in ("rows", "vt", "regs"):
                out.append((form, 8, case, exp))
    out += [(form, nw, case, exp) for form in ("rows", "vt", "regs") for nw in (1, 3)]  # fewer waves: the other records stay untouched
    return dt, out


def run_driver(exe, cases, tmp_path):
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for form, nw, case, _ in cases:
            K, V = A.lds_images(case, "rows" if form == "rows" else "vt")
            f.write(np.array([A.FORMS[form], nw] + list(case["counts"]), dtype=np.int32).tobytes())
            f.write(np.uint32(SENT).tobytes())
            f.write(case["q_packed"].astype(np.uint32).tobytes())
            f.write(K.tobytes())
            f.write(V.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
    return np.fromfile(fout, dtype=np.float32).reshape(len(cases), 8, 66)


@pytest.mark.parametrize("mfma", [True, False], ids=["matrix-pipe", "vector-pipe"])
def test_block_against_float64(cases, mfma, tmp_path):
    dt, cs = cases
    got = run_driver(driver_exe(dt, mfma), cs, tmp_path)
    worst, by_vt = {}, {}
    for ci, (form, nw, case, exp) in enumerate(cs):
        for w in range(8):
            name = f"{dt} {'mfma' if mfma else 'valu'} {form} case {ci} wave {w} of {nw} keys {case['counts'][w]}"
            if w >= nw:
                assert (got[ci, w].view(np.uint32) == SENT).all(), f"{name}: a record of a wave that did not run changed"
                continue
            worst[form] = max(worst.get(form, 0.0), A.check_record(name, got[ci, w], exp[w], dt))
        # the register-held block follows its LDS twin in the case list: the same inputs, the same bits
        if form == "vt":
            by_vt[id(case), nw] = got[ci, :nw]
        if form == "regs":
            assert np.array_equal(by_vt[id(case), nw].view(np.uint32), got[ci, :nw].view(np.uint32)), f"{dt} case {ci}: registers and LDS differ"
    for form, w in sorted(worst.items()):
        print(f"{dt} {'matrix-pipe' if mfma else 'vector-pipe'} {form}: worst error / bound {w:.4f}")
