"""CPU: the chunked long-form kernels (csrc/long_cuts.hip) compile for gfx950, in both builds, without scratch memory or register
spills (tests/test_kernel_resources.py says why that is a test), and stay within the registers and the LDS of their build (DESIGN.md
"Chunked long-form": the levels kernel keeps 384 levels in LDS, the plan kernel one (value, frame) pair per wave, the window kernel's
tile is dynamic). Only the resource metadata is read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")

#            VGPRs, SGPRs, static LDS bytes: ceilings a little above what the build takes (VGPRs and SGPRs in steps of 8; the levels
#            kernel holds two frames' loads at once: 29 VGPRs, still eight waves per SIMD)
CEILINGS = {"long_levels": (32, 40, 1536), "long_cut_plan": (24, 48, 32), "long_cut_compact": (16, 32, 0), "mel_window_cut": (40, 48, 0)}


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills_and_ceilings(f16, tmp_path):
    out = tmp_path / "long_cuts.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "long_cuts.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    short = [next(k for k in CEILINGS if k + "_kernel" in n) for n in names]
    assert sorted(short) == sorted(CEILINGS)
    n = len(names)
    assert field("private_segment_fixed_size") == [0] * n and field("vgpr_spill_count") == [0] * n and field("sgpr_spill_count") == [0] * n
    for i, k in enumerate(short):
        vg, sg, lds = CEILINGS[k]
        got = (field("vgpr_count")[i], field("sgpr_count")[i], field("group_segment_fixed_size")[i])
        print(k, got)
        assert got[0] <= vg and got[1] <= sg and got[2] == lds, (k, got)
    # the levels kernel's traffic over the store: 1 + 2 R / tile <= 1.25 at the default R = 25 (tile 256, halo up to 64 each side)
    assert CEILINGS["long_levels"][2] == (256 + 2 * 64) * 4 and 1 + 2 * 25 / 256 <= 1.25
