"""CPU: the resample kernel (csrc/resample.hip) compiles for gfx950, in both builds, without scratch memory or register spills
(tests/test_kernel_resources.py says why that is a test), and stays within the registers and the LDS of its build (DESIGN.md "Sample
rates": 34 VGPRs, 46 SGPRs, 46080 bytes of LDS = the 9472-float input span + the 2048-float table). Only the resource metadata is read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")

#            VGPRs, SGPRs, LDS bytes: ceilings a little above what the build takes (VGPRs and SGPRs in steps of 8)
CEILINGS = {"resample": (40, 56, 46080)}


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills_and_ceilings(f16, tmp_path):
    out = tmp_path / "resample.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "resample.hip")],
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
    # 160 KB of LDS per CU: three workgroups of this kernel fit a CU side by side
    assert 3 * CEILINGS["resample"][2] <= 160 * 1024
