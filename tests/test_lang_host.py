"""CPU: the language detection kernel's resources in both builds (no scratch, no spills)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_language_kernel_compiles_without_scratch_or_spills(f16, tmp_path):
    out = tmp_path / "lang.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out),
                        os.path.join(ROOT, "whisper.axera_amd", "csrc", "decode_language.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    assert sum("language_detect_kernel" in n for n in names) == 1, names
    assert re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M) == ["0"] * len(names)
    assert all(int(x) == 0 for x in re.findall(r"^\s+\.(?:vgpr|sgpr)_spill_count:\s+(\d+)", text, re.M))
    vg = dict(zip(names, (int(x) for x in re.findall(r"^\s+\.vgpr_count:\s+(\d+)", text, re.M))))
    assert all(v <= 128 for v in vg.values()), vg  # one 256-thread workgroup per clip: occupancy is not what bounds it
