"""CPU: the FP8 cross K/V kernels (csrc/cross_kv_fp8.hip) compile for gfx950, in both builds, without scratch memory or register
spills (tests/test_kernel_resources.py says why that is a test), convert with the packed OCP instructions, and the attention kernel
keeps the registers that leave two workgroups of the widest instantiation (three of the others) on a CU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills(f16, tmp_path):
    out = tmp_path / "cross_kv_fp8.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "cross_kv_fp8.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    n = len(names)
    # the quantise kernel and the attention kernel's query modes: q from a buffer, fused (generic and d_model 384 / 512 / 768 / 1024), folded
    assert sum("cross_kv_quantize_kernel" in x for x in names) == 1 and sum("decode_cross_attention_fp8_kernel" in x for x in names) == 7, names
    assert field("private_segment_fixed_size") == [0] * n and field("vgpr_spill_count") == [0] * n and field("sgpr_spill_count") == [0] * n
    for name, vg in zip(names, field("vgpr_count")):
        assert vg <= (64 if "quantize" in name else 256), (name, vg)
        if "fp8_kernelILi1ELi32" not in name and "fp8_kernelILi1ELi24" not in name and "quantize" not in name:
            assert vg <= 168, (name, vg)  # three workgroups per CU
    assert "v_cvt_pk_f32_fp8" in text and "v_cvt_pk_fp8_f32" in text and "v_pk_fma_f32" in text
