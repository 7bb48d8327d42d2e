"""CPU: the span cross-attention kernels (csrc/decode_attention_span.hip) compile for gfx950, in both builds, without scratch memory
or register spills (tests/test_kernel_resources.py says why that is a test), and the attention kernel stays within the registers and
the LDS DESIGN.md "Cross-attention spans" states for it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_no_scratch_no_spills(f16, tmp_path):
    out = tmp_path / "decode_attention_span.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "decode_attention_span.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    n = len(names)
    # plan, span set, and the attention kernel: {h16, fp8} x {q from a buffer, fused: generic and d_model 384 / 512 / 768 / 1024}
    assert sum("cross_span_plan_kernel" in x for x in names) == 1 and sum("cross_span_set_kernel" in x for x in names) == 1
    assert sum("decode_cross_attention_span_kernel" in x for x in names) == 12 and n == 14, names
    assert field("private_segment_fixed_size") == [0] * n and field("vgpr_spill_count") == [0] * n and field("sgpr_spill_count") == [0] * n
    for name, vg, lds in zip(names, field("vgpr_count"), field("group_segment_fixed_size")):
        if "attention" not in name:
            continue
        fp8, read = "ILb1E" in name, "ELi0ELi0E" in name
        assert lds == (1312 if read else 5440), (name, lds)  # 4 wave records + the query (+ the LayerNormed row of the fused projection)
        # two workgroups per CU at the widest projection (d_model 1024: 32 weight chunks per lane), three from d_model 768 down over
        # the code images, and the read-query instantiations at 128 registers or fewer
        assert vg <= (128 if read else 192 if fp8 else 224), (name, vg)
        if fp8 and "ELi32E" not in name:
            assert vg <= 168, (name, vg)
