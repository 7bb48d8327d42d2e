"""CPU: the rules instantiations of the one-clip persistent launch (decode_persistent_kernel<..., RULES = 1>), compiled
for gfx950 in both builds: no scratch, no VGPR spills, at most 128 VGPRs (1024-thread workgroups), and SGPR spills at most 15 % above
the plain instantiation of the same shape in the same build — the headroom convention of tests/test_kernel_resources.py, whose own
ceilings cover the new names as well."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")


@pytest.fixture(scope="module", params=[0, 1], ids=["bf16", "fp16"])
def kernels(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("pts_asm") / f"decode_persistent.{request.param}.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={request.param}", "--cuda-device-only", "-S", "-o", str(out), os.path.join(CSRC, "decode_persistent.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]  # noqa: E731
    cols = [field(k) for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count")]
    assert names and all(len(c) == len(names) for c in cols)
    return {n: dict(scratch=a, vspill=b, sspill=c, vgprs=d) for n, a, b, c, d in zip(names, *cols) if "decode_persistent_kernel" in n}


def _shape(name):
    """template arguments of a mangled kernel name: (LD, CD, LF, CF, PROF, QF, RULES)"""
    m = re.search(r"decode_persistent_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)EEE", name)
    assert m, name
    return tuple(int(x) for x in m.groups())


def test_rules_instantiations(kernels):
    by_shape = {_shape(n): k for n, k in kernels.items()}
    rules = {s: k for s, k in by_shape.items() if s[6] == 1}
    # every shape of the launch, folded where the plain launch is folded; no timeline build
    assert sorted(s[:4] for s in rules if s[5] == 0) == sorted({s[:4] for s in by_shape})
    assert sorted(s[:4] for s in rules if s[5] == 1) == sorted({s[:4] for s in by_shape if s[5] == 1 and s[6] == 0})
    assert all(s[4] == 0 for s in rules)
    for s, k in sorted(rules.items()):
        plain = by_shape[s[:6] + (0,)]
        print(s, k, "plain SGPR spills", plain["sspill"])
        assert k["scratch"] == 0 and k["vspill"] == 0, (s, k)
        assert k["vgprs"] <= 128, (s, k)
        assert k["sspill"] <= plain["sspill"] * 1.15, (s, k["sspill"], plain["sspill"])
