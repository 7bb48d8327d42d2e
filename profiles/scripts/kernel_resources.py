#!/usr/bin/env python3
"""Register / LDS / spill table of every HIP kernel of the engine (hipcc --offload-arch=gfx950 -S, no GPU needed):
    python profiles/scripts/kernel_resources.py [--f16] > profiles/rNN_kernel_resources.txt
Columns from the code-object metadata: vgpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count, private (scratch) bytes,
static LDS bytes. tests/test_kernel_resources.py asserts the scratch / VGPR-spill columns are zero.

    python profiles/scripts/kernel_resources.py --parent DIR > profiles/NAME_kernel_resources.txt
compares this tree with another checkout's csrc directory (DIR = its whisper.axera_amd/csrc), both builds, the Makefile's flags:
one line per kernel with the six columns of either tree, marked `<< waves` where the waves-per-SIMD bucket changes (512 unified
VGPRs per SIMD, allocated in granules of 8, at most 8 waves) and `*` where any column differs.
`--files decode_timestamps,decode_beam` keeps either form to those kernel files."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")
FILES = ["frontend", "gemm", "encoder_attn", "decoder", "decode_gemv", "decode_gemm", "decode_persistent", "decode_persistent2", "decode_timestamps", "decode_beam"]
if "--files" in sys.argv:
    FILES = sys.argv[sys.argv.index("--files") + 1].split(",")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]  # whisper.axera_amd/Makefile HIPFLAGS
KEYS = ["vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]


def resources(csrc, name, f16):
    """[(demangled kernel name, [six columns])] of one kernel file, in the file's own order."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, name + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I" + os.path.join(ROOT, "include"), f"-DAXW_F16={f16}",
                        "--cuda-device-only", "-S", "-o", out, os.path.join(csrc, name + ".hip")], check=True, capture_output=True)
        text = open(out).read()
    rows = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        def g(k):
            m = re.search(r"\." + k + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        sym = g("name")
        try:
            dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip() or sym
        except OSError:
            dem = sym
        dem = re.sub(r"\(.*", "", dem).replace("void ", "").replace("axw::bf::", "").replace("axw::hf::", "")
        rows.append((dem, [g(k) for k in KEYS]))
    return rows


def waves(vgpr):
    return min(8, 512 // max(8, (int(vgpr) + 7) // 8 * 8))


def main():
    if "--parent" not in sys.argv:
        f16 = "1" if "--f16" in sys.argv else "0"
        print(f"# hipcc --offload-arch=gfx950 -O3 -DAXW_F16={f16}; kernel | vgpr | sgpr | vgpr spills | sgpr spills | scratch B | static LDS B")
        for name in FILES:
            print(f"## {name}.hip")
            for dem, cols in resources(CSRC, name, f16):
                print(" | ".join([dem] + cols))
        return
    parent = sys.argv[sys.argv.index("--parent") + 1]
    jobs = [(c, n, f) for f in ("0", "1") for n in FILES for c in (parent, CSRC)]
    with ThreadPoolExecutor(max_workers=int(os.environ.get("JOBS", "6"))) as ex:
        res = dict(zip(jobs, ex.map(lambda j: resources(*j), jobs)))
    print("# hipcc " + " ".join(FLAGS) + "; kernel | parent: vgpr sgpr vgpr-spills sgpr-spills scratch-B LDS-B | this tree: the same | marks")
    print("# marks: `*` a column differs, `<< waves a -> b` the waves-per-SIMD bucket changes (512 VGPRs per SIMD, granules of 8, at most 8)")
    changed, moved = 0, []
    for f16 in ("0", "1"):
        for name in FILES:
            print(f"## {name}.hip -DAXW_F16={f16}")
            old, new = res[(parent, name, f16)], dict(res[(CSRC, name, f16)])
            for dem, a in old:
                b = new.pop(dem, None)
                if b is None:
                    print(f"{dem} | {' '.join(a)} | (gone)")
                    continue
                mark = ""
                if a != b:
                    mark = " | *"
                    changed += 1
                if waves(a[0]) != waves(b[0]):
                    mark += f" << waves {waves(a[0])} -> {waves(b[0])}"
                    moved.append(f"{name}.hip F16={f16} {dem}")
                print(f"{dem} | {' '.join(a)} | {' '.join(b)}{mark}")
            for dem, b in new.items():
                print(f"{dem} | (new) | {' '.join(b)}")
    print(f"# {changed} kernels with a changed column; waves-per-SIMD bucket changed in {len(moved)}: {', '.join(moved) if moved else 'none'}")


if __name__ == "__main__":
    main()
