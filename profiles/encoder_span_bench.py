"""The encoder over each clip's own span (DESIGN.md "Encoder spans") against the default handle: Whisper-small dims, synthetic weights,
one MI355X, Bench("encoder") (ms per pass of N clips, ITERS passes between two events). One process per handle, the modes alternating
(ROUNDS processes each); every figure is the median over the rounds with [min .. max].

  full            default handle: all 1500 frames, today's kernels
  enc             cross_span="encoder", every clip at AX_WHISPER_BENCH_CROSS_SPAN = 1500, 750, 300 frames and one mixed run (spans uniform
                  in 150 .. 1500); the block height chosen by the engine's rule
  enc-64 / enc-128  the same with AX_WHISPER_ENC_SPAN_ROWS forced: the 64- against the 128-row choice

    python profiles/encoder_span_bench.py > profiles/encoder_span_bench.txt
"""
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))

MDIR = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
ROUNDS = int(os.environ.get("AXW_BENCH_ROUNDS", "3"))
ITERS = 5
CLIPS = (1, 4, 16, 64)
SPANS = ("1500", "750", "300", "mixed")
MODES = ("full", "enc", "enc-64", "enc-128")


def child(mode):
    import whisper_axera_amd as wa

    if mode.startswith("enc-"):
        os.environ["AX_WHISPER_ENC_SPAN_ROWS"] = mode[4:]
    e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=64, cross_span="full" if mode == "full" else "encoder")
    for n in CLIPS:
        for s in SPANS if mode != "full" else ("1500",):
            os.environ["AX_WHISPER_BENCH_CROSS_SPAN"] = s
            n0 = e.get_config_int("encoder_span_passes")
            e.bench("encoder", n, 0, 2)
            ms = e.bench("encoder", n, 0, ITERS) / ITERS
            assert (e.get_config_int("encoder_span_passes") > n0) == (mode != "full")
            print(f"RESULT\t{n} clips, span {s}\t{ms:.6f}", flush=True)
    e.close()


def main():
    import modelgen

    if not os.path.exists(os.path.join(MDIR, "small", "small.safetensors")):
        modelgen.write_model_dir(MDIR, "small", seed=0)
    res = {m: {} for m in MODES}
    for _ in range(ROUNDS):
        for mode in MODES:  # a fresh process per handle, the modes alternating
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", mode], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"child {mode} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT\t"):
                    _, k, v = ln.split("\t")
                    res[mode].setdefault(k, []).append(float(v))
    fmt = lambda a: f"{np.median(a):8.3f} [{min(a):.3f} .. {max(a):.3f}]"
    print(f"# small dims, Bench(encoder), {ITERS} passes per figure, {ROUNDS} processes per mode alternating ({' / '.join(MODES)}): ms per pass, "
          f"median [min .. max]; x: against the default handle's full pass of as many clips", flush=True)
    for n in CLIPS:
        base = res["full"][f"{n} clips, span 1500"]
        print(f"{n:3d} clips   full {fmt(base)}", flush=True)
        for s in SPANS:
            line = f"    span {s:>5}"
            for m in MODES[1:]:
                a = res[m][f"{n} clips, span {s}"]
                line += f"   {m} {fmt(a)} x{np.median(a) / np.median(base):.3f}"
            print(line, flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        main()
