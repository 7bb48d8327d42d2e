"""Language detection: the prefill route (the layers of one decoder step + language_detect_kernel) against the step-fed route (one
decoder step with the logits dump, the pick on the host) — DESIGN.md "Language and task per clip". Bench("detect_language") on
Whisper-small dims (synthetic weights, bf16) at 1, 8 and 64 clips. Every figure comes from a FRESH process (--one), the two routes alternating,
AXW_BENCH_ROUNDS rounds (default 5), medians. One timed call is AX_WHISPER_DetectLanguageStage's work: reset, the [sot] position,
the pick, the results on the host, with the host synchronisations the engine makes.

    python profiles/lang_detect_bench.py [clips ...] > profiles/lang_detect_bench.txt
    python profiles/lang_detect_bench.py --one prefill|step CLIPS ITERS     # one route alone, one process
The kernel's own time: a kernel trace of one route alone with nothing else traced, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/lang_detect_bench.py --one prefill 8 20
and the language_detect_kernel line of OUT's kernel statistics."""
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
ROUTES = {"prefill": 0, "step": 1}


def engine(max_batch):
    import modelgen
    import whisper_axera_amd as wa

    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    return wa.Whisper("small", mdir, "zh", device=0, max_batch=max_batch)


def one(route, B, iters):
    e = engine(B)
    e.bench("detect_language", B, ROUTES[route], 2)  # warm: scratch, code objects
    ms = e.bench("detect_language", B, ROUTES[route], iters) / iters
    e.close()
    return ms


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        route, B, iters = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        print("%s clips %d: %.4f ms per call" % (route, B, one(route, B, iters)))
        sys.exit(0)
    clips = [int(x) for x in (sys.argv[1:] or ["1", "8", "64"])]
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    engine(1).close()  # the model directory exists before the first timed process
    for B in clips:
        got = {r: [] for r in ROUTES}
        for _ in range(rounds):
            for r in ROUTES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", r, str(B), "20"], capture_output=True, text=True, check=True).stdout
                got[r].append(float(out.split(":")[1].split()[0]))
        a, b = float(np.median(got["prefill"])), float(np.median(got["step"]))
        print(f"clips {B:3d}: prefill route {a:8.4f} ms, step-fed route {b:8.4f} ms ({b / a:5.2f} x)"
              f"  (rounds: {[['%.4f' % x for x in got[r]] for r in ROUTES]})", flush=True)
