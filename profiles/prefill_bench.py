"""Prompt prefill: the prefill pass against the step-fed route (DESIGN.md "Prompt conditioning"). Bench("prefill_pass") and
Bench("prefill_step") on ONE handle (Whisper-small dims, synthetic weights, bf16), every slot with a context of L positions, at
L = 64 and 226 and 1, 8 and 64 clips; the two routes alternate, AXW_BENCH_ROUNDS rounds (default 5), medians. One timed call is
reset + prefill_prompts: the table upload, the route, the no-speech row and the hand-over, with the host synchronisations the
engine makes (hipEvents around the whole call, so host gaps count: it is what a prompted window pays before its first decision).
The step-fed route enqueues its L decoder steps launch by launch (it is not captured into a graph).

    python profiles/prefill_bench.py [clips ...] > profiles/prefill_bench.txt
    python profiles/prefill_bench.py --one pass|step CLIPS L ITERS     # one route alone (for a profiler run)"""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))


def engine(max_batch):
    import modelgen
    import whisper_axera_amd as wa

    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    return wa.Whisper("small", mdir, "zh", device=0, max_batch=max_batch)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        route, B, L, iters = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
        e = engine(B)
        print("%s clips %d L %d: %.3f ms per call" % (route, B, L, e.bench("prefill_" + route, B, L, iters) / iters))
        e.close()
        sys.exit(0)
    clips = [int(x) for x in (sys.argv[1:] or ["1", "8", "64"])]
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    e = engine(max(clips))
    print("prefill route of the handle: %d (0 the prefill pass, 1 step-fed)" % e.get_config_int("prefill"))
    for B in clips:
        for L in (64, 226):
            it = {"pass": 10, "step": 2 if B * L > 4000 else 4}
            for r in it:  # warm: scratch, code objects
                e.bench("prefill_" + r, B, L, 1)
            got = {"pass": [], "step": []}
            for _ in range(rounds):
                for r in ("pass", "step"):
                    got[r].append(e.bench("prefill_" + r, B, L, it[r]) / it[r])
            a, b = float(np.median(got["pass"])), float(np.median(got["step"]))
            print(f"clips {B:3d} L {L:3d}: prefill pass {a:9.3f} ms, step-fed {b:9.3f} ms ({b / a:6.2f} x; {b / L:.3f} ms per fed position)"
                  f"  (rounds: {[['%.3f' % x for x in got[r]] for r in ('pass', 'step')]})", flush=True)
    e.close()
