"""A decoder step of the PARENT commit's library against this tree's, on any Bench target: ms per step at each batch size
(Whisper-small dims, synthetic weights), medians over rounds. Every round of every side is a fresh process that measures every
named target at every batch size; the sides alternate, the parent first. A point passes when this tree's median is not above
the parent's by more than the parent's own spread (max - min over its rounds).

    AXW_PARENT_LIB=/path/to/parent/libax_whisper.so python profiles/step_ab.py TARGET [TARGET ...] --batches 1,4,64 --arg 224

--arg is Bench's third argument: the decode offset of the decode_step_ts* targets, the beam size of decode_step_beam (whose batch
sizes are slots). AX_WHISPER_BENCH_TEMPERATURE, read by decode_step_ts_sampled, is passed on to both sides. --iters (default 50)
steps per timed region, AXW_BENCH_ROUNDS (default 5) rounds."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(R, "whisper.axera_amd", "lib", "libax_whisper.so")


def measure(lib_path, targets, batches, arg, iters):
    """{target: {batch: ms per step}} from the library at lib_path (this process loads exactly one library)"""
    sys.path.insert(0, R)
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen
    import whisper_axera_amd as wa

    wa.LIB_PATH = lib_path
    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=max(batches))
    out = {}
    for name in targets:
        out[name] = {}
        for B in batches:
            e.bench(name, B, arg, iters)  # (the first call captures the graph)
            out[name][B] = e.bench(name, B, arg, iters) / iters
    e.close()
    return out


def child(lib, a):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, *a.targets, "--batches", a.batches, "--arg", str(a.arg),
                        "--iters", str(a.iters)], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise SystemExit("round failed (%s):\n" % lib + p.stdout[-2000:] + p.stderr[-2000:])
    return json.loads(line[0][7:])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("targets", nargs="+")
    ap.add_argument("--batches", default="1,4,64")
    ap.add_argument("--arg", type=int, default=224)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.targets, batches, a.arg, a.iters)))
        sys.exit(0)
    parent = os.environ["AXW_PARENT_LIB"]
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    got = {side: {t: {B: [] for B in batches} for t in a.targets} for side in ("parent", "tree")}
    for r in range(rounds):
        for side, lib in (("parent", parent), ("tree", TREE_LIB)):
            for t, by_batch in child(lib, a).items():
                for B, v in by_batch.items():
                    got[side][t][int(B)].append(v)
    temp = os.environ.get("AX_WHISPER_BENCH_TEMPERATURE")
    print(f"# arg {a.arg}, {a.iters} steps per timed region, {rounds} rounds" + (f", AX_WHISPER_BENCH_TEMPERATURE={temp}" if temp is not None else ""))
    fmt = lambda v: " ".join("%.4f" % x for x in v)
    for t in a.targets:
        for B in batches:
            p, q = got["parent"][t][B], got["tree"][t][B]
            mp, mq, spread = float(np.median(p)), float(np.median(q)), max(p) - min(p)
            print(f"{t} B {B:3d}: parent median {mp:.4f} ms (spread {spread:.4f}; {fmt(p)}), tree median {mq:.4f} ms ({fmt(q)}), "
                  f"tree - parent {mq - mp:+.4f}: {'pass' if mq - mp <= spread else 'FAIL'}", flush=True)
