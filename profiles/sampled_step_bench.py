"""Sampled mode's cost per decoder step: Bench("decode_step_ts_scored") against Bench("decode_step_ts_sampled") with every clip at
temperature 0 and at temperature 1, at 1, 4 and 64 clips (Whisper-small dims, synthetic weights, decode offset 224), medians over
rounds. Every round of every side is a fresh process; the sides alternate. With AXW_PARENT_LIB set to a libax_whisper.so built
from the PARENT commit, the parent's decode_step_ts_scored is measured the same way, alternating with this tree's rounds.

    python profiles/sampled_step_bench.py [batches ...] > profiles/sampled_step_bench.txt"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(R, "whisper.axera_amd", "lib", "libax_whisper.so")
ITERS = 50
# side -> (Bench target, AX_WHISPER_BENCH_TEMPERATURE)
SIDES = {"scored": ("decode_step_ts_scored", None), "sampled_t0": ("decode_step_ts_sampled", "0"), "sampled_t1": ("decode_step_ts_sampled", "1")}


def measure(lib_path, batches, name):
    """{batch: ms per step} of one Bench target from the library at lib_path (this process loads exactly one library)"""
    sys.path.insert(0, R)
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen
    import whisper_axera_amd as wa

    wa.LIB_PATH = lib_path
    have = C.CDLL(lib_path)
    wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}  # (the parent's library lacks the sampled symbols)
    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=max(batches))
    out = {}
    for B in batches:
        e.bench(name, B, 224, ITERS)  # (the first call captures the graph)
        out[B] = e.bench(name, B, 224, ITERS) / ITERS
    e.close()
    return out


def child(lib, batches, name, temperature):
    env = dict(os.environ)
    if temperature is not None:
        env["AX_WHISPER_BENCH_TEMPERATURE"] = temperature
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, ",".join(map(str, batches)), name], capture_output=True,
                       text=True, timeout=600, env=env)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise SystemExit("round failed (%s, %s):\n" % (lib, name) + p.stdout[-2000:] + p.stderr[-2000:])
    return {int(k): v for k, v in json.loads(line[0][7:]).items()}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(measure(sys.argv[2], [int(x) for x in sys.argv[3].split(",")], sys.argv[4])))
        sys.exit(0)
    batches = [int(x) for x in (sys.argv[1:] or ["1", "4", "64"])]
    parent = os.environ.get("AXW_PARENT_LIB")
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    got = {s: {B: [] for B in batches} for s in list(SIDES) + (["parent_scored"] if parent else [])}
    for r in range(rounds):
        if parent:
            for B, v in child(parent, batches, "decode_step_ts_scored", None).items():
                got["parent_scored"][B].append(v)
        for s, (name, temp) in SIDES.items():
            for B, v in child(TREE_LIB, batches, name, temp).items():
                got[s][B].append(v)
    med = lambda v: float(np.median(v))
    for B in batches:
        a, b, c = (med(got[s][B]) for s in ("scored", "sampled_t0", "sampled_t1"))
        print(f"B {B:3d} this tree: scored {a:.4f} ms, sampled t=0 {b:.4f} ms ({b / a:.4f} x scored), sampled t=1 {c:.4f} ms ({c / a:.4f} x scored)"
              f"  (rounds: {[['%.4f' % x for x in got[s][B]] for s in ('scored', 'sampled_t0', 'sampled_t1')]})", flush=True)
        if parent:
            pa = med(got["parent_scored"][B])
            print(f"B {B:3d} parent:    scored {pa:.4f} ms; tree / parent {a / pa:.4f}  (rounds: {['%.4f' % x for x in got['parent_scored'][B]]})", flush=True)
