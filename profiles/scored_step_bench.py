"""Scored mode's cost per decoder step: Bench("decode_step"), Bench("decode_step_ts") and Bench("decode_step_ts_scored") at 1, 4
and 64 clips (Whisper-small dims, synthetic weights, decode offset 224), run alternately A/B/C/A/B/C, medians. With
AXW_PARENT_LIB set to a libax_whisper.so built from the PARENT commit, a child process per round
measures the parent's decode_step and decode_step_ts the same way, alternating with this tree's rounds."""
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["decode_step", "decode_step_ts", "decode_step_ts_scored"]
ITERS = 50


def measure(lib_path, batches, names, rounds):
    """{name: {batch: [ms per step, one per round]}} from the library at lib_path (this process loads exactly one library)"""
    sys.path.insert(0, R)
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen
    import whisper_axera_amd as wa

    wa.LIB_PATH = lib_path
    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=max(batches))
    out = {n: {B: [] for B in batches} for n in names}
    for B in batches:
        for _ in range(rounds):
            for n in names:
                out[n][B].append(e.bench(n, B, 224, ITERS) / ITERS)
    e.close()
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":  # one round of the parent's two names, as JSON
        lib, batches = sys.argv[2], [int(x) for x in sys.argv[3].split(",")]
        # the parent's library has no scored symbols: bind what it has
        sys.path.insert(0, R)
        import whisper_axera_amd as wa

        import ctypes as C
        have = C.CDLL(lib)
        wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}
        print("RESULT " + json.dumps(measure(lib, batches, NAMES[:2], 1)))
        sys.exit(0)
    batches = [int(x) for x in (sys.argv[1:] or ["1", "4", "64"])]
    parent = os.environ.get("AXW_PARENT_LIB")
    rounds = 4
    mine = {n: {B: [] for B in batches} for n in NAMES}
    theirs = {n: {B: [] for B in batches} for n in NAMES[:2]}
    for r in range(rounds):  # a fresh process per round and side: parent, this tree, parent, ...
        for side, lib in (("parent", parent), ("tree", os.path.join(R, "whisper.axera_amd", "lib", "libax_whisper.so"))):
            if not lib:
                continue
            if side == "parent":
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, ",".join(map(str, batches))], capture_output=True, text=True, timeout=600)
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    raise SystemExit("parent round failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
                got = json.loads(line[0][7:])
                for n in theirs:
                    for B in batches:
                        theirs[n][B] += got[n][str(B)]
            else:
                p = subprocess.run([sys.executable, "-c", "import sys, json; sys.path.insert(0, %r); import scored_step_bench as s; print('RESULT ' + json.dumps(s.measure(%r, %r, s.NAMES, 1)))"
                                    % (os.path.dirname(os.path.abspath(__file__)), lib, batches)], capture_output=True, text=True, timeout=600)
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    raise SystemExit("round failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
                got = json.loads(line[0][7:])
                for n in mine:
                    for B in batches:
                        mine[n][B] += got[n][str(B)]
    med = lambda v: float(np.median(v))
    for B in batches:
        a, b, c = (med(mine[n][B]) for n in NAMES)
        print(f"B {B:3d} this tree: decode_step {a:.4f} ms, decode_step_ts {b:.4f} ms, decode_step_ts_scored {c:.4f} ms; scored / ts {c / b:.4f}, ts / plain {b / a:.4f}"
              f"  (rounds: {[['%.4f' % x for x in mine[n][B]] for n in NAMES]})", flush=True)
        if parent:
            pa, pb = med(theirs["decode_step"][B]), med(theirs["decode_step_ts"][B])
            print(f"B {B:3d} parent:    decode_step {pa:.4f} ms, decode_step_ts {pb:.4f} ms; tree / parent {a / pa:.4f} (plain) {b / pb:.4f} (ts)"
                  f"  (rounds: {[['%.4f' % x for x in theirs[n][B]] for n in NAMES[:2]]})", flush=True)
