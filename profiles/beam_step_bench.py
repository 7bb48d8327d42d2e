"""Beam search's cost per decoder step: Bench("decode_step_ts_scored") against Bench("decode_step_beam") (beam size 5) at 5, 20 and
60 slots (Whisper-small dims, synthetic weights, decode offset 224), medians over rounds. Every round of every side is a fresh
process; the sides alternate. With AXW_PARENT_LIB set to a libax_whisper.so built from the PARENT commit, the parent's
decode_step_ts_scored is measured the same way, alternating with this tree's rounds.

The beam step is the captured step up to the logits dump plus the candidates, selection, reorder and advance launches; from the
start state of a decode (one live hypothesis per clip) its first iterations fan the hypotheses out; how many slots the reorder
launch copied per iteration, and whether clips completed, is read back from an untimed repeat of the pass and printed.

    python profiles/beam_step_bench.py [slots ...] > profiles/beam_step_bench.txt"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(R, "whisper.axera_amd", "lib", "libax_whisper.so")
ITERS = 50
BEAM = 5
# side -> (Bench target, arg: the decode offset of the scored step, the beam size of the beam step)
SIDES = {"scored": ("decode_step_ts_scored", 224), "beam": ("decode_step_beam", BEAM)}


def measure(lib_path, batches, name, arg):
    """{slots: ms per step} of one Bench target from the library at lib_path (this process loads exactly one library)"""
    sys.path.insert(0, R)
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen
    import whisper_axera_amd as wa

    wa.LIB_PATH = lib_path
    have = C.CDLL(lib_path)
    wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}  # (the parent's library lacks the beam symbols)
    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=max(batches))
    out = {}
    for B in batches:
        e.bench(name, B, arg, ITERS)  # (the first call captures the graph)
        out[B] = [e.bench(name, B, arg, ITERS) / ITERS]
        if name == "decode_step_beam":  # what the timed iterations did: slots copied per iteration, clips complete at the end
            out[B] += [e.get_config_int("beam_bench_moved_slots") / max(e.get_config_int("beam_bench_iters"), 1), e.get_config_int("beam_bench_complete_clips")]
    e.close()
    return out


def child(lib, batches, name, arg):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, ",".join(map(str, batches)), name, str(arg)],
                       capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise SystemExit("round failed (%s, %s):\n" % (lib, name) + p.stdout[-2000:] + p.stderr[-2000:])
    return {int(k): v for k, v in json.loads(line[0][7:]).items()}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(measure(sys.argv[2], [int(x) for x in sys.argv[3].split(",")], sys.argv[4], int(sys.argv[5]))))
        sys.exit(0)
    batches = [int(x) for x in (sys.argv[1:] or ["5", "20", "60"])]
    parent = os.environ.get("AXW_PARENT_LIB")
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    moved = {}
    got = {s: {B: [] for B in batches} for s in list(SIDES) + (["parent_scored"] if parent else [])}
    for r in range(rounds):
        if parent:
            for B, v in child(parent, batches, "decode_step_ts_scored", 224).items():
                got["parent_scored"][B].append(v[0])
        for s, (name, arg) in SIDES.items():
            for B, v in child(TREE_LIB, batches, name, arg).items():
                got[s][B].append(v[0])
                if len(v) > 1:
                    moved[B] = v[1:]
    med = lambda v: float(np.median(v))
    for B in batches:
        a, b = med(got["scored"][B]), med(got["beam"][B])
        print(f"slots {B:3d} this tree: scored {a:.4f} ms, beam (K = {BEAM}) {b:.4f} ms ({b / a:.4f} x scored; {moved[B][0]:.2f} of {B} slots copied "
              f"per iteration, {moved[B][1]} clips complete at the end)"
              f"  (rounds: {[['%.4f' % x for x in got[s][B]] for s in ('scored', 'beam')]})", flush=True)
        if parent:
            pa = med(got["parent_scored"][B])
            print(f"slots {B:3d} parent:    scored {pa:.4f} ms; tree / parent {a / pa:.4f}  (rounds: {['%.4f' % x for x in got['parent_scored'][B]]})", flush=True)
