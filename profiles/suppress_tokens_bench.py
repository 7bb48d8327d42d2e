"""Token suppression's cost per decoder step (DESIGN.md "Token suppression"): Bench("decode_step_ts_scored"), "decode_step_ts_sampled",
"decode_step_beam" (beam size 5) and "stream_step_ts" at 5, 20 and 64 slots (the beam step at 60: a multiple of its beam size),
Whisper-small dims, synthetic weights, decode offset 224; medians over rounds and the spread (max - min) of each side. Every round
of every side is a fresh process and the sides alternate within a round.

Sides: "empty", this tree with no set installed; "set", this tree with the 82 non-speech ids installed
(tests/golden/non_speech_multilingual.json); with AXW_PARENT_LIB set to a libax_whisper.so built from the PARENT commit, "parent";
with AXW_ALT_LIB set to another build of this tree (the other way of reading the mask: its words read from global memory in the
row loop of every kernel, or staged in LDS in every kernel), "alt_set", the same set through that library.

    python profiles/suppress_tokens_bench.py > profiles/suppress_tokens_bench.txt"""
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
# leg -> (Bench target, arg: the decode offset of a step leg, the beam size of the beam leg, slots)
LEGS = {"scored": ("decode_step_ts_scored", 224, (5, 20, 64)), "sampled": ("decode_step_ts_sampled", 224, (5, 20, 64)),
        "beam": ("decode_step_beam", BEAM, (5, 20, 60)), "stream": ("stream_step_ts", 224, (5, 20, 64))}


def measure(lib_path, install):
    """{leg: {slots: ms per step}} from the library at lib_path (this process loads exactly one library)"""
    sys.path.insert(0, R)
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen
    import whisper_axera_amd as wa

    wa.LIB_PATH = lib_path
    have = C.CDLL(lib_path)
    wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}  # (the parent's library lacks the new symbols)
    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=64)
    if install:
        e.set_suppress_tokens(json.load(open(os.path.join(R, "tests", "golden", "non_speech_multilingual.json"))))
        assert e.get_config_int("n_suppress_tokens") == 82
    out = {}
    for leg, (name, arg, batches) in LEGS.items():
        out[leg] = {}
        for B in batches:
            e.bench(name, B, arg, ITERS)  # (the first call captures the graph)
            out[leg][B] = e.bench(name, B, arg, ITERS) / ITERS
    e.close()
    return out


def child(lib, install):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, str(int(install))], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise SystemExit("round failed (%s, set %d):\n" % (lib, install) + p.stdout[-2000:] + p.stderr[-2000:])
    return {leg: {int(k): v for k, v in d.items()} for leg, d in json.loads(line[0][7:]).items()}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(measure(sys.argv[2], sys.argv[3] == "1")))
        sys.exit(0)
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    sides = {"empty": (TREE_LIB, False), "set": (TREE_LIB, True)}
    if os.environ.get("AXW_PARENT_LIB"):
        sides = {"parent": (os.environ["AXW_PARENT_LIB"], False), **sides}
    if os.environ.get("AXW_ALT_LIB"):
        sides["alt_set"] = (os.environ["AXW_ALT_LIB"], True)
    got = {s: {leg: {B: [] for B in LEGS[leg][2]} for leg in LEGS} for s in sides}
    for r in range(rounds):
        for s, (lib, install) in sides.items():
            for leg, d in child(lib, install).items():
                for B, v in d.items():
                    got[s][leg][B].append(v)
        print("# round %d done" % r, file=sys.stderr, flush=True)
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    for leg in LEGS:
        for B in LEGS[leg][2]:
            line = "%-7s slots %2d:" % (leg, B)
            for s in sides:
                v = got[s][leg][B]
                line += "  %s %.4f ms (spread %.4f)" % (s, med(v), spread(v))
            e = med(got["empty"][leg][B])
            if "parent" in sides:
                p = got["parent"][leg][B]
                line += "  | empty - parent %+.4f ms (%s the parent's spread)" % (e - med(p), "within" if abs(e - med(p)) <= spread(p) else "OUTSIDE")
            line += "  | set / empty %.4f" % (med(got["set"][leg][B]) / e)
            if "alt_set" in sides:
                line += ", alt_set / empty %.4f" % (med(got["alt_set"][leg][B]) / e)
            print(line, flush=True)
            print("          rounds: " + "; ".join("%s %s" % (s, ["%.4f" % x for x in got[s][leg][B]]) for s in sides), flush=True)
