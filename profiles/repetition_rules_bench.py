"""The repetition rules' cost per decoder step (DESIGN.md "Repetition rules"): Bench("decode_step_ts_scored") at 5 and 64 slots,
Whisper-small dims, synthetic weights, decode offset 224; medians over rounds and the spread (max - min) of each side. Every round of
every side is a fresh process and the sides alternate within a round, as in profiles/suppress_tokens_bench.py.

Sides: "off", this tree with no rules set; "rules", this tree with (1.1, 3) and the 82 non-speech ids installed
(tests/golden/non_speech_multilingual.json); with AXW_PARENT_LIB set to a libax_whisper.so built from the PARENT commit, "parent".

    python profiles/repetition_rules_bench.py > profiles/repetition_rules_bench.txt"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(R, "whisper.axera_amd", "lib", "libax_whisper.so")
ITERS = 50
OFFSET = 224
SLOTS = (5, 64)


def measure(lib_path, rules):
    """{slots: ms per step} from the library at lib_path (this process loads exactly one library)"""
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
    if rules:
        e.set_suppress_tokens(json.load(open(os.path.join(R, "tests", "golden", "non_speech_multilingual.json"))))
        e.set_repetition_rules(1.1, 3)
        assert e.get_config_int("repetition_rules") == 1
    out = {}
    for B in SLOTS:
        e.bench("decode_step_ts_scored", B, OFFSET, ITERS)  # (the first call captures the graph)
        out[B] = e.bench("decode_step_ts_scored", B, OFFSET, ITERS) / ITERS
    e.close()
    return out


def child(lib, rules):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, str(int(rules))], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise SystemExit("round failed (%s, rules %d):\n" % (lib, rules) + p.stdout[-2000:] + p.stderr[-2000:])
    return {int(k): v for k, v in json.loads(line[0][7:]).items()}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(measure(sys.argv[2], sys.argv[3] == "1")))
        sys.exit(0)
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "3"))
    sides = {"off": (TREE_LIB, False), "rules": (TREE_LIB, True)}
    if os.environ.get("AXW_PARENT_LIB"):
        sides = {"parent": (os.environ["AXW_PARENT_LIB"], False), **sides}
    got = {s: {B: [] for B in SLOTS} for s in sides}
    for r in range(rounds):
        for s, (lib, rules) in sides.items():
            for B, v in child(lib, rules).items():
                got[s][B].append(v)
        print("# round %d done" % r, file=sys.stderr, flush=True)
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    for B in SLOTS:
        line = "scored slots %2d:" % B
        for s in sides:
            line += "  %s %.4f ms (spread %.4f)" % (s, med(got[s][B]), spread(got[s][B]))
        off = med(got["off"][B])
        if "parent" in sides:
            p = got["parent"][B]
            line += "  | off - parent %+.4f ms (%s the parent's spread)" % (off - med(p), "within" if abs(off - med(p)) <= spread(p) else "OUTSIDE")
        line += "  | rules - off %+.4f ms per step, rules / off %.4f" % (med(got["rules"][B]) - off, med(got["rules"][B]) / off)
        print(line, flush=True)
        print("          rounds: " + "; ".join("%s %s" % (s, ["%.4f" % x for x in got[s][B]]) for s in sides), flush=True)
