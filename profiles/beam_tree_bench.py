"""Beam search over an ancestry table (DESIGN.md "Tree self-attention"): Bench("decode_step_beam") and Bench("decode_attn_beam"), beam
size 5, at 5, 20, 60 and 120 slots (Whisper-small dims, synthetic weights, from decode offset 224), the protocol of
profiles/beam_shared_fp8_bench.py. Contenders in fresh processes, alternating round by round: the PARENT commit's build
(AXW_BENCH_PARENT_LIB=<its libax_whisper.so>; left out when unset) opened with cross_kv="fp8" and beam_cross="shared" ("parent"); this
tree's handle with the same two modes ("both"); this tree's handle with beam_self="tree" as well ("tree"). Medians of ROUNDS rounds,
every round printed, and per size the fraction of the self K/V stream the tree handle's last counted step read
(beam_bench_self_blocks_needed / _total). The bench starts positions [0, 224) of every hypothesis on ONE slot of its clip (a decode
that far has long lost all but one ancestor of its early positions); AX_WHISPER_BENCH_TREE_PREFIX=identity starts them on K slots.

Criteria, set before the run: the "both" median lies inside the parent's round-to-round spread (nothing it runs changed); the tree
step is a win at a size if its median lies below the "both" handle's fastest round there.

    python profiles/beam_tree_bench.py [slots ...] > profiles/beam_tree_bench.txt"""
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, BEAM = 50, 5
ROUNDS = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
MDIR = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
BOTH = dict(cross_kv="fp8", beam_cross="shared")
MODES = {"parent": BOTH, "both": BOTH, "tree": dict(BOTH, beam_self="tree")}


def child(mode, batches):
    """{target: {slots: ms per step}} of one handle (this process loads exactly one library)"""
    sys.path.insert(0, R)
    import ctypes as C
    import whisper_axera_amd as wa

    if mode == "parent":
        wa.LIB_PATH = os.environ["AXW_BENCH_PARENT_LIB"]
        have = C.CDLL(wa.LIB_PATH)
        wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}
    e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=max(batches), **MODES[mode])
    out = {"decode_step_beam": {}, "decode_attn_beam": {}, "blocks": {}}
    for what in ("decode_step_beam", "decode_attn_beam"):
        for B in batches:
            n0 = e.get_config_int("beam_self_tree_launches") if mode != "parent" else 0
            e.bench(what, B, BEAM, ITERS)  # (the first call captures the graph)
            out[what][B] = e.bench(what, B, BEAM, ITERS) / ITERS
            if mode != "parent":
                assert (e.get_config_int("beam_self_tree_launches") > n0) == (mode == "tree"), (mode, what, B)
            if mode == "tree" and what == "decode_step_beam":
                out["blocks"][B] = [e.get_config_int("beam_bench_self_blocks_needed"), e.get_config_int("beam_bench_self_blocks_total"),
                                    e.get_config_int("beam_bench_moved_slots"), e.get_config_int("beam_bench_iters")]
    e.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen

    batches = [int(x) for x in (sys.argv[1:] or ["5", "20", "60", "120"])]
    if not os.path.exists(os.path.join(MDIR, "small", "small.safetensors")):
        modelgen.write_model_dir(MDIR, "small", seed=0)
    modes = (("parent",) if os.environ.get("AXW_BENCH_PARENT_LIB") else ()) + ("both", "tree")
    got, blocks = {m: {} for m in modes}, {}
    for _ in range(ROUNDS):
        for mode in modes:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, ",".join(map(str, batches))], capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"round failed ({mode}):\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
            res = json.loads(line[0][7:])
            blocks.update({int(B): v for B, v in res.pop("blocks").items()})
            for what, per in res.items():
                for B, v in per.items():
                    got[mode].setdefault((what, int(B)), []).append(v)
    print(f"# Whisper-small dims, beam size {BEAM}, from decode offset 224, {ITERS} steps per figure, {ROUNDS} fresh processes per contender alternating "
          f"({' / '.join(modes)}); ms per step: median (rounds); tree prefix: {os.environ.get('AX_WHISPER_BENCH_TREE_PREFIX', 'one slot per clip')}")
    fmt = lambda v: f"{np.median(v):.4f} ({' '.join('%.4f' % x for x in v)})"
    for what in ("decode_step_beam", "decode_attn_beam"):
        for B in batches:
            print(f"{what} {B:3d} slots:")
            for m in modes:
                print(f"    {m:8s}{fmt(got[m][what, B])}")
            bo, tr = got["both"][what, B], got["tree"][what, B]
            line = f"    tree / both {np.median(tr) / np.median(bo):.3f}; tree median {'below' if np.median(tr) < min(bo) else 'NOT below'} the both handle's fastest round {min(bo):.4f}"
            if "parent" in got:
                pa = got["parent"][what, B]
                line += f"\n    both / parent {np.median(bo) / np.median(pa):.4f}, the parent's spread {min(pa) / np.median(pa):.4f} .. {max(pa) / np.median(pa):.4f}"
            print(line, flush=True)
    for B in batches:
        need, total, moved, iters = blocks[B]
        print(f"self K/V stream {B:3d} slots: {need} of {total} (slot, block) loads per layer and head in the last counted step = {need / total:.3f}; "
              f"{moved} slots moved in {iters} steps = {moved / (iters * B):.3f} per slot and step")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], [int(x) for x in sys.argv[3].split(",")])
    else:
        main()
