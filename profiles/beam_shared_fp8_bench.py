"""Beam search with both opt-in modes on one handle (DESIGN.md "Shared cross K/V over FP8 codes"): Bench("decode_step_beam") and
Bench("decode_attn_beam"), beam size 5, at 5, 20, 60 and 120 slots (Whisper-small dims, synthetic weights, from decode offset 224), the
protocol of profiles/beam_shared_cross_bench.py. Contenders in fresh processes, alternating round by round: the PARENT commit's
build (AXW_BENCH_PARENT_LIB=<its libax_whisper.so>; left out when unset) opened with both modes, where such a handle still runs h16
copies as its FP8-only handle does ("parent"), and opened shared-only ("parent_sh"); this tree's FP8-only handle, this tree's
shared-only handle, this tree's handle with both. Medians of ROUNDS rounds, every round printed.

Criteria, set before the run: the FP8-only and the shared-only medians lie inside the round-to-round spread of the parent's handle that
runs the same launches (nothing they run changed); the both-mode step is a win at a size if its median lies below the shared-only handle's fastest round there.

    python profiles/beam_shared_fp8_bench.py [slots ...] > profiles/beam_shared_fp8_bench.txt"""
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, BEAM = 50, 5
ROUNDS = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
MDIR = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
MODES = {"parent": dict(cross_kv="fp8", beam_cross="shared"), "parent_sh": dict(beam_cross="shared"), "fp8": dict(cross_kv="fp8"), "shared": dict(beam_cross="shared"),
         "both": dict(cross_kv="fp8", beam_cross="shared")}
COUNTERS = ("beam_cross_shared_launches", "cross_kv_fp8_launches")
MOVES = {"parent": (False, False), "parent_sh": (True, False), "fp8": (False, False), "shared": (True, False), "both": (True, True)}  # which counter a beam step moves


def child(mode, batches):
    """{target: {slots: ms per step}} of one handle (this process loads exactly one library)"""
    sys.path.insert(0, R)
    import ctypes as C
    import whisper_axera_amd as wa

    if mode.startswith("parent"):
        wa.LIB_PATH = os.environ["AXW_BENCH_PARENT_LIB"]
        have = C.CDLL(wa.LIB_PATH)
        wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}
    e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=max(batches), **MODES[mode])
    out = {"decode_step_beam": {}, "decode_attn_beam": {}}
    for what in out:
        for B in batches:
            n0 = [e.get_config_int(c) for c in COUNTERS]
            e.bench(what, B, BEAM, ITERS)  # (the first call captures the graph)
            out[what][B] = e.bench(what, B, BEAM, ITERS) / ITERS
            assert tuple(e.get_config_int(c) > n for c, n in zip(COUNTERS, n0)) == MOVES[mode], (mode, what, B)
    e.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen

    batches = [int(x) for x in (sys.argv[1:] or ["5", "20", "60", "120"])]
    if not os.path.exists(os.path.join(MDIR, "small", "small.safetensors")):
        modelgen.write_model_dir(MDIR, "small", seed=0)
    modes = (("parent", "parent_sh") if os.environ.get("AXW_BENCH_PARENT_LIB") else ()) + ("fp8", "shared", "both")
    got = {m: {} for m in modes}
    for _ in range(ROUNDS):
        for mode in modes:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, ",".join(map(str, batches))], capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"round failed ({mode}):\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
            for what, per in json.loads(line[0][7:]).items():
                for B, v in per.items():
                    got[mode].setdefault((what, int(B)), []).append(v)
    print(f"# Whisper-small dims, beam size {BEAM}, from decode offset 224, {ITERS} steps per figure, {ROUNDS} fresh processes per contender alternating "
          f"({' / '.join(modes)}); ms per step: median (rounds)")
    fmt = lambda v: f"{np.median(v):.4f} ({' '.join('%.4f' % x for x in v)})"
    for what in ("decode_step_beam", "decode_attn_beam"):
        for B in batches:
            print(f"{what} {B:3d} slots:")
            for m in modes:
                print(f"    {m:10s}{fmt(got[m][what, B])}")
            f8, sh, bo = (got[m][what, B] for m in ("fp8", "shared", "both"))
            line = f"    both / shared {np.median(bo) / np.median(sh):.3f}, both / fp8-only {np.median(bo) / np.median(f8):.3f}; both median " \
                   f"{'below' if np.median(bo) < min(sh) else 'NOT below'} the shared-only handle's fastest round {min(sh):.4f}"
            if "parent" in got:
                for name, v, pa in (("fp8-only", f8, got["parent"][what, B]), ("shared-only", sh, got["parent_sh"][what, B])):
                    line += f"\n    {name} / its parent {np.median(v) / np.median(pa):.4f}, that parent's spread {min(pa) / np.median(pa):.4f} .. {max(pa) / np.median(pa):.4f}"
            print(line, flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], [int(x) for x in sys.argv[3].split(",")])
    else:
        main()
