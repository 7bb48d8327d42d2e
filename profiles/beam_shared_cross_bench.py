"""Beam search over one cross K/V copy per clip (DESIGN.md "Shared cross K/V") against the copy path: Bench("decode_step_beam"), beam
size 5, at 5, 20 and 60 slots (Whisper-small dims, synthetic weights, from decode offset 224), the method of
profiles/beam_step_bench.py. Three libraries / handles in fresh processes, alternating round by round: the PARENT commit's build
(AXW_BENCH_PARENT_LIB=<its libax_whisper.so>; left out when unset), this tree's default handle, this tree's shared handle. Medians of
ROUNDS rounds, every round printed. Beside it Bench("decode_attn_beam"): the attention launches alone (self and cross) of the same
step, default against shared (the parent has no such target).

The cross-attention launches alone come from a kernel-stats run of their own (self-attention is decode_attention_kernel<0>, the copy
path's cross-attention <1> fused or <2> folded, the shared path's decode_cross_attention_group_kernel), one handle per run:

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/beam_shared_cross_bench.py --stats copy|shared 60

The criterion for calling the mode a win at a size: the shared median lies below the default handle's fastest round.

    python profiles/beam_shared_cross_bench.py [slots ...] > profiles/beam_shared_cross_bench.txt"""
import json
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, BEAM = 50, 5
ROUNDS = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
MDIR = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")


def child(mode, batches):
    """{target: {slots: ms per step}} of one handle (this process loads exactly one library)"""
    sys.path.insert(0, R)
    import ctypes as C
    import whisper_axera_amd as wa

    if mode == "parent":  # it knows neither the switch nor what came with it
        wa.LIB_PATH = os.environ["AXW_BENCH_PARENT_LIB"]
        have = C.CDLL(wa.LIB_PATH)
        wa.SYMBOLS = {k: v for k, v in wa.SYMBOLS.items() if hasattr(have, k)}
        e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=max(batches))
    else:
        e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=max(batches), beam_cross=mode)
        assert e.get_config_int("beam_cross_shared") == (1 if mode == "shared" else 0)
    out = {"decode_step_beam": {}, "decode_attn_beam": {}}
    for what in out if mode != "parent" else ("decode_step_beam",):
        for B in batches:
            n0 = 0 if mode == "parent" else e.get_config_int("beam_cross_shared_launches")
            e.bench(what, B, BEAM, ITERS)  # (the first call captures the graph)
            out[what][B] = e.bench(what, B, BEAM, ITERS) / ITERS
            if mode != "parent":
                assert (e.get_config_int("beam_cross_shared_launches") > n0) == (mode == "shared"), (mode, what, B)
    e.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
    import modelgen

    batches = [int(x) for x in (sys.argv[1:] or ["5", "20", "60"])]
    if not os.path.exists(os.path.join(MDIR, "small", "small.safetensors")):
        modelgen.write_model_dir(MDIR, "small", seed=0)
    modes = (("parent",) if os.environ.get("AXW_BENCH_PARENT_LIB") else ()) + ("copy", "shared")
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
    print(f"# Whisper-small dims, beam size {BEAM}, from decode offset 224, {ITERS} steps per figure, {ROUNDS} fresh processes per mode alternating "
          f"({' / '.join(modes)}); ms per step: median (rounds)")
    fmt = lambda v: f"{np.median(v):.4f} ({' '.join('%.4f' % x for x in v)})"
    for what in ("decode_step_beam", "decode_attn_beam"):
        for B in batches:
            c, s = got["copy"][what, B], got["shared"][what, B]
            line = f"{what} {B:3d} slots: default {fmt(c)}  shared {fmt(s)}  shared / default {np.median(s) / np.median(c):.3f}"
            if what == "decode_step_beam":
                line += f"  shared median {'below' if np.median(s) < min(c) else 'NOT below'} the default's fastest round {min(c):.4f}"
                if "parent" in got:
                    pa = got["parent"][what, B]
                    line += f"\n{'':27s}parent {fmt(pa)}  default / parent {np.median(c) / np.median(pa):.4f}, parent's spread {min(pa) / np.median(pa):.4f} .. {max(pa) / np.median(pa):.4f}"
            print(line, flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--stats":  # ITERS attention-only steps (after as many warm ones) of one handle, for the profiler
        sys.path.insert(0, R)
        import whisper_axera_amd as wa
        e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=int(sys.argv[3]), beam_cross=sys.argv[2])
        e.bench("decode_attn_beam", int(sys.argv[3]), BEAM, ITERS)
        e.close()
    elif len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], [int(x) for x in sys.argv[3].split(",")])
    else:
        main()
