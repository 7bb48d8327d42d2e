"""Cross-attention over each slot's own audio span (DESIGN.md "Cross-attention spans") against the default handle: Whisper-small
dims, synthetic weights, one MI355X, Bench("decode_step") at t = 224 (ms per step, ITERS replays of the captured step between two
events). One process per handle, the modes alternating (ROUNDS processes each); every figure is the median over the rounds with
[min .. max]. With AXW_BENCH_PARENT_LIB=<a libax_whisper.so built from the commit before the mode> that library's default handle is a
mode of its own ("parent"): the default handle of this tree ("h16", "fp8") has to sit within the parent's round-to-round spread.

  parent / h16 / fp8      default handles: all 1500 frames, today's kernels
  span-h16 / span-fp8     cross_span="audio" handles, every slot at AX_WHISPER_BENCH_CROSS_SPAN = 1500, 750, 300 keys, and one mixed
                          run (64 slots, spans uniform in 150 .. 1500)
  span-h16-1piece         the same kernel with one piece per (slot, head) (AX_WHISPER_CROSS_SPAN_PIECES=1), the mixed run only: what
                          balancing by blocks buys over a launch paced by its longest clip

    python profiles/cross_span_bench.py > profiles/cross_span_bench.txt
"""
import os
import subprocess
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))

MDIR = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
ROUNDS = int(os.environ.get("AXW_BENCH_ROUNDS", "3"))
ITERS, T = 200, 224
SLOTS = (4, 16, 64, 128, 256)
SPANS = (1500, 750, 300)


def child(mode):
    import whisper_axera_amd as wa

    span = mode.startswith("span-")
    if mode == "parent":  # the library of the commit before the mode: it has neither the two new symbols nor the variable
        wa.LIB_PATH = os.environ["AXW_BENCH_PARENT_LIB"]
        for name in ("AX_WHISPER_CrossSpanAttention", "AX_WHISPER_GetCrossSpans"):
            wa.SYMBOLS.pop(name)
        e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=256)
    else:
        if mode.endswith("-1piece"):
            os.environ["AX_WHISPER_CROSS_SPAN_PIECES"] = "1"
        e = wa.Whisper("small", MDIR, "zh", device=0, max_batch=256, cross_kv="fp8" if "fp8" in mode else "h16", cross_span="audio" if span else "full")
        assert e.get_config_int("cross_span") == (1 if span else 0)
    out = {}
    e.bench("encoder", 16, 0, 1)  # the cross K/V of 16 slots; the kernels' time does not depend on the values

    def step(b, key):
        n0 = 0 if mode == "parent" else e.get_config_int("cross_span_launches")
        e.bench("decode_step", b, T, 20)  # warm: capture, first replays
        out[key] = e.bench("decode_step", b, T, ITERS) / ITERS
        assert mode == "parent" or (e.get_config_int("cross_span_launches") > n0) == span

    if not mode.endswith("-1piece"):
        for b in SLOTS:
            for s in SPANS if span else (1500,):
                os.environ["AX_WHISPER_BENCH_CROSS_SPAN"] = str(s)
                step(b, f"{b} slots, span {s}")
    if span:
        os.environ["AX_WHISPER_BENCH_CROSS_SPAN"] = "mixed"
        step(64, "64 slots, spans 150..1500")
    e.close()
    for k, v in out.items():
        print(f"RESULT\t{k}\t{v:.6f}", flush=True)


def main():
    import modelgen

    if not os.path.exists(os.path.join(MDIR, "small", "small.safetensors")):
        modelgen.write_model_dir(MDIR, "small", seed=0)
    modes = (("parent",) if os.environ.get("AXW_BENCH_PARENT_LIB") else ()) + ("h16", "span-h16", "fp8", "span-fp8", "span-h16-1piece")
    res = {m: {} for m in modes}
    for _ in range(ROUNDS):
        for mode in modes:  # a fresh process per handle, the modes alternating
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", mode], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"child {mode} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT\t"):
                    _, k, v = ln.split("\t")
                    res[mode].setdefault(k, []).append(float(v))
    fmt = lambda a: f"{np.median(a):8.4f} [{min(a):.4f} .. {max(a):.4f}]"
    print(f"# small dims, decode_step at t = {T}, {ITERS} replays per figure, {ROUNDS} processes per mode alternating ({' / '.join(modes)}): "
          f"ms per step, median [min .. max]", flush=True)
    print("# default handles (all 1500 frames)")
    for b in SLOTS:
        k = f"{b} slots, span 1500"
        line = f"{b:4d} slots"
        for m in ("parent", "h16", "fp8"):
            if m in res and k in res[m]:
                line += f"   {m} {fmt(res[m][k])}"
        if "parent" in res and k in res["parent"]:
            line += f"   h16 / parent {np.median(res['h16'][k]) / np.median(res['parent'][k]):.3f}"
        print(line, flush=True)
    for kv in ("h16", "fp8"):
        print(f"# span handle over the {kv} images against the default {kv} handle of this tree (ratio below 1: the span handle is faster)")
        for b in SLOTS:
            base = np.median(res[kv][f"{b} slots, span 1500"])
            line = f"{b:4d} slots"
            for s in SPANS:
                a = res["span-" + kv][f"{b} slots, span {s}"]
                line += f"   span {s}: {fmt(a)} x{np.median(a) / base:.3f}"
            print(line, flush=True)
        a = res["span-" + kv]["64 slots, spans 150..1500"]
        print(f"  64 slots, spans uniform in 150 .. 1500: {fmt(a)} x{np.median(a) / np.median(res[kv]['64 slots, span 1500']):.3f}", flush=True)
    a, b = res["span-h16"]["64 slots, spans 150..1500"], res["span-h16-1piece"]["64 slots, spans 150..1500"]
    print(f"# 64 slots, spans uniform in 150 .. 1500, h16: balanced pieces {fmt(a)}   one piece per (slot, head) {fmt(b)}   balanced / one piece {np.median(a) / np.median(b):.3f}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        main()
