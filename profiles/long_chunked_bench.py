"""Chunked long-form cost (Whisper-small dims, synthetic weights, one MI355X, max_batch 64), A/B/C alternating, medians. Writes
profiles/long_chunked_bench.txt.

One file of 3600 s (the demo clip tiled), per-window budgets 48 and 224:
  (a) run_long_windows on the one file: the seek loop, one window per pass;
  (b) run_long_chunked_windows on it: the windows chosen first, 64 per pass;
  (c) run_long_windows on 64 such files cut to 150 s, side by side: 64-wide passes through the same encoder and step graph.
Acceptance: (b) in windows/s is no more than 10 % below (c) at the same budget. (b) / (a) is reported, not gated.
Also Bench("long_cut_plan") for the hour file: levels + plan kernels on the resident store, next to one decode pass of (b).

(The committed file also holds, appended by hand, the headline of bench.py for the parent commit and this tree, alternating.)

AXW_CHUNK_BENCH_SECONDS / AXW_CHUNK_BENCH_ROUNDS / AXW_CHUNK_BENCH_BUDGETS shrink the run for a first look."""
import os
import sys
import time
import wave

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
import modelgen  # noqa: E402
import whisper_axera_amd as wa  # noqa: E402

mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
    modelgen.write_model_dir(mdir, "small", seed=0)
SECONDS = int(os.environ.get("AXW_CHUNK_BENCH_SECONDS", "3600"))
ROUNDS = int(os.environ.get("AXW_CHUNK_BENCH_ROUNDS", "3"))
BUDGETS = [int(x) for x in os.environ.get("AXW_CHUNK_BENCH_BUDGETS", "48,224").split(",")]
SLOTS, SIDE = 64, 150

w = wave.open(os.path.join(R, "tests", "golden", "demo.wav"))
demo = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).astype(np.float32) / np.float32(32768.0)
hour = np.ascontiguousarray(np.tile(demo, SECONDS * 16000 // len(demo) + 1)[: SECONDS * 16000])
side = [np.ascontiguousarray(np.roll(hour, -7919 * k)[: SIDE * 16000]) for k in range(SLOTS)]
e = wa.Whisper("small", mdir, "zh", device=0, max_batch=SLOTS)
OUT = os.path.join(R, "profiles", "long_chunked_bench.txt")
open(OUT, "w").close()


def say(line):  # (line by line: a run that is cut short leaves what it measured)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


say(f"# one file of {SECONDS} s, {SLOTS} slots, {ROUNDS} rounds alternating a / b / c, medians; windows/s")
for budget in BUDGETS:
    runs = {"a": lambda: e.run_long_windows([hour], max_new=budget), "b": lambda: e.run_long_chunked_windows([hour], max_new=budget),
            "c": lambda: e.run_long_windows(side, max_new=budget)}
    n = {k: sum(len(log) for log in f()) for k, f in runs.items()}  # warm: graphs captured, arenas allocated
    t = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, f in runs.items():
            t[k].append(timed(f)[0])
    med = {k: float(np.median(v)) for k, v in t.items()}
    rate = {k: n[k] / med[k] for k in runs}
    say(f"budget {budget:3d}: (a) seek loop, one file: {n['a']} windows, {rate['a']:.1f} windows/s ({med['a']:.2f} s) | (b) chunked, one file: {n['b']} windows, "
        f"{rate['b']:.1f} windows/s ({med['b']:.2f} s) | (c) seek loop, {SLOTS} files of {SIDE} s: {n['c']} windows, {rate['c']:.1f} windows/s ({med['c']:.2f} s)")
    say(f"budget {budget:3d}: b / c = {rate['b'] / rate['c']:.4f} (acceptance: >= 0.90: {'met' if rate['b'] >= 0.9 * rate['c'] else 'MISSED'}) | b / a = "
        f"{rate['b'] / rate['a']:.2f}  (seconds a {['%.2f' % x for x in t['a']]} b {['%.2f' % x for x in t['b']]} c {['%.2f' % x for x in t['c']]})")
iters = 20
ms = [e.bench("long_cut_plan", 1, SECONDS, iters) / iters for _ in range(ROUNDS)]
enc = [e.bench("encoder", SLOTS, 0, 5) / 5 for _ in range(ROUNDS)]
say(f"long_cut_plan, one file of {SECONDS} s: {float(np.median(ms)):.4f} ms ({['%.4f' % x for x in ms]}); the encoder alone of one {SLOTS}-window pass: "
    f"{float(np.median(enc)):.2f} ms")
hbm = len(hour) // 160 * e.n_mels * 4 / 6.3e9  # ms to read the store once at 6.3 TB/s
say(f"(the store of that file is {len(hour) // 160 * e.n_mels * 4 / 1e6:.1f} MB: {hbm:.4f} ms at 6.3 TB/s; the levels kernel reads it 1.2 times)")
e.close()
