"""Long-form cost (Whisper-small dims, synthetic weights, one MI355X), A/B alternating, medians:

1. 16 files of 150 s through run_long_windows against the SAME windows (the 30 s of audio at every logged seek) fed as clips
   through run_timestamp_tokens_batch in batches of 16 with the same per-window budget. Budget 2 forces a full advance per window
   (no pair of timestamps in two ids: 5 windows per file); budget 48 reports the window count actually taken.
   Expectation: long-form windows per second within 10 % of the batched clips per second — the allowance covers one ids D2H,
   the host rule and one seek H2D per pass, and the window kernel.
2. Bench("frontend_long") for one file of 30 s, 300 s and 3600 s next to Bench("frontend") for one clip: ms, and ms per 30 s."""
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
import modelgen  # noqa: E402
import whisper_axera_amd as wa  # noqa: E402

mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
    modelgen.write_model_dir(mdir, "small", seed=0)
N_FILES, SECONDS, ROUNDS = 16, 150, 3
e = wa.Whisper("small", mdir, "zh", device=0, max_batch=N_FILES)
rng = np.random.default_rng(0)
files = [(rng.standard_normal(16000 * SECONDS) * 0.05).astype(np.float32) for _ in range(N_FILES)]

for budget in (2, 48):
    logs = e.run_long_windows(files, max_new=budget)  # warm: graphs captured, arena allocated
    clips = [files[f][w[0] * 160: w[0] * 160 + 480000] for f, log in enumerate(logs) for w in log]
    n_win = len(clips)
    passes = 1 + max(w[4] for log in logs for w in log)

    def as_clips():
        for i in range(0, n_win, N_FILES):
            e.run_timestamp_tokens_batch(clips[i:i + N_FILES], max_new=budget)

    as_clips()  # warm
    a, b, fe = [], [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        as_clips()
        a.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        e.run_long_windows(files, max_new=budget)
        b.append(time.perf_counter() - t0)
        fe.append(e.timings()["frontend_ms"])
    ma, mb = float(np.median(a)), float(np.median(b))
    print(f"budget {budget:2d}: {n_win} windows in {passes} passes | clips in batches of {N_FILES}: {n_win / ma:.1f} windows/s ({1e3 * ma:.1f} ms) | "
          f"long-form: {n_win / mb:.1f} windows/s ({1e3 * mb:.1f} ms, of which upload + whole-file front-end {float(np.median(fe)):.1f} ms) | "
          f"ratio {ma / mb:.4f}  (A {['%.1f' % (1e3 * x) for x in a]} B {['%.1f' % (1e3 * x) for x in b]})", flush=True)

iters = 20
base = []
for _ in range(ROUNDS):
    base.append(e.bench("frontend", 1, 0, iters) / iters)
print(f"frontend (one 30 s clip, each launch waits for its length upload): {float(np.median(base)):.4f} ms", flush=True)
for seconds in (30, 300, 3600):
    ms = [e.bench("frontend_long", 1, seconds, iters) / iters for _ in range(ROUNDS)]
    m = float(np.median(ms))
    print(f"frontend_long one file of {seconds:4d} s: {m:.4f} ms = {m * 30 / seconds:.4f} ms per 30 s  ({['%.4f' % x for x in ms]})", flush=True)
e.close()
