"""Timestamp mode's cost per decoder step: Bench("decode_step_ts") against Bench("decode_step") at 1, 4 and 64 clips
(Whisper-small dims, synthetic weights, decode offset 224), run alternately A/B/A/B; plus one timestamp-mode greedy call of
one clip (the launch-per-phase step: timestamp mode does not use the persistent launch) against the plain one."""
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
iters, rounds = 50, 4
e = wa.Whisper("small", mdir, "zh", device=0, max_batch=64)
for B in [int(x) for x in (sys.argv[1:] or ["1", "4", "64"])]:
    a, b = [], []
    for _ in range(rounds):
        a.append(e.bench("decode_step", B, 224, iters) / iters)
        b.append(e.bench("decode_step_ts", B, 224, iters) / iters)
    ma, mb = float(np.median(a)), float(np.median(b))
    print(f"B {B:3d} decode_step ms {ma:.4f} decode_step_ts ms {mb:.4f} ratio {mb / ma:.4f}  (A {['%.4f' % x for x in a]} B {['%.4f' % x for x in b]})", flush=True)
pcm = (np.random.default_rng(0).standard_normal(16000 * 10) * 0.05).astype(np.float32)
for label, fn in [("plain", lambda: e.run_tokens_batch([pcm], max_new=440)), ("timestamps", lambda: e.run_timestamp_tokens_batch([pcm], max_new=440))]:
    fn()
    t0 = time.perf_counter()
    ids = fn()[0]
    t = e.timings()
    print(f"one clip {label}: {len(ids)} ids, decode {t['decode_ms']:.1f} ms, {t['steps']} steps, wall {1e3 * (time.perf_counter() - t0):.1f} ms", flush=True)
e.close()
