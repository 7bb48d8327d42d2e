"""Sample-rate conversion: the resample kernel beside the STFT pass of the same batch — DESIGN.md §11 "Sample rates".
Bench("resample") for clips of 30 s at 8000, 44100 and 48000 Hz and Bench("frontend") for clips of 30 s, at 1 and 64 clips, on
Whisper-small dims (synthetic weights, bf16; neither kernel depends on the model beyond n_mels). One handle, every shape warmed by a
first call, then AXW_BENCH_ROUNDS rounds (default 5) alternating over the shapes, 20 launches back to back per timed call between two
device events; medians per launch. The floor of a shape is the larger of its multiply-adds over the chip's fp32 vector peak and its
traffic over the HBM peak (PEAK_* below, from the vendor's data sheet for the MI355X: 157.3 TFLOP/s fp32 vector, 8 TB/s).

    python profiles/resample_bench.py > profiles/resample_bench.txt"""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
PEAK_FLOPS = 157.3e12
PEAK_BYTES = 8.0e12
RATES = (8000, 44100, 48000)
ITERS = 20


def floor_ms(rate, B, filt):
    L, M, K = filt
    n_in, n_out = 30 * rate, 480000
    flop = 2.0 * B * n_out * 2 * K
    traffic = 4.0 * B * (n_in + n_out)
    return flop, traffic, 1e3 * max(flop / PEAK_FLOPS, traffic / PEAK_BYTES)


if __name__ == "__main__":
    import modelgen
    import whisper_axera_amd as wa

    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=64)
    shapes = [("frontend", 0, B) for B in (1, 64)] + [("resample", r, B) for r in RATES for B in (1, 64)]
    got = {s: [] for s in shapes}
    for what, arg, B in shapes:
        e.bench(what, B, arg, 2)  # warm: tables, staging, code objects
    for _ in range(rounds):
        for s in shapes:
            what, arg, B = s
            got[s].append(e.bench(what, B, arg, ITERS) / ITERS)
    e.close()
    fe = {B: float(np.median(got[("frontend", 0, B)])) for B in (1, 64)}
    for B in (1, 64):
        print(f"frontend  16000 Hz x {B:2d} clips of 30 s: {fe[B]:8.4f} ms per pass  (rounds: {['%.4f' % x for x in got[('frontend', 0, B)]]})")
    for what, rate, B in shapes[2:]:
        filt = wa.resample_filter(rate)[:3]
        ms = float(np.median(got[(what, rate, B)]))
        flop, traffic, fl = floor_ms(rate, B, filt)
        print(f"resample {rate:6d} Hz x {B:2d} clips of 30 s (L {filt[0]}, M {filt[1]}, {2 * filt[2]} taps): {ms:8.4f} ms per launch = {ms / fe[B]:5.2f} x the STFT pass; "
              f"{flop:.3g} flop, {traffic / 1e6:.1f} MB, floor {fl:.4f} ms, {ms / fl:6.1f} x the floor  (rounds: {['%.4f' % x for x in got[(what, rate, B)]]})")
