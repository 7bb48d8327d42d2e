"""Word alignment: the GPU route against the host route (DESIGN.md "Word-level timestamps"). Bench("word_align") and
Bench("word_align_host") on ONE handle (Whisper-small dims, synthetic weights, bf16), every slot with n_text text ids against all
1500 encoder frames, at n_text = 60 and 220 and 1, 8 and 64 clips; the two routes alternate, AXW_BENCH_ROUNDS rounds (default 5),
medians. One timed call is AX_WHISPER_AlignTokens without the matrix output: table upload, the teacher-forced prefill pass with the
QK-softmax kernel behind the cross-attention query GEMM of every aligned layer, then normalise + median + DTW on the GPU (word_align)
or on the host from the P scratch copied back layer by layer (word_align_host), the token log-probabilities, the results on the host.
Host wall time: both routes end on the host.

    python profiles/word_align_bench.py [clips ...] > profiles/word_align_bench.txt
    python profiles/word_align_bench.py --one gpu|host CLIPS N_TEXT ITERS     # one route alone (for a profiler run)"""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))

TARGET = {"gpu": "word_align", "host": "word_align_host"}


def engine(max_batch):
    import modelgen
    import whisper_axera_amd as wa

    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    return wa.Whisper("small", mdir, "zh", device=0, max_batch=max_batch)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        route, B, n, iters = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
        e = engine(B)
        print("%s clips %d n_text %d: %.3f ms per call" % (route, B, n, e.bench(TARGET[route], B, n, iters) / iters))
        e.close()
        sys.exit(0)
    clips = [int(x) for x in (sys.argv[1:] or ["1", "8", "64"])]
    rounds = int(os.environ.get("AXW_BENCH_ROUNDS", "5"))
    e = engine(max(clips))
    print("word_align route of the handle: %d (0 the kernels, 1 the host)" % e.get_config_int("word_align"))
    for B in clips:
        for n in (60, 220):
            it = {"gpu": 4 if B < 64 else 2, "host": 2 if B < 64 else 1}
            for r in it:  # warm: scratch, code objects
                e.bench(TARGET[r], B, n, 1)
            got = {"gpu": [], "host": []}
            for _ in range(rounds):
                for r in ("gpu", "host"):
                    got[r].append(e.bench(TARGET[r], B, n, it[r]) / it[r])
            a, b = float(np.median(got["gpu"])), float(np.median(got["host"]))
            print(f"clips {B:3d} n_text {n:3d}: kernels {a:10.3f} ms, host {b:10.3f} ms ({b / a:6.2f} x)"
                  f"  (rounds: {[['%.3f' % x for x in got[r]] for r in ('gpu', 'host')]})", flush=True)
    e.close()
