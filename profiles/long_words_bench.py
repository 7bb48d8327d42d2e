"""Long-form word timestamps: what they cost (Whisper-small dims, bf16, synthetic weights, one MI355X).

  python profiles/long_words_bench.py logprob          one fresh process: Bench("word_logprob") and Bench("word_logprob_rows") at 60 and
                                                       220 ids x 1, 8, 64 clips, ms per call (host wall time, scratch allocation inside)
  python profiles/long_words_bench.py long N           one fresh process: N synthetic 10-minute files through run_long_windows with
                                                       and without word_timestamps, 48 ids per window: wall seconds, windows
  python profiles/long_words_bench.py                  the driver: the two above in fresh processes, alternating, three rounds each

The A/B inside one process alternates the two routes per size; the driver repeats whole processes so that a process's clock state
does not decide the comparison (see the spread between rounds in profiles/long_words_bench.txt)."""
import os
import subprocess
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))


def engine(max_batch):
    import modelgen
    import whisper_axera_amd as wa

    mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
    if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
        modelgen.write_model_dir(mdir, "small", seed=0)
    return wa.Whisper("small", mdir, "zh", device=0, max_batch=max_batch)


def logprob():
    e = engine(64)
    iters = 5
    for n_ids in (60, 220):
        for clips in (1, 8, 64):
            t = {"word_logprob": [], "word_logprob_rows": []}
            for _ in range(3):
                for what in t:
                    t[what].append(e.bench(what, clips, n_ids, iters) / iters)
            f, r = float(np.median(t["word_logprob"])), float(np.median(t["word_logprob_rows"]))
            print(f"logprob {clips:2d} clips x {n_ids:3d} ids: fused {f:8.3f} ms  rows {r:9.3f} ms  rows / fused {r / f:6.1f}  "
                  f"(fused {['%.3f' % x for x in t['word_logprob']]} rows {['%.3f' % x for x in t['word_logprob_rows']]})", flush=True)
    e.close()


def long(n_files):
    e = engine(max(n_files, 1))
    rng = np.random.default_rng(0)
    files = [(rng.standard_normal(16000 * 600) * 0.05).astype(np.float32) for _ in range(n_files)]
    for words in (None, True, None, True):
        t0 = time.perf_counter()
        out = e.run_long_windows(files, max_new=48, word_timestamps=words)
        dt = time.perf_counter() - t0
        logs = out[0] if words else out
        print(f"long {n_files} files of 600 s, word_timestamps {bool(words)}: {dt:7.3f} s, {sum(len(log) for log in logs)} windows, "
              f"{sum(len(w[-1]['words']) for log in logs for w in log) if words else 0} words", flush=True)
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "logprob":
        logprob()
    elif len(sys.argv) > 2 and sys.argv[1] == "long":
        long(int(sys.argv[2]))
    else:
        for rnd in range(3):
            for args in (["logprob"], ["long", "1"], ["long", "8"]):
                r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=900)
                if r.returncode != 0:  # a process that died: nothing more is started on the device
                    sys.exit(r.returncode)
