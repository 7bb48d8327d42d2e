"""The slot stream in timestamp mode against the plain slot stream and the batched scored step (Whisper-small dims, synthetic
weights, one MI355X). Writes profiles/stream_ts_bench.txt (AXW_BENCH_OUT: another file).

  1. bench.py's stream64 workload (384 clips of 30 s through 64 refilled slots, budgets U{60..150} ids, admitted as slots free up) in
     mode 0 (run_stream) and mode 1 (run_stream_timestamps), three alternating rounds after one warm-up each, medians in clips/s.
     Mode 1 walks its prefix step by step (two more steps per clip) and runs the logits dump and the rules kernel at every step, so it
     is not expected to reach mode 0; the figure says what a server pays for segments, scores and languages.
  2. Bench("stream_step_ts") beside Bench("decode_step_ts_scored") at 8 and 64 clips, three alternating rounds, medians in ms per
     step. Expectation: the mode-1 stream step costs no more than the batched scored step at the same clip count, plus that
     measurement's own round-to-round spread (the only addition is a branch at offset 0).

AXW_STREAM_TS_ROUNDS / AXW_STREAM_TS_CLIPS shrink the run for a first look."""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
import bench as headline  # noqa: E402  (realistic_budgets, N_SAMP: the workload is bench.py's)
import modelgen  # noqa: E402
import whisper_axera_amd as wa  # noqa: E402

mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
    modelgen.write_model_dir(mdir, "small", seed=0, tiktoken_path=os.path.join(R, "tests", "golden", "multilingual.tiktoken"))
ROUNDS = int(os.environ.get("AXW_STREAM_TS_ROUNDS", "3"))
N_CLIPS = int(os.environ.get("AXW_STREAM_TS_CLIPS", "384"))
SLOTS = 64
OUT = os.environ.get("AXW_BENCH_OUT", os.path.join(R, "profiles", "stream_ts_bench.txt"))
open(OUT, "w").close()


def say(line):  # (line by line: a run that is cut short leaves what it measured)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


distinct = [modelgen.synth_clip(i, headline.N_SAMP) for i in range(SLOTS)]
clips = [distinct[i % SLOTS] for i in range(N_CLIPS)]
budgets = headline.realistic_budgets(N_CLIPS, seed=20260105)
e = wa.Whisper("small", mdir, "zh", device=0, max_batch=SLOTS)


def mode0():
    got, _ = e.run_stream(clips, SLOTS, max_new=budgets)
    return sum(len(g) for g in got)


def mode1():
    got = e.run_stream_timestamps(clips, SLOTS, max_new=budgets)
    return sum(len(g[1]) for g in got)


say(f"stream64 workload: whisper-small bf16, {N_CLIPS} clips of 30 s through {SLOTS} refilled slots, budgets U{{60..150}} ids, {ROUNDS} alternating rounds")
for fn in (mode0, mode1):
    fn()  # warm: graphs, buffers
rates = {"mode0": [], "mode1": []}
for r in range(ROUNDS):
    for name, fn in (("mode0", mode0), ("mode1", mode1)):
        t0 = time.perf_counter()
        n_ids = fn()
        dt = time.perf_counter() - t0
        rates[name].append(N_CLIPS / dt)
        say(f"  round {r} {name}: {N_CLIPS / dt:8.2f} clips/s  ({dt:.3f} s, {n_ids / N_CLIPS:.1f} ids per clip)")
for name in rates:
    say(f"{name}: median {statistics.median(rates[name]):.2f} clips/s  (min {min(rates[name]):.2f}, max {max(rates[name]):.2f})")
say(f"mode1 / mode0: {statistics.median(rates['mode1']) / statistics.median(rates['mode0']):.3f}")

ITERS = 100
for n in (8, 64):
    ms = {"decode_step_ts_scored": [], "stream_step_ts": []}
    for r in range(ROUNDS):
        for what in ms:
            ms[what].append(e.bench(what, n, 100, ITERS) / ITERS)
    a, b = ms["decode_step_ts_scored"], ms["stream_step_ts"]
    spread = max(a) - min(a)
    say(f"{n:3d} clips, step at offset 100: decode_step_ts_scored {statistics.median(a):.4f} ms (rounds {', '.join('%.4f' % x for x in a)}), "
        f"stream_step_ts {statistics.median(b):.4f} ms (rounds {', '.join('%.4f' % x for x in b)})")
    verdict = "within" if statistics.median(b) <= statistics.median(a) + spread else "ABOVE"
    say(f"     stream step - scored step = {statistics.median(b) - statistics.median(a):+.4f} ms; the scored step's own spread {spread:.4f} ms: {verdict} the expectation")
e.close()
