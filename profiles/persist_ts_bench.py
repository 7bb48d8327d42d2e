"""One clip in timestamp and scored mode through the persistent launch's rules instantiation against the
launch-per-phase step (Whisper-small dims, synthetic weights, one MI355X). Two handles in one process — the route on (AX_WHISPER_PERSIST_TS=1)
and off (the default, the parent's route) — alternating, medians and spread of the decode stage (GetTimings):

1. one clip, a budget of 440 ids: plain mode through the persistent launch; timestamp and scored mode through the new route;
   timestamp and scored mode with the switch off;
2. one file through the seek loop, switch on and off: windows per second. The workload is (a) of profiles/long_chunked_bench.py
   (run_long_windows, ONE file of 3600 s, a budget of 224 ids per window), not the 16 files of profiles/longform_bench.py: the route
   takes a pass only when one file is decoded, and (a) is the workload behind the 9.5 windows/s of profiles/long_chunked_bench.txt
   that the one-clip cost was quoted from."""
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
ROUNDS, IDS = 7, 440
FILE_SECONDS = int(os.environ.get("AXW_BENCH_FILE_SECONDS", "3600"))


def say(line):
    print(line, flush=True)


os.environ["AX_WHISPER_PERSIST_TS"] = "1"
on = wa.Whisper("small", mdir, "zh", device=0, max_batch=1)
os.environ["AX_WHISPER_PERSIST_TS"] = "0"
off = wa.Whisper("small", mdir, "zh", device=0, max_batch=1)
del os.environ["AX_WHISPER_PERSIST_TS"]
assert on.get_config_int("persistent_ts") == 1 and off.get_config_int("persistent_ts") == 0
rng = np.random.default_rng(0)
clip = (rng.standard_normal(16000 * 30) * 0.05).astype(np.float32)

arms = {
    "plain, persistent launch": lambda: on.run_tokens(clip, max_new=IDS),
    "timestamps, rules in the launch": lambda: on.run_timestamp_tokens_batch([clip], max_new=IDS)[0],
    "scored, rules in the launch": lambda: on.run_timestamp_scores_batch([clip], max_new=IDS)[0]["ids"],
    "timestamps, switch off": lambda: off.run_timestamp_tokens_batch([clip], max_new=IDS)[0],
    "scored, switch off": lambda: off.run_timestamp_scores_batch([clip], max_new=IDS)[0]["ids"],
}
handle = {k: (off if "off" in k else on) for k in arms}
ms = {k: [] for k in arms}
n_ids = {}
for k, fn in arms.items():  # warm: graphs captured, buffers allocated
    n_ids[k] = len(fn())
c0 = on.persistent_ts_launches
for _ in range(ROUNDS):
    for k, fn in arms.items():
        fn()
        ms[k].append(handle[k].timings()["decode_ms"])
assert on.persistent_ts_launches == c0 + 2 * ROUNDS and off.persistent_ts_launches == 0 and on.get_config_int("persistent_giveups") == 0
say(f"# one clip, Whisper-small dims, budget {IDS} ids, decode stage, {ROUNDS} rounds alternating in one process: median [min .. max] ms")
med = {}
for k in arms:
    med[k] = float(np.median(ms[k]))
    say(f"{k:34s}: {n_ids[k]:3d} ids  {med[k]:8.2f} [{min(ms[k]):.2f} .. {max(ms[k]):.2f}]")
for mode in ("timestamps", "scored"):
    a, b = med[f"{mode}, rules in the launch"], med[f"{mode}, switch off"]
    say(f"{mode}: {b / a:.2f}x the switched-off route; {a / med['plain, persistent launch']:.3f}x the plain launch")

audio = (rng.standard_normal(16000 * FILE_SECONDS) * 0.05).astype(np.float32)
sec = {"on": [], "off": []}
nwin = {}
for name, e in (("on", on), ("off", off)):
    nwin[name] = len(e.run_long_windows([audio], max_new=224)[0])  # warm
c0 = on.persistent_ts_launches
for _ in range(3):
    for name, e in (("on", on), ("off", off)):
        t0 = time.perf_counter()
        e.run_long_windows([audio], max_new=224)
        sec[name].append(time.perf_counter() - t0)
assert on.persistent_ts_launches == c0 + 3 * nwin["on"]
say(f"# the seek loop over one file of {FILE_SECONDS} s, budget 224 ids per window, 3 rounds alternating: windows/s (seconds)")
for name in ("on", "off"):
    m = float(np.median(sec[name]))
    say(f"switch {name:3s}: {nwin[name]} windows, {nwin[name] / m:.1f} windows/s ({m:.2f} s; {['%.2f' % x for x in sec[name]]})")
on.close()
off.close()
