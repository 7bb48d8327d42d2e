"""A/B of the one-clip persistent launch with and without resident vocabulary rows (AX_WHISPER_VOCAB_RESIDENT), inside ONE process:
two handles of Whisper-small, alternating full-context decodes of the same 30 s clip, timings()["decode_ms"] per clip.
usage: vocab_resident_ab.py [pairs 8]      prints the per-arm values, mean, standard deviation and the verdict (gain > 3 x larger std)"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))
import numpy as np
import torch  # noqa: F401  (first: libax_whisper.so then binds to the HIP runtime torch ships, as in bench.py)
import modelgen
import whisper_axera_amd as wa

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
mdir = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
if not os.path.exists(os.path.join(mdir, "small", "small.safetensors")):
    modelgen.write_model_dir(mdir, "small", seed=0)
clip = modelgen.synth_clip(0, 480000)


def engine(resident):
    if resident:
        os.environ.pop("AX_WHISPER_VOCAB_RESIDENT", None)
    else:
        os.environ["AX_WHISPER_VOCAB_RESIDENT"] = "0"
    e = wa.Whisper("small", mdir, "zh", device=0, max_batch=1)  # the switch is read at construction
    os.environ.pop("AX_WHISPER_VOCAB_RESIDENT", None)
    return e


arms = {"resident": engine(True), "streamed": engine(False)}
rows = {k: e.L.AX_WHISPER_GetConfigInt(e.h, b"vocab_resident_rows") for k, e in arms.items()}
print("vocab_resident_rows:", rows, flush=True)
ids = {}
for k, e in arms.items():  # warm-up, and the ids must agree
    for _ in range(2):
        ids[k] = e.run_tokens(clip)
assert ids["resident"] == ids["streamed"] and len(ids["resident"]) == 444, (len(ids["resident"]), len(ids["streamed"]))
ms = {k: [] for k in arms}
for i in range(pairs):
    for k in (("streamed", "resident") if i % 2 == 0 else ("resident", "streamed")):
        arms[k].run_tokens(clip)
        ms[k].append(float(arms[k].timings()["decode_ms"]))
for k in ms:
    print(f"{k:9s} decode_ms per clip: " + " ".join(f"{v:.3f}" for v in ms[k]), flush=True)
m = {k: float(np.mean(v)) for k, v in ms.items()}
s = {k: float(np.std(v, ddof=1)) for k, v in ms.items()}
gain = m["streamed"] - m["resident"]
print(f"mean streamed {m['streamed']:.3f} (std {s['streamed']:.3f})  resident {m['resident']:.3f} (std {s['resident']:.3f})  gain {gain:.3f} ms per clip"
      f" = {100 * gain / m['streamed']:.2f} %;  3 x larger std = {3 * max(s.values()):.3f}: {'counts' if gain > 3 * max(s.values()) else 'does not count'}")
for e in arms.values():
    e.close()
