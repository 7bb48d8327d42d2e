"""The FP8 cross K/V switch (DESIGN.md "FP8 cross K/V") against the default h16 handle: Whisper-small dims, synthetic weights, one
MI355X. One process per handle, the modes alternating (h16, fp8, h16, fp8, ...: ROUNDS processes each), every figure the median
over the rounds with [min .. max]; the h16 rounds among themselves are the A/A spread a difference has to exceed. With
AXW_BENCH_PARENT_LIB=<a libax_whisper.so built from the commit before the switch> that library's default handle is a third mode in
the same rotation ("parent"): the default handle of this tree has to sit within the spread of it.

Per process: Bench("decode_attn") and Bench("decode_step") at t = 224 for 4, 16, 64, 128 and 256 clips (ms per step, ITERS replays of
the captured step between two events), Bench("encoder") per clip at 16 clips and — fp8 handle — Bench("cross_kv_quant") per clip
beside it, and the clips/s of a 64-clip greedy decode with a budget of 100 ids (host clock around decode_greedy, which ends in a
synchronise). --turbo adds turbo dims in the fp16 build at 16 clips (decode_attn and decode_step). Last, the share of greedy ids
that differ between an h16 and an fp8 handle on the five models of the model_real_* goldens (realistic activation statistics),
the golden's clip and three seeded ones in one 4-clip call, 32 ids per clip.

    python profiles/cross_kv_fp8_bench.py [--turbo] > profiles/cross_kv_fp8_bench.txt
"""
import os
import subprocess
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "whisper.axera_amd", "tools"))

MDIR = os.environ.get("AXW_BENCH_MODEL_DIR", "/tmp/axw_bench_models")
ROUNDS = int(os.environ.get("AXW_BENCH_ROUNDS", "3"))
ITERS, T = 200, 224
CLIPS = (4, 16, 64, 128, 256)


def child(mode, model):
    import whisper_axera_amd as wa

    small = model == "small"
    if mode == "parent":  # the library of the commit before the switch: it has neither the two new symbols nor the variable
        wa.LIB_PATH = os.environ["AXW_BENCH_PARENT_LIB"]
        for name in ("AX_WHISPER_GetCrossKVFp8", "AX_WHISPER_CrossKVQuantize"):
            wa.SYMBOLS.pop(name)
        e = wa.Whisper(model, MDIR, "zh", device=0, max_batch=256 if small else 16)
    else:
        e = wa.Whisper(model, MDIR, "zh", device=0, max_batch=256 if small else 16, cross_kv=mode)
        assert e.get_config_int("cross_kv_fp8") == (1 if mode == "fp8" else 0)
    out = {}
    enc_clips = 16
    # the cross K/V (and, fp8, the codes) of 16 slots; the other slots of the larger steps hold their zero-initialised images (scale 0,
    # code 0 on the fp8 handle): the kernels' time does not depend on the values
    e.bench("encoder", enc_clips, 0, 1)
    for b in CLIPS if small else (16,):
        for what in ("decode_attn", "decode_step"):
            e.bench(what, b, T, 20)  # warm: capture, first replays
            out[f"{what} {b}"] = e.bench(what, b, T, ITERS) / ITERS
    if small:
        out["encoder per clip"] = e.bench("encoder", enc_clips, 0, 5) / 5 / enc_clips
        if mode == "fp8":
            out["cross_kv_quant per clip"] = e.bench("cross_kv_quant", enc_clips, 0, 20) / 20 / enc_clips
        rng = np.random.default_rng(0)
        mel = np.clip(rng.standard_normal((64, e.n_mels, 3000)).astype(np.float32) * 0.4, -1.0, 1.5)
        e.encode_mel(mel)
        n0 = e.get_config_int("cross_kv_fp8_launches")
        e.decode_greedy(64, max_new=100)  # warm
        if mode != "parent":
            assert (e.get_config_int("cross_kv_fp8_launches") > n0) == (mode == "fp8")
        best = []
        for _ in range(3):
            t0 = time.perf_counter()
            ids = e.decode_greedy(64, max_new=100)
            best.append(64 / (time.perf_counter() - t0))
        out["clips/s, 64 clips x 100 ids"] = float(np.median(best))
        out["ids per clip"] = float(np.mean([len(x) for x in ids]))
    e.close()
    for k, v in out.items():
        print(f"RESULT\t{k}\t{v:.6f}", flush=True)


REAL = (("real_micro_demo", "micro", 41, "zh"), ("real_mini_synth", "mini", 42, "zh"), ("real_miniturbo_synth", "miniturbo", 43, "yue"),
        ("real_tiny_demo", "tiny", 44, "zh"), ("real_small_demo", "small", 45, "zh"))  # tests/golden/make_model_goldens.py


def real_ids():
    """greedy ids of an h16 and an fp8 handle on the models of the model_real_* goldens: 4 clips per call (the batched step)"""
    import tempfile

    sys.path.insert(0, os.path.join(R, "tests", "golden"))
    import modelgen
    import whisper_axera_amd as wa
    from make_model_goldens_inputs import golden_mel, synth_mel

    for name, model, seed, lang in REAL:
        dims = modelgen.DIMS[model]
        with tempfile.TemporaryDirectory() as td:
            modelgen.write_model_dir(td, model, dims, weights=modelgen.realistic_weights(dims, seed),
                                     tiktoken_path=os.path.join(R, "tests", "golden", "multilingual.tiktoken"))
            mels = np.stack([golden_mel(name)] + [synth_mel(70 + i, dims["n_mels"], 3000 - 400 * i) for i in range(3)])
            got = {}
            for mode in ("h16", "fp8"):
                e = wa.Whisper(model, td, lang, device=0, max_batch=4, cross_kv=mode)
                e.encode_mel(mels)
                got[mode] = e.decode_greedy(4, max_new=32)
                e.close()
        n = sum(max(len(a), len(b)) for a, b in zip(got["h16"], got["fp8"]))
        diff = sum(sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b)) for a, b in zip(got["h16"], got["fp8"]))
        first = [next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None) for a, b in zip(got["h16"], got["fp8"])]
        print(f"RESULT\t{name}\t{diff} of {n} ids differ ({100.0 * diff / max(n, 1):.1f} %), first difference per clip at {first}", flush=True)


def ids_section():
    print("# greedy ids, h16 handle against fp8 handle, models of the model_real_* goldens (4 clips per call, 32 ids per clip)", flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "ids", "-"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child ids failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT\t"):
            print(ln.split("\t", 1)[1].replace("\t", ": "), flush=True)


def main():
    import modelgen

    turbo = "--turbo" in sys.argv
    modes = (("parent",) if os.environ.get("AXW_BENCH_PARENT_LIB") else ()) + ("h16", "fp8")
    for model in ("small",) + (("turbo",) if turbo else ()):
        if not os.path.exists(os.path.join(MDIR, model, f"{model}.safetensors")):
            modelgen.write_model_dir(MDIR, model, seed=0, **({"dtype": "F16"} if model == "turbo" else {}))
        res = {m: {} for m in ("parent", "h16", "fp8")}
        rounds = ROUNDS if model == "small" else min(ROUNDS, 2)
        for _ in range(rounds):
            for mode in modes:  # a fresh process per handle, the modes alternating
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", mode, model], capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"child {mode} {model} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                for ln in r.stdout.splitlines():
                    if ln.startswith("RESULT\t"):
                        _, k, v = ln.split("\t")
                        res[mode].setdefault(k, []).append(float(v))
        print(f"# {model} dims{' (fp16 build)' if model == 'turbo' else ''}, t = {T}, {ITERS} replays per figure, {rounds} processes per mode alternating ({' / '.join(modes)}): "
              f"median [min .. max]; ms per step unless the line says otherwise", flush=True)
        for k in res["h16"]:
            a = res["h16"][k]
            line = f"{k:30s} h16 {np.median(a):9.4f} [{min(a):.4f} .. {max(a):.4f}]"
            if k in res["parent"]:
                c = res["parent"][k]
                line = f"{k:30s} parent {np.median(c):9.4f} [{min(c):.4f} .. {max(c):.4f}]   " + line[31:]
            if k in res["fp8"]:
                b = res["fp8"][k]
                line += f"   fp8 {np.median(b):9.4f} [{min(b):.4f} .. {max(b):.4f}]   fp8 / h16 {np.median(b) / np.median(a):.3f}"
            print(line, flush=True)
        for k in res["fp8"]:
            if k not in res["h16"]:
                b = res["fp8"][k]
                print(f"{k:30s} fp8 {np.median(b):9.4f} [{min(b):.4f} .. {max(b):.4f}]", flush=True)
        if model == "small":
            ids_section()


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "child":
        real_ids() if sys.argv[2] == "ids" else child(sys.argv[2], sys.argv[3])
    else:
        main()
