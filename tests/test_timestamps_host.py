"""CPU: the segment-timestamp contract off the GPU — the Python rules on hand-built rows, AX_WHISPER_SplitSegments against the
segmenter's pseudo-code on seeded sequences, the rules kernel's resources in both builds, and the four new exports."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import ts_reference as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["AX_WHISPER_RunPCMBatchTimestampTokens", "AX_WHISPER_DecodeForcedTimestamps", "AX_WHISPER_ApplyTimestampRules",
               "AX_WHISPER_SplitSegments"]


@pytest.mark.parametrize("nv", [51865, 51866])
def test_python_rules_on_crafted_rows(nv):
    cases = tsr.crafted_cases(nv)
    for name, x, seq, want in cases:
        got, _ = tsr.decide(x, seq, 50364 if nv == 51865 else 50365, 50257)
        assert got == want, (name, got, want)
    # every branch of rules 2 and 5 is among them
    T = 50364 if nv == 51865 else 50365
    infos = [tsr.decide(x, seq, T, 50257)[1] for _, x, seq, _ in cases]
    assert {i["branch2"] for i in infos} >= {"open", "closed", None}
    assert {i["rule5"] for i in infos} == {True, False}


def test_python_allowed_sets():
    T, E, nv = 50364, 50257, 51865
    ok = tsr.allowed([], T, E, nv)
    assert not ok[:T].any() and ok[T:T + 51].all() and not ok[T + 51:].any()
    ok = tsr.allowed([T + 20, 5, T + 30], T, E, nv)  # pair open: text masked, eot kept, t_last itself allowed
    assert not ok[:E].any() and ok[E] and not ok[E + 1:T + 30].any() and ok[T + 30:].all()
    ok = tsr.allowed([T + 20, 5], T, E, nv)          # after text: strictly later timestamps
    assert ok[:E + 1].all() and not ok[E + 1:T + 21].any() and ok[T + 21:].all()


def _random_ids(rng, T, E, nv):
    n = rng.randrange(0, 64)
    kind = rng.random()
    if kind < 0.5:  # grammatical: pairs of rising timestamps around text runs, sometimes a dangling tail
        out, t = [], T + rng.randrange(0, 10)
        while len(out) < n:
            out.append(t)
            out += [rng.randrange(0, E) for _ in range(rng.randrange(0, 5))]
            t = min(t + rng.randrange(0, 40), nv - 1)
            if rng.random() < 0.85:
                out.append(t)
        return out[:n]
    pool = lambda: rng.choice([rng.randrange(0, E), rng.randrange(T, nv), rng.randrange(E, T), T, rng.randrange(-5, 0), nv + 7])
    return [pool() for _ in range(n)]


def test_split_segments_matches_the_pseudo_code(built_lib):
    L = built_lib.load_library()
    rng = random.Random(1234)
    pi = C.POINTER(C.c_int)
    for it in range(10000):
        nv = 51865 if it % 2 else 51866
        T, E = (50364 if nv == 51865 else 50365), 50257
        ids = _random_ids(rng, T, E, nv)
        clip = rng.choice([30.0, 7.25, 0.5])
        want = tsr.split_segments(ids, T, E, clip)
        n_max = rng.choice([len(ids) // 2 + 1, 0, 1, 2]) if it % 7 == 0 else len(ids) // 2 + 1
        pad = 4  # canaries past n_max must survive
        st, en = np.full(n_max + pad, -7.0, dtype=np.float32), np.full(n_max + pad, -7.0, dtype=np.float32)
        tb, te = np.full(n_max + pad, -7, dtype=np.int32), np.full(n_max + pad, -7, dtype=np.int32)
        a = np.asarray(ids, dtype=np.int32)
        n = C.c_int(-1)
        rc = L.AX_WHISPER_SplitSegments(a.ctypes.data_as(built_lib.ip), len(a), T, E, clip, n_max, st.ctypes.data_as(built_lib.fp),
                                        en.ctypes.data_as(built_lib.fp), tb.ctypes.data_as(pi), te.ctypes.data_as(pi), C.byref(n))
        assert rc == 0
        assert n.value == min(len(want), n_max), (ids, want, n.value)
        assert (st[n_max:] == -7.0).all() and (en[n_max:] == -7.0).all() and (tb[n_max:] == -7).all() and (te[n_max:] == -7).all()
        for k in range(n.value):
            s, e, b, f = want[k]
            assert np.isclose(st[k], s, rtol=1e-6, atol=1e-5) and np.isclose(en[k], e, rtol=1e-6, atol=1e-5) and tb[k] == b and te[k] == f, (ids, k, want)
    # segment text ranges of grammatical ids hold no timestamp
    ids = [50364, 1, 2, 50400, 50400, 3, 50500, 50500, 4]
    segs = built_lib.split_segments(ids, 50364, 50257, 12.0)
    assert [(round(s, 2), round(e, 2)) for s, e, _, _ in segs] == [(0.0, 0.72), (0.72, 2.72), (2.72, 12.0)]
    assert all(i < 50364 for _, _, b, f in segs for i in ids[b:f])


def test_split_segments_rejects_bad_arguments(built_lib):
    L = built_lib.load_library()
    n = C.c_int()
    assert L.AX_WHISPER_SplitSegments(None, 3, 50364, 50257, 1.0, 0, None, None, None, None, C.byref(n)) == -1
    assert L.AX_WHISPER_SplitSegments(None, 0, 50364, 50257, 1.0, 0, None, None, None, None, C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_rules_kernel_compiles_without_scratch_or_spills(f16, tmp_path):
    out = tmp_path / "ts.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out),
                        os.path.join(ROOT, "whisper.axera_amd", "csrc", "decode_timestamps.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    assert any("timestamp_rules_kernel" in n for n in names), names
    assert re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M) == ["0"] * len(names)
    assert all(int(x) == 0 for x in re.findall(r"^\s+\.(?:vgpr|sgpr)_spill_count:\s+(\d+)", text, re.M))


def test_new_symbols_are_exported(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
