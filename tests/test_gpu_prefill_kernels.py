"""GPU: the prompt-prefill kernels alone (whisper.axera_amd/csrc/decode_prefill.hip) through tests/cpp/prefill_kernels_driver.cpp,
against float64 references with per-element bounds derived from the rounding points (notation of tests/decode_kernel_reference.py:
u = 2^-24, u16 = 2^-8 bfloat16 / 2^-11 half, hulp = half an ulp of the 16-bit type).

embed        x = tok_emb[ctx] + pos[row_pos]: one fp32 addition of an exact widening and an fp32 value -> bit-equal to numpy's.
cache store  a copy: the K / V rows of every context position bit-equal at the index maps of decode_kernel_reference.py (restated
             from decode_layout.hpp, compared element for element by the CPU suite); every other element of every slot keeps its fill.
attention    s_j = 0.125 q.k_j over the keys the query sees, w = softmax(s), o = sum_j w_j v_j; q, K, V are h16 and exact.
  scores: 64 exact products summed in fp32 by the matrix core:  ds_j = 0.125 * 65 u sum_d |q_d k_jd| + u |s_j|
  weights: exp2(s sc - m sc) by one FMA and v_exp_f32, carried through C = blocks + 2 rescalings of the online softmax:
           eps_j = ds_j + u (3 C + 2 (s_max - s_j))            (decode_kernel_reference.py, "Attention")
  the numerator's weights are narrowed to h16 (the denominator's are not): u16 w_j |v_j| (+ 2^-25 |v_j| in half: subnormal weights)
  fp32 sums of n terms, the rescalings, the division: (n + C + 3) u PV, PV = sum_j w_j |v_j|
  E = 2 sum_j w_j eps_j (|v_j| + |o|) + u16 PV (+ 2^-25 sum_j |v_j|) + (n + C + 3) u PV, and the h16 store: + hulp(|o| + E)
  Keys beyond what a clip may see hold NaN in the caches: nothing of them may reach an output, and output rows at or
  beyond the length keep their fill."""
import os
import subprocess

import numpy as np
import pytest

import decode_kernel_reference as dkr
from encoder_kernel_reference import SENT16, from_bits, hulp, to_bits, u16
from kernel_driver import BUILD, HIPCC, PKG, ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LENGTHS = (1, 4, 63, 64, 65, 129, 226)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def driver(request, built_lib):
    """build/prefill_kernels_driver.<dt>, linked against the decode_prefill object of that build"""
    dt = request.param
    exe = os.path.join(BUILD, "prefill_kernels_driver." + dt)
    src = os.path.join(ROOT, "tests", "cpp", "prefill_kernels_driver.cpp")
    obj = os.path.join(BUILD, f"decode_prefill.{dt}.o")
    deps = [src] + [os.path.join(PKG, "csrc", f) for f in ("decode_prefill.hip", "common.hpp", "decode_layout.hpp")]
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(f) for f in deps)):
        if not os.path.exists(obj) or os.path.getsize(obj) == 0 or os.path.getmtime(obj) < max(os.path.getmtime(f) for f in deps[1:]):
            r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DAXW_F16=" + ("1" if dt == "f16" else "0"),
                                "-I" + os.path.join(ROOT, "include"), "-c", deps[1], "-o", exe + ".kernels.o"], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            obj = exe + ".kernels.o"
        for cmd in ([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DAXW_F16=" + ("1" if dt == "f16" else "0"),
                     "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-c", src, "-o", exe + ".o"],
                    [HIPCC, "--offload-arch=gfx950", exe + ".o", obj, "-o", exe]):
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
    return dt, exe


def _run(exe, mode, tmp_path, head, arrays, tag):
    fin, fout = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    with open(fin, "wb") as f:
        f.write(np.array((list(head) + [0] * 8)[:8], dtype=np.int32).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), (mode, tag, r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return np.fromfile(fout, dtype=np.uint8)


def _tables(lens, slots):
    row0 = np.cumsum([0] + list(lens[:-1])).astype(np.int32)
    row_pos = np.concatenate([np.arange(L) for L in lens]).astype(np.int32)
    row_slot = np.concatenate([np.full(L, s) for L, s in zip(lens, slots)]).astype(np.int32)
    return row0, row_pos, row_slot


def test_embed(driver, tmp_path):
    dt, exe = driver
    rng = np.random.default_rng(5)
    d, nv, npos = 192, 300, 230
    lens = (226, 1, 65)
    _, row_pos, _ = _tables(lens, (0, 1, 2))
    rows = len(row_pos)
    ctx = rng.integers(0, nv, rows).astype(np.int32)
    emb = to_bits(rng.standard_normal((nv, d)), dt)
    pos = rng.standard_normal((npos, d)).astype(np.float32)
    got = _run(exe, "embed", tmp_path, (rows, d, nv, npos), (ctx, row_pos, emb, pos), "embed").view(np.float32).reshape(rows, d)
    want = from_bits(emb, dt).astype(np.float32)[ctx] + pos[row_pos]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("H", [2, 4])
def test_cache_store(driver, tmp_path, H):
    """Ragged clips in slots 3 and 1 of four: their rows [0, L) hold the K / V columns, everything else its fill."""
    dt, exe = driver
    rng = np.random.default_rng(7 + H)
    d, pad, slots = 64 * H, 448, 4
    lens, where = (129, 64), (3, 1)
    _, row_pos, row_slot = _tables(lens, where)
    rows = len(row_pos)
    qkv = to_bits(rng.standard_normal((rows, 3 * d)), dt)
    fill = np.full(slots * H * pad * 64, SENT16, dtype=np.uint16)
    out = _run(exe, "store", tmp_path, (rows, d, pad, slots), (row_pos, row_slot, qkv, fill, fill), "store%d" % H).view(np.uint16)
    k, v = out[: fill.size].reshape(slots, H, pad * 64), out[fill.size:].reshape(slots, H, pad * 64)
    want_k, want_v = fill.reshape(slots, H, pad * 64).copy(), fill.reshape(slots, H, pad * 64).copy()
    dd = np.arange(64)
    for r in range(rows):
        for h in range(H):
            want_k[row_slot[r], h, dkr.kcache_index(row_pos[r], dd)] = qkv[r, d + 64 * h: d + 64 * h + 64]
            want_v[row_slot[r], h, dkr.vcache_index(row_pos[r], dd)] = qkv[r, 2 * d + 64 * h: 2 * d + 64 * h + 64]
    assert np.array_equal(k, want_k) and np.array_equal(v, want_v)
    assert (k[0] == SENT16).all() and (k[2] == SENT16).all() and (v[0] == SENT16).all() and (v[2] == SENT16).all()  # neighbouring slots


def _attention_case(dt, exe, tmp_path, rng, H, lens, where, slots, pad, n_keys, ldq, tag):
    """One launch; returns the worst error / bound. n_keys < 0: causal over the self cache."""
    d = 64 * H
    row0, row_pos, _ = _tables(lens, where)
    rows = int(sum(lens))
    nan16 = np.uint16(SENT16)
    q = to_bits(rng.standard_normal((rows, ldq)) * 1.5, dt)
    kn = rng.standard_normal((slots, H, pad, 64))
    vn = rng.standard_normal((slots, H, pad, 64))
    kb, vb = to_bits(kn, dt).reshape(slots, H, pad, 64), to_bits(vn, dt).reshape(slots, H, pad, 64)
    for L, s in zip(lens, where):  # what no query of the clip may see
        lim = L if n_keys < 0 else n_keys
        kb[s, :, lim:], vb[s, :, lim:] = nan16, nan16
    kc, vc = np.empty((slots, H, pad * 64), dtype=np.uint16), np.empty((slots, H, pad * 64), dtype=np.uint16)
    key, dd = np.meshgrid(np.arange(pad), np.arange(64), indexing="ij")
    kc[:, :, dkr.kcache_index(key, dd)] = kb
    vc[:, :, dkr.vcache_index(key, dd)] = vb
    out0 = np.full((rows, d), SENT16, dtype=np.uint16)
    got = _run(exe, "attn", tmp_path, (len(lens), H, pad, n_keys, slots, ldq, rows, max(lens)), (row0, np.array(lens, dtype=np.int32),
               np.array(where, dtype=np.int32), q, kc, vc, out0), tag).view(np.uint16).reshape(rows, d)
    worst = 0.0
    q64, k64, v64 = from_bits(q, dt).reshape(rows, ldq), from_bits(kb, dt), from_bits(vb, dt)
    for c, (L, s) in enumerate(zip(lens, where)):
        for i in range(L):
            n = i + 1 if n_keys < 0 else n_keys
            C = (n + 63) // 64 + 2
            for h in range(H):
                qq, K, V = q64[row0[c] + i, 64 * h: 64 * h + 64], k64[s, h, :n], v64[s, h, :n]
                sj = 0.125 * (K @ qq)
                w = np.exp(sj - sj.max())
                w /= w.sum()
                o = w @ V
                ds = 0.125 * 65 * U * (np.abs(K) @ np.abs(qq)) + U * np.abs(sj)
                eps = ds + U * (3 * C + 2 * (sj.max() - sj))
                PV = w @ np.abs(V)
                E = 2 * ((w * eps) @ (np.abs(V) + np.abs(o))) + u16(dt) * PV + (n + C + 3) * U * PV
                if dt == "f16":
                    E = E + 2.0 ** -25 * np.abs(V).sum(axis=0)
                bound = E + hulp(np.abs(o) + E, dt)
                g = from_bits(got[row0[c] + i, 64 * h: 64 * h + 64], dt)
                assert np.isfinite(g).all(), (tag, c, i, h)
                ratio = float((np.abs(g - o) / bound).max())
                assert ratio <= 1.0, (tag, "clip", c, "query", i, "head", h, ratio)
                worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("H", [2, 4])
def test_attention_self(driver, tmp_path, H):
    """Causal mode on every length, two clips of different length per launch, non-zero slots; q with the row stride of the QKV buffer."""
    dt, exe = driver
    rng = np.random.default_rng(11 + H)
    worst = 0.0
    for lens, where in (((1, 226), (2, 0)), ((129, 4), (1, 3)), ((63, 65), (3, 2)), ((64,), (1,))):
        worst = max(worst, _attention_case(dt, exe, tmp_path, rng, H, lens, where, 4, 448, -1, 3 * 64 * H, "self%d_%d" % (H, lens[0])))
    print("%s heads %d self: worst error / bound %.3f" % (dt, H, worst))


@pytest.mark.parametrize("H", [2, 4])
def test_attention_cross(driver, tmp_path, H):
    """Cross mode: 1500 keys in 24 blocks, the last one with 28; and a key count below one block."""
    dt, exe = driver
    rng = np.random.default_rng(13 + H)
    worst = _attention_case(dt, exe, tmp_path, rng, H, (65, 4), (1, 0), 2, 1536, 1500, 64 * H, "cross%d" % H)
    worst = max(worst, _attention_case(dt, exe, tmp_path, rng, H, (1, 64), (0, 1), 2, 1536, 28, 64 * H, "cross28_%d" % H))
    print("%s heads %d cross: worst error / bound %.3f" % (dt, H, worst))
