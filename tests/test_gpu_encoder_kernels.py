"""GPU: every encoder kernel alone, its WHOLE output against float64, both builds (bfloat16 and half).

tests/cpp/encoder_kernels_driver.cpp is linked against the objects `make` produced for libax_whisper.so (build/gemm.*.o,
build/encoder_attn.*.o), so what runs here is the shipped code. Each case is one launch — launch_gemm, launch_layernorm_bf16
or launch_encoder_attention — with the strides and offsets Engine::run_encoder (csrc/engine.cpp) gives it; every output buffer
comes back in full with its guards. tests/encoder_kernel_reference.py holds the float64 references and the per-element bounds
(derived in its docstring, no free constants); tests/test_encoder_kernel_reference.py shows without a GPU that a faithful
float32 emulation stays inside those bounds and that seeded defects do not. Everything a launch must not write (guards, h1 row
0 and its trailing row, V^T frames >= M, cross-K/V rows >= T and unmapped slots, partial slabs of other splits and clips) holds
a NaN sentinel before the launch and must hold it bit for bit afterwards.

GEMM: conv1, conv2, Q/K/V^T (whole and as the two side-by-side launches), out-proj and FFN2 (in-place residual onto a non-zero
C; split-K with every slice count the engine's rule picks, followed by the LayerNorm fold), FFN1, plain bias, cross K/V
(n_layer 2 and 4, more slots than clips, a non-identity slot map) at d 384 / 512 / 768 / 1024 / 1280 and 1-3 clips, plus per
launch one clip count (4, 8 or 15 at d = 768) that gives the stream kernel 270 / 288 tiles (more than the 256 CUs, not a
multiple) and the ring kernel >= 256; each under gemm_force_tile 0, 1, 2 and 5 with the kernel that really ran
(gemm_last_kernel) asserted. test_every_kernel_ran_every_epilogue counts kernel x epilogue x orientation per build.
LayerNorm: d 128 .. 2048, 1503 rows (not a multiple of 4), 0 / 2 / 3 / 4 partials, outlier channels, constant rows.
Attention: the engine's shape (T 1500, 2 / 6 / 20 heads, 1 / 3 clips) and the contract's edges (T 4, 64, 128, 132, 1472, 1476
with 3 heads x 3 clips), eight score families dealt over the (clip, head) pairs, thresholds 0 / 0.5 / 8 / 16, each against
float64, and finite garbage in the padded V^T frames changing no bit.

A driver run has its own timeout; after one that fails, nothing further is launched and the remaining cases fail at once.

Worst error / bound measured on MI355X (printed by -s), bf16 | fp16: GEMM bias 0.966 | 0.772, GELU 0.994 | 0.955, Q/K/V^T
0.983 | 0.885, cross K/V 0.984 | 0.887 (16-bit outputs: the output's half ulp dominates), conv2 0.008 | 0.007, residual
0.007 | 0.007, split-K partials 0.020 | 0.022 (fp32 outputs: any-order bound against the MFMA's real order); LayerNorm 1.000 |
1.000 (half-ulp ties), fold x 0.694 | 0.713, fold y 0.997 | 0.974; attention flat 0.379 | 0.373, falling 0.330 | 0.370, rising by 6
0.449 | 0.403, by 10 0.449 | 0.418, |score/8| ~ 300 0.249 | 0.089, dominant key 0.000 (the output is that key's v exactly).
Wall time 3.7 min (76 tests). In the fp16 build at threshold 16 a row maximum rising by 15.9997-16 log2 units overflows half
(tests/test_encoder_kernel_reference.py shows it; the engine stops that build at 15); none of the families here lands there."""
import os
import subprocess
import time

import numpy as np
import pytest

import encoder_kernel_reference as ekr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper.axera_amd")
BUILD = os.path.join(PKG, "build")
HIPCC = "/opt/rocm/bin/hipcc"
DTYPES = ("bf16", "f16")
WIDTHS = (384, 512, 768, 1024, 1280)
T = 1500

_state = {"dead": None, "t0": time.time()}
_ran = {dt: set() for dt in DTYPES}   # (kernel, epilogue, swapped) of every checked launch
_worst = {}


def _driver_exe(dt):
    """build/encoder_kernels_driver.<dt>, relinked whenever it is older than its source or the objects it links."""
    exe = os.path.join(BUILD, "encoder_kernels_driver." + dt)
    src = os.path.join(ROOT, "tests", "cpp", "encoder_kernels_driver.cpp")
    objs = [os.path.join(BUILD, f"{k}.{dt}.o") for k in ("gemm", "encoder_attn")]
    srcs = [src] + [os.path.join(PKG, "csrc", f) for f in ("gemm.hip", "encoder_attn.hip", "common.hpp", "decode_layout.hpp")]
    newest = max(os.path.getmtime(f) for f in srcs + [o for o in objs if os.path.exists(o)])
    if os.path.exists(exe) and os.path.getmtime(exe) >= newest:
        return exe
    r = subprocess.run(["make", "-C", PKG, "-j16"] + [os.path.relpath(o, PKG) for o in objs], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    obj = exe + ".o"
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DAXW_F16=" + ("1" if dt == "f16" else "0"),
                 "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj] + objs + ["-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, _driver_exe(request.param)


class Manifest:
    def __init__(self, tmp):
        self.tmp, self.lines, self.n = str(tmp), [], 0

    def path(self, name):
        return os.path.join(self.tmp, name)

    def alloc(self, name, content):
        """content: an array (initial content) — the driver adds the guards."""
        content = np.ascontiguousarray(content)
        self.n += 1
        f = self.path(f"in{self.n}.bin")
        content.tofile(f)
        self.lines.append(f"alloc {name} {content.nbytes} {f}")

    def add(self, line):
        self.lines.append(line)

    def dump(self, name, file, base=None):
        self.lines.append(f"dump {name} {self.path(file)}" + (f" {self.path(base)}" if base else ""))

    def run(self, exe, timeout):
        """One driver process. Returns {launch id: (kernel before, last kernel)}."""
        if _state["dead"]:
            pytest.fail("not run: an earlier driver run failed (" + _state["dead"] + ")")
        mf = self.path("manifest.txt")
        with open(mf, "w") as f:
            f.write("\n".join(self.lines) + "\n")
        try:
            r = subprocess.run([exe, mf], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _state["dead"] = "timeout"
            raise
        if r.returncode != 0 or not r.stdout.rstrip().endswith("done"):
            _state["dead"] = f"exit status {r.returncode}"
            pytest.fail(f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
        return {ln.split()[1]: (int(ln.split()[2]), int(ln.split()[3])) for ln in r.stdout.splitlines() if ln.startswith("ran ")}

    def load(self, file, may_be_same=False):
        """uint16 view of a dump, or None for one the driver found equal to its base and did not write. The file is removed."""
        f = self.path(file)
        if not os.path.exists(f):
            assert may_be_same, file
            return None
        a = np.fromfile(f, dtype=np.uint16)
        os.remove(f)
        return a


def note(dt, what, ratio):
    key = (dt, what)
    _worst[key] = max(_worst.get(key, 0.0), ratio)


# ------------------------------------------------------------------------------------------ GEMM
FORCES = (0, 1, 2, 5)
KEYS = ("epi", "M", "N", "K", "batch", "d", "t_pad", "nbt", "n_layer", "qkv_part", "ksplit", "lda", "a_bs", "ldc", "c_bs", "c2_bs",
        "c3_bs", "part_stride", "A", "A_off", "W", "bias", "C", "C_off", "aux", "C2", "C3", "slot_map", "part")


# the launcher's own choice where the tile arithmetic is easy to do by hand: (d, clips, case, first column) -> kernel.
# One clip: at most 40 x 6 tiles of 256x128, below the 256 CUs -> 128x128. mlp.0 at 768: 24 x 6 x 3 = 432 ring tiles but only
# 216 square ones -> ring; at 4 clips 288 square tiles would fill 288 / 512 of two rounds against 576 / 768 for the ring
# (1.15 x 0.5625 < 0.75) -> ring; the same sum keeps the 15-clip launches (270 square tiles) on the ring.
AUTO_KERNEL = {(768, 1, "ffn1", 0): 1, (768, 1, "qkv", 0): 1, (768, 1, "qkv", 1536): 1, (1280, 1, "ffn1", 0): 1, (1280, 1, "cross4", 0): 1,
               (768, 3, "ffn1", 0): 2, (1280, 2, "ffn1", 0): 2, (768, 4, "ffn1", 0): 2, (768, 15, "oproj_resid", 0): 2,
               (768, 15, "ffn2_resid", 0): 2, (384, 3, "oproj_resid", 0): 1, (768, 8, "conv1", 0): 2}


def gemm_cases(d, clips, family):
    """[(name, kind, kwargs)] of one width and clip count."""
    out = [(k, k, {}) for k in ("conv1", "conv2", "qkv", "qk", "v", "oproj_resid", "ffn2_resid", "ffn1")]
    out.append(("cross4", "cross", dict(n_layer=4)))
    if clips == 2 or family == "realistic":
        out.append(("cross2", "cross", dict(n_layer=2)))
    if d == 768:
        out.append(("bias", "bias", {}))
    for kind, K in (("oproj_part", d), ("ffn2_part", 4 * d)):
        for ks in sorted({ekr.split_k_rule(d, K, b) for b in (1, 2)} - {1}):  # every slice count the engine's rule can pick
            out.append((f"{kind}{ks}", kind, dict(ksplit=ks)))
    return out


def run_gemm_group(driver, tmp_path, d, clips, family, cases, forces=FORCES, seed0=0):
    dt, exe = driver
    m = Manifest(tmp_path)
    built = []
    for ci, (name, kind, kw) in enumerate(cases):
        p, bufs = ekr.gemm_case(kind, d, clips, dt, family, seed0 + 1000 * d + 100 * clips + ci, T=T, **kw)
        outs = [p[k] for k in ("C", "C2", "C3", "part") if p.get(k)]
        for bname, content in bufs.items():
            m.alloc(bname, content)
        args = " ".join(f"{k}={p[k]}" for k in KEYS if k in p)
        fold = None
        for force in (forces if p["epi"] != ekr.EPI_PARTIAL else (0,)):  # split-K has one kernel whatever is forced
            for o in outs:
                m.add(f"reset {o}")
            m.add(f"gemm {name}:{force} force={force} {args}")
            for o in outs:
                m.dump(o, f"{name}.{force}.{o}", None if force == forces[0] else f"{name}.{forces[0]}.{o}")
        if p["epi"] == ekr.EPI_PARTIAL:  # the LayerNorm that follows folds the partials the GPU just wrote
            rng = np.random.default_rng(seed0 + ci)
            rows = clips * T
            fold = dict(x=rng.standard_normal((rows, d)).astype(np.float32), g=rng.uniform(0.5, 1.5, d).astype(np.float32),
                        b=rng.uniform(-1, 1, d).astype(np.float32))
            m.alloc("x", fold["x"]); m.alloc("g", fold["g"]); m.alloc("b", fold["b"]); m.alloc("y", ekr.sentinel(rows * d, 2))
            m.add(f"ln {name}:fold x=x g=g b=b y=y rows={rows} d={d} part=part n_part={p['ksplit']} part_stride={p['part_stride']} part_bias=bias")
            m.dump("x", f"{name}.fold.x"); m.dump("y", f"{name}.fold.y")
            for b in ("x", "g", "b", "y"):
                m.add(f"free {b}")
        for bname in bufs:
            m.add(f"free {bname}")
        built.append((name, p, bufs, outs, fold))
    ran = m.run(exe, timeout=600)
    for name, p, bufs, outs, fold in built:
        exp = ekr.gemm_expect(p, bufs, dt)
        assert set(exp) == set(outs)
        cols = ekr.launches(p)
        gpu_part = None
        for force in (forces if p["epi"] != ekr.EPI_PARTIAL else (0,)):
            kernels = [k for k in ran[f"{name}:{force}"] if k][-len(cols):]
            assert len(kernels) == len(cols), (name, force, ran[f"{name}:{force}"])
            for (n0, nc), kernel in zip(cols, kernels):
                a_elems, nk = clips * p["a_bs"] + p["M"] * p["lda"], p["K"] // 64
                if p["epi"] == ekr.EPI_PARTIAL or force == 1:
                    assert kernel == 1, (name, force, kernel)   # gemm_bf16_kernel, 128x128
                elif force == 2:
                    assert kernel == 2, (name, force, kernel)   # gemm256_bf16_kernel, the 256x128 ring
                elif force == 5 and (nk < 4 or nk % 2 == 1 or nc % 256 != 0):
                    assert kernel == 1, (name, force, kernel)   # the stream kernel's rule excludes this launch: gemm_bf16_kernel
                elif force == 5:
                    assert kernel == 5, (name, force, kernel)   # gemm256ps_bf16_kernel, 256x256 stream per CU
                else:  # the launcher's own choice: its rule restated (encoder_kernel_reference.expected_kernel), and literals
                    assert kernel == ekr.expected_kernel(0, p["M"], nc, p["K"], clips, a_elems, p["N"] * p["K"]), (name, kernel)
                    assert kernel == AUTO_KERNEL.get((d, clips, name, n0), kernel), (name, kernel)
                swapped = (p["epi"] == ekr.EPI_QKV and n0 == 2 * d) or (p["epi"] == ekr.EPI_CROSS_KV and n0 == 0)
                _ran[dt].add((kernel, p["epi"], swapped))
            for o in outs:
                got = m.load(f"{name}.{force}.{o}", may_be_same=force != forces[0])
                if got is None:  # bit-identical to the first run of this case, which was checked
                    continue
                w = ekr.check(f"{dt} d {d} clips {clips} {family} {name} force {force} {o}", got, exp[o], dt)
                note(dt, f"gemm epilogue {p['epi']}", w)
                if p["epi"] == ekr.EPI_PARTIAL:
                    gpu_part = got[ekr.GUARD // 2:-(ekr.GUARD // 2)].view(np.float32)
        if fold is not None:  # LayerNorm alone: its reference folds the partials the GPU produced (checked just above)
            g, ks, ps, rows = ekr.GUARD // 2, p["ksplit"], p["part_stride"], clips * T
            xs, ys = m.load(f"{name}.fold.x"), m.load(f"{name}.fold.y")
            for a in (xs, ys):
                assert (a[:g] == ekr.SENT16).all() and (a[-g:] == ekr.SENT16).all(), f"{name}: the fold stored into a guard"
            parts = np.stack([gpu_part[q * ps:q * ps + rows * d].reshape(rows, d) for q in range(ks)])
            xr, xb, yr, yb = ekr.layernorm_expect(fold["x"], fold["g"], fold["b"], dt, parts, bufs["bias"])
            note(dt, "layernorm fold x", ekr.check_values(f"{name} fold x", xs[g:-g].view(np.float32).reshape(rows, d), xr, xb))
            note(dt, "layernorm fold y", ekr.check_values(f"{name} fold y", ekr.from_bits(ys[g:-g], dt).reshape(rows, d), yr, yb))
        del exp


@pytest.mark.parametrize("clips", (1, 2, 3))
@pytest.mark.parametrize("d", WIDTHS)
def test_gemm_launches_of_the_encoder(driver, tmp_path, d, clips):
    run_gemm_group(driver, tmp_path, d, clips, "uniform", gemm_cases(d, clips, "uniform"))


@pytest.mark.parametrize("d", WIDTHS)
def test_gemm_launches_realistic_statistics(driver, tmp_path, d):
    run_gemm_group(driver, tmp_path, d, 1, "realistic", gemm_cases(d, 1, "realistic"), seed0=7)


# per launch one clip count at d = 768 that gives the stream kernel 270 / 288 tiles of 256x256 (more than the 256 CUs and
# not a multiple) and the ring kernel >= 256 tiles of 256x128: conv1 3 x 12 x 8, Q,K 6 x 6 x 8, FFN1 and the cross K and V
# halves 12 x 6 x 4, the others 3 x 6 x 15
@pytest.mark.parametrize("clips, kinds", [(4, ("ffn1", "cross", "bias")), (8, ("conv1", "qk")), (15, ("conv2", "v", "oproj_resid", "ffn2_resid"))])
def test_gemm_more_tiles_than_cus(driver, tmp_path, clips, kinds):
    run_gemm_group(driver, tmp_path, 768, clips, "uniform", [(k, k, {}) for k in kinds], seed0=3)


def test_every_kernel_ran_every_epilogue(driver):
    dt, _ = driver
    want = {(k, e, s) for k in (1, 2, 5) for e, s in ((ekr.EPI_BIAS, False), (ekr.EPI_GELU, False), (ekr.EPI_GELU_POS, False),
                                                     (ekr.EPI_RESID, False), (ekr.EPI_QKV, False), (ekr.EPI_QKV, True),
                                                     (ekr.EPI_CROSS_KV, False), (ekr.EPI_CROSS_KV, True))} | {(1, ekr.EPI_PARTIAL, False)}
    assert want <= _ran[dt], sorted(want - _ran[dt])


# ------------------------------------------------------------------------------------------ LayerNorm
LN_ROWS = 1503  # not a multiple of the 4 rows of a workgroup


def layernorm_rows(rng, rows, d):
    """rows dealt over three families: N(0, 1); three outlier channels at |x| 150-500; constant (variance 0: eps decides)."""
    x = rng.standard_normal((rows, d)).astype(np.float32)
    ch = rng.choice(d, 3, replace=False)
    x[1::3, ch] += (rng.uniform(150, 500, 3) * rng.choice([-1, 1], 3)).astype(np.float32)
    x[2::3] = rng.choice([0.0, 0.5, -3.0, 1.7], (len(x[2::3]), 1)).astype(np.float32)
    return x


def test_layernorm(driver, tmp_path):
    dt, exe = driver
    m = Manifest(tmp_path)
    rng = np.random.default_rng(23)
    cases = []
    for d in (128, 384, 512, 768, 1024, 1280, 2048):
        for n_part in (0, 2, 3, 4):
            name = f"ln{d}.{n_part}"
            x = layernorm_rows(rng, LN_ROWS, d)
            g, b = rng.uniform(0.5, 1.5, d).astype(np.float32), rng.uniform(-1, 1, d).astype(np.float32)
            ps = (LN_ROWS + 5) * d
            part = rng.standard_normal((max(n_part, 1), ps)).astype(np.float32)
            pb = rng.uniform(-1, 1, d).astype(np.float32)
            m.alloc("x", x); m.alloc("g", g); m.alloc("b", b); m.alloc("y", ekr.sentinel(LN_ROWS * d, 2)); m.alloc("part", part); m.alloc("pb", pb)
            m.add(f"ln {name} x=x g=g b=b y=y rows={LN_ROWS} d={d} part=part n_part={n_part} part_stride={ps} part_bias=pb")
            m.dump("x", name + ".x"); m.dump("y", name + ".y")
            for bn in ("x", "g", "b", "y", "part", "pb"):
                m.add(f"free {bn}")
            cases.append((name, d, n_part, x, g, b, part[:n_part, :LN_ROWS * d].reshape(n_part, LN_ROWS, d) if n_part else None, pb if n_part else None))
    m.run(exe, timeout=300)
    gd = ekr.GUARD // 2
    for name, d, n_part, x, g, b, part, pb in cases:
        xs, ys = m.load(name + ".x"), m.load(name + ".y")
        for a in (xs, ys):
            assert (a[:gd] == ekr.SENT16).all() and (a[-gd:] == ekr.SENT16).all(), f"{name}: store into a guard"
        xr, xb, yr, yb = ekr.layernorm_expect(x, g, b, dt, part, pb)
        w = ekr.check_values(name + " y", ekr.from_bits(ys[gd:-gd], dt).reshape(LN_ROWS, d), yr, yb)
        if n_part:
            w = max(w, ekr.check_values(name + " x", xs[gd:-gd].view(np.float32).reshape(LN_ROWS, d), xr, xb))
        else:
            assert np.array_equal(xs[gd:-gd], x.view(np.uint16).ravel()), f"{name}: x written without partials"
        print(f"{dt} {name}: worst error / bound {w:.3f}")
        note(dt, "layernorm", w)


# ------------------------------------------------------------------------------------------ attention
THRS = (0.0, 0.5, 8.0, 16.0)
ATTN_SHAPES = [(1500, 2, 1), (1500, 2, 3), (1500, 6, 1), (1500, 6, 3), (1500, 20, 1), (1500, 20, 3)] + \
              [(t, 3, 3) for t in (4, 64, 128, 132, 1472, 1476)]  # heads x clips odd: the XCD remap sees a grid that is no multiple of 8


@pytest.mark.parametrize("T_, heads, clips", ATTN_SHAPES)
def test_attention(driver, tmp_path, T_, heads, clips):
    dt, exe = driver
    m = Manifest(tmp_path)
    rng = np.random.default_rng(T_ * 100 + heads * 10 + clips)
    d, t_pad = heads * 64, (T_ + 63) // 64 * 64
    q, k, v = (np.zeros((clips, T_, heads, 64), np.float32) for _ in range(3))
    fam = {}
    for c in range(clips):
        for h in range(heads):
            fam[c, h] = ekr.ATTN_FAMILIES[(c * heads + h + T_ + heads) % len(ekr.ATTN_FAMILIES)]
            q[c, :, h], k[c, :, h], v[c, :, h] = ekr.attention_inputs(rng, T_, dt, fam[c, h])
    vt = {}
    for pad in ("zero", "garbage"):  # V^T [clip][head][64][t_pad] in the stored frame order; frames >= T: zeros, or finite garbage
        nat = np.zeros((clips, heads, 64, t_pad), np.float32) if pad == "zero" else rng.uniform(-4, 4, (clips, heads, 64, t_pad)).astype(np.float32)
        nat[..., :T_] = v.transpose(0, 2, 3, 1)
        stored = np.empty_like(nat)
        stored[..., ekr.vt_perm(np.arange(t_pad))] = nat
        vt[pad] = ekr.to_bits(stored, dt)
    m.alloc("q", ekr.to_bits(q, dt)); m.alloc("k", ekr.to_bits(k, dt)); m.alloc("o", ekr.sentinel(clips * T_ * d, 2))
    m.alloc("vt_zero", vt["zero"]); m.alloc("vt_garbage", vt["garbage"])
    for thr in THRS:
        for pad in ("zero", "garbage"):
            m.add("reset o")
            m.add(f"attn a{thr}{pad} q=q k=k vt=vt_{pad} o=o batch={clips} T={T_} t_pad={t_pad} d={d} heads={heads} thr={thr}")
            m.dump("o", f"o.{thr}.{pad}")
    m.run(exe, timeout=300)
    refs = {ch: ekr.attention_expect(q[ch[0], :, ch[1]].astype(np.float64), k[ch[0], :, ch[1]].astype(np.float64),
                                     v[ch[0], :, ch[1]].astype(np.float64), dt, t_pad) for ch in fam}
    gd = ekr.GUARD // 2
    for thr in THRS:
        oz, og = m.load(f"o.{thr}.zero"), m.load(f"o.{thr}.garbage")
        assert (oz[:gd] == ekr.SENT16).all() and (oz[-gd:] == ekr.SENT16).all(), "store into a guard"
        assert np.array_equal(oz, og), f"thr {thr}: finite garbage in the padded V^T frames changed the result"
        o = ekr.from_bits(oz[gd:-gd], dt).reshape(clips, T_, heads, 64)
        for (c, h), (ref, bound) in refs.items():
            w = ekr.check_values(f"{dt} T {T_} heads {heads} clip {c} head {h} {fam[c, h]} thr {thr}", o[c, :, h], ref, bound)
            note(dt, f"attention {fam[c, h]}", w)


def test_zz_report(driver):
    dt, _ = driver
    for (t, what), w in sorted(_worst.items()):
        if t == dt:
            print(f"{dt} {what}: worst error / bound {w:.3f}")
    print(f"wall time so far {time.time() - _state['t0']:.0f} s")
