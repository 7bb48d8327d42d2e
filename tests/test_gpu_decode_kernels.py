"""GPU: every kernel of the batched decoder step (3 or more clips) alone, its WHOLE output against float64, both builds.

tests/cpp/decode_kernels_driver.cpp is linked against the objects `make` produced for libax_whisper.so (build/decode_gemm.*.o,
build/decoder.*.o), so what runs here is the shipped code. Each case is one launch — launch_decode_cgemm, launch_decode_gemm
(rt = 0 included), launch_act_prep, launch_decode_attention, launch_pack_weight_frag(_split) — or the two or three launches of one
hand-off (split-K partials -> act_prep; the query fold's QKV launch -> o launch -> decode_attention_kernel<2>; an attention launch
repeated without a reset), with strides and offsets as Engine's step builders (csrc/engine_decode.cpp) set them. Every output buffer
comes back whole with its guards; everything a launch must not write (cache rows other than off[b], clips >= batch of a clip
block, rows >= N, other slices' partial slabs, records of finished clips, the guards) holds a NaN sentinel before and the same
bits after. tests/decode_kernel_reference.py holds the references, the index maps and the bounds (derived in its docstring);
tests/test_decode_kernel_reference.py shows without a GPU that a float32 emulation stays inside them and sixteen seeded defects do
not. test_every_decode_kernel_ran_every_form counts launcher x epilogue / query mode x instantiation per build.

A driver process has its own timeout; after one that fails, nothing further is launched and the remaining cases fail at once.

NOT YET MEASURED ON MI355X: no GPU run could be obtained while this file was written, so the worst error / bound per launcher,
epilogue and build (printed by -s and by test_zz_report), the file's wall time, the kappa finding and the fp16 fold headroom are
still to be filled in here and in DESIGN.md. What is known without a GPU: the driver compiles and links for both builds, and the
whole file passes when the driver process is replaced by the float32 emulations of tests/test_decode_kernel_reference.py (138
tests; the modelgen-like residual family gives |g . x0| <= 257, a headroom of 255 x to half's 65504).
"""
import time

import numpy as np
import pytest

import decode_kernel_reference as R
import kernel_driver

pytestmark = pytest.mark.gpu

DTYPES = kernel_driver.DTYPES

_session = kernel_driver.Session()
_ran, _worst, _state = _session.ran, _session.worst, _session.state
_facts = {}


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, kernel_driver.driver_exe(request.param)


def form_of(cmd, p, qall=None):
    """What a launch exercises: launcher, epilogue / query mode, template instantiation."""
    if cmd == "cgemm":
        ch = (p["K"] // 32 + 7) // 8 if p.get("ln_w") else 0
        inp = ("foldln" if p.get("fold_row0") else "ln") if p.get("ln_w") else ("foldpair" if p.get("fold_row0") else "pair")
        return ("cgemm", p["epilogue"], inp, max(ch, 2) if ch else 0, p["rt"])
    if cmd == "dgemm":
        nb = (p["batch"] + 15) // 16
        return ("logits0", nb, (p["K"] // 32 + 7) // 8) if p["rt"] == 0 else ("dgemm", p["epilogue"], p["rt"], nb)
    if cmd == "actprep":
        return ("actprep", p["do_ln"], p["n_part"])
    if cmd == "attn":
        mode = "fold" if p.get("tq") else "fused" if p.get("wq") else "q"
        inst = p["d_model"] // 32 if mode == "fused" and p["d_model"] in (384, 512, 768, 1024) and qall != "0" else 0
        out = ("pair1" if p.get("n_split", 1) == 1 else "pairN") if p.get("out_hi") else "part"
        return ("attn", mode, inst, out, "self" if p["n_keys"] < 0 else "cross")
    return (cmd,)


def grid_of(cmd, p):
    if cmd == "cgemm":
        return (p["N"] + 16 * p["rt"] - 1) // (16 * p["rt"]), (p["batch"] + 15) // 16, 1
    if cmd == "dgemm":
        return R.dgemm_grid(p["N"], p["rt"]), p["ksplit"] if p["epilogue"] == R.GEPI_PARTIAL else 1, 1
    if cmd == "actprep":
        return p["batch"], 1, 1
    if cmd == "attn":
        return p.get("n_split", 1), p["n_head"], p["batch"]
    return 2048, 1, 1


def run_groups(driver, tmp_path, groups, timeout=120, qall=None, keep=None):
    return kernel_driver.run_groups(_session, R.verify, form_of, grid_of, driver, tmp_path, groups, timeout=timeout, qall=qall, keep=keep)


OFFS8 = (0, 7, 63, 64, 65, 127, 128, 447)
G = R.linear_group


# ------------------------------------------------------------------------------------------ launch_decode_cgemm
@pytest.mark.parametrize("K", (128, 384, 512, 768, 1024, 1280))
def test_cgemm_layernorm_prologue(driver, tmp_path, K):
    """Every CH instantiation (K 128 and 384 share CH = 2), rt 1 and 2 (N no multiple of 32), batches 1 .. 40 with nbs above the
    blocks in use, the three row families and the two shifted ones dealt over the clips of every launch, and modelgen's stream."""
    dt = driver[0]
    groups = [G(dt, K + 1, "cgemm", K=K, N=40, batch=17, nbs=3, epi=R.GEPI_STORE, ln=True),
              G(dt, K + 2, "cgemm", K=K, N=72, batch=15, nbs=2, epi=R.GEPI_STORE, rt=2, ln=True),
              G(dt, K + 3, "cgemm", K=K, N=100, batch=40, nbs=4, epi=R.GEPI_GELU, rt=2, ln=True),
              G(dt, K + 4, "cgemm", K=K, N=24, batch=16, nbs=2, epi=R.GEPI_GELU, ln=True, family="realistic"),
              G(dt, K + 5, "cgemm", K=K, N=40, batch=1, nbs=1, epi=R.GEPI_STORE, ln=True, family="realistic")]
    keep = {}
    run_groups(driver, tmp_path, groups, keep=keep)
    # the kappa finding: per row family of the first launch, the worst error / bound and the worst error relative to the row's largest output
    bufs, ls = groups[0]
    _, ident, p, _ = ls[0]
    exp, _, info = R.gemm_expect(p, bufs, dt)
    e = exp[p["out"]]
    got = R.strip(ident, keep[ident][p["out"]]).view(np.float32)[:17 * 40].astype(np.float64).reshape(17, 40)
    ref, bound = e.ref[:17 * 40].reshape(17, 40), e.bound[:17 * 40].reshape(17, 40)
    for c in range(17):
        fam = R.LN_FAMILIES[c % len(R.LN_FAMILIES)]
        err = np.abs(got[c] - ref[c])
        old = _facts.setdefault((dt, "ln family"), {}).get(fam, (0.0, 0.0, 0.0))
        _facts[dt, "ln family"][fam] = (max(old[0], float(info["kappa"][c])), max(old[1], float((err / bound[c]).max())), max(old[2], float(err.max() / np.abs(ref[c]).max())))


@pytest.mark.parametrize("K", (128, 768, 3072, 5120))
def test_cgemm_pair_input(driver, tmp_path, K):
    """K = 128: fewer k-steps than waves; 5120: two trips of the depth-8 loop. RESID runs in place onto a non-zero out."""
    dt = driver[0]
    run_groups(driver, tmp_path, [G(dt, K + 1, "cgemm", K=K, N=48, batch=16, nbs=2, epi=R.GEPI_RESID),
                                  G(dt, K + 2, "cgemm", K=K, N=40, batch=17, nbs=3, epi=R.GEPI_RESID, family="realistic"),
                                  G(dt, K + 3, "cgemm", K=K, N=72, batch=40, nbs=4, epi=R.GEPI_RESID, rt=2),
                                  G(dt, K + 4, "cgemm", K=K, N=24, batch=1, nbs=1, epi=R.GEPI_STORE),
                                  G(dt, K + 5, "cgemm", K=K, N=72, batch=15, nbs=1, epi=R.GEPI_STORE, rt=2),
                                  G(dt, K + 6, "cgemm", K=K, N=100, batch=17, nbs=2, epi=R.GEPI_GELU),
                                  G(dt, K + 7, "cgemm", K=K, N=40, batch=15, nbs=2, epi=R.GEPI_GELU, rt=2, family="realistic")])


@pytest.mark.parametrize("rt", (1, 2))
def test_cgemm_qkv_cache_rows(driver, tmp_path, rt):
    """d_model 384, eight clips at eight different cache rows, a clip stride with slack: only row off[b] of clip b's own cache."""
    dt = driver[0]
    rng = np.random.default_rng(rt)
    run_groups(driver, tmp_path, [G(dt, 10 + rt, "cgemm", K=384, N=1152, batch=8, nbs=1, epi=R.GEPI_QKV_CACHE, rt=rt, ln=True, d_model=384, offs=OFFS8),
                                  G(dt, 20 + rt, "cgemm", K=384, N=1152, batch=8, nbs=2, epi=R.GEPI_QKV_CACHE, rt=rt, ln=True, d_model=384,
                                    offs=rng.permutation(OFFS8), family="realistic"),
                                  G(dt, 30 + rt, "cgemm", K=384, N=1152, batch=8, nbs=1, epi=R.GEPI_QKV_CACHE, rt=rt, d_model=384, offs=OFFS8[::-1])])


@pytest.mark.parametrize("batch", (4, 20))
@pytest.mark.parametrize("d", (384, 768))
def test_cgemm_query_fold_hand_off(driver, tmp_path, d, batch):
    """QKV launch (rows [3d, 4d) against ln_w2 . x) -> o launch (W_lo, out2 accumulation, stat_part) -> decode_attention_kernel<2>,
    on modelgen's residual family (in the half build too: finite and within bound) and on the benign one."""
    dt = driver[0]
    groups = [R.fold_group(dt, d + batch, d=d, batch=batch, nbs=(batch + 15) // 16 + 1, n_split=6 if batch == 4 else 1, family="realistic"),
              R.fold_group(dt, d + batch + 1, d=d, batch=batch, nbs=(batch + 15) // 16, n_split=3 if batch == 4 else 2, n_keys=200, family="benign")]
    run_groups(driver, tmp_path, groups, timeout=180)
    bufs, ls = groups[0]
    x, g2 = R.typed(ls[0][2], bufs)["x"][:batch * d].reshape(batch, d), bufs["ln_w2"]
    _facts.setdefault((dt, "fold |g x0|"), []).append(float(np.abs(x * g2).max()))


# ------------------------------------------------------------------------------------------ launch_decode_gemm
DGEMM = [(1, 3, 1280, R.GEPI_STORE, 40), (4, 16, 1280, R.GEPI_STORE, 100), (1, 17, 5120, R.GEPI_RESID, 24), (4, 48, 1280, R.GEPI_RESID, 72),
         (1, 64, 1280, R.GEPI_GELU, 40), (4, 17, 5120, R.GEPI_GELU, 100), (1, 48, 5120, R.GEPI_STORE, 24), (4, 64, 5120, R.GEPI_RESID, 72),
         (4, 3, 1280, R.GEPI_GELU, 100), (1, 16, 5120, R.GEPI_GELU, 40)]


@pytest.mark.parametrize("half", (0, 1))
def test_dgemm_epilogues(driver, tmp_path, half):
    """rt 1 and 4, NB 1 - 4, K 1280 and 5120, N with a ragged last row tile; QKV_CACHE with per-clip rows."""
    dt = driver[0]
    rng = np.random.default_rng(half)
    groups = [G(dt, 100 + i, "dgemm", K=K, N=N, batch=b, nbs=(b + 15) // 16 + (i % 2), epi=epi, rt=rt, family="realistic" if i % 3 == 0 else "benign")
              for i, (rt, b, K, epi, N) in enumerate(DGEMM) if i % 2 == half]
    b = (17, 64)[half]
    groups.append(G(dt, 120 + half, "dgemm", K=1280, N=1152, batch=b, nbs=(b + 15) // 16, epi=R.GEPI_QKV_CACHE, rt=(1, 4)[half], d_model=384,
                    offs=rng.permutation(448)[:b]))
    groups.append(G(dt, 122 + half, "dgemm", K=1280, N=1152, batch=8, nbs=1, epi=R.GEPI_QKV_CACHE, rt=(4, 1)[half], d_model=384, offs=OFFS8))
    run_groups(driver, tmp_path, groups, timeout=180)


@pytest.mark.parametrize("K, batch", [(384, 17), (512, 3), (768, 16), (1280, 48), (5120, 64), (1280, 3)])
def test_dgemm_split_k_partials_and_their_fold(driver, tmp_path, K, batch):
    """The slice counts ksplit_for gives (1, 2, 3, 4), other slices' slabs and clips >= batch of a slab untouched, then the
    launch_act_prep that folds what the GPU wrote."""
    run_groups(driver, tmp_path, [R.partial_group(driver[0], K + batch, K=K, d=384, batch=batch, nbs=(batch + 15) // 16 + 1)])


@pytest.mark.parametrize("rt, batch, K", [(1, 16, 1280), (4, 64, 1280), (4, 17, 5120), (1, 48, 1280)])
def test_dgemm_logits_and_argmax_ties(driver, tmp_path, rt, batch, K):
    dt = driver[0]
    nbs = (batch + 15) // 16
    run_groups(driver, tmp_path, [R.logits_group(dt, rt + batch, K=K, N=300, batch=batch, nbs=nbs, rt=rt),
                                  R.logits_group(dt, rt + batch + 1, K=K, N=300, batch=batch, nbs=nbs + 1, rt=rt, dump=False),
                                  R.logits_group(dt, rt + batch + 2, K=K, N=83, batch=batch, nbs=nbs, rt=rt, offs=np.arange(batch) % 3, skip=3),
                                  R.logits_group(dt, rt + batch + 3, K=K, N=83, batch=batch, nbs=nbs, rt=rt, offs=np.arange(batch) % 4, skip=3)])


# ------------------------------------------------------------------------------------------ rt = 0: the resident vocabulary projection
@pytest.mark.parametrize("K", (128, 384, 768, 1024, 1280))
def test_logits_resident_every_instantiation(driver, tmp_path, K):
    dt = driver[0]
    batches = [b for b in (16, 17, 32, 48, 64) if R.logits_resident_ok(K, b)]
    assert len(batches) >= 4
    groups = [R.logits_group(dt, K + b, K=K, N=16 * 5 + 3, batch=b, nbs=(b + 15) // 16 + (b == 17), rt=0) for b in batches]
    groups.append(R.logits_group(dt, K, K=K, N=83, batch=16, nbs=1, rt=0, offs=np.arange(16) % 3, skip=3))   # all below: nothing written
    groups.append(R.logits_group(dt, K + 1, K=K, N=83, batch=17, nbs=2, rt=0, offs=np.arange(17) // 16 * 3, skip=3))  # one clip at the threshold
    run_groups(driver, tmp_path, groups)


@pytest.mark.parametrize("n_rb", (1, 255, 256, 257, 512, 513, 768, 769))
def test_logits_resident_row_block_counts(driver, tmp_path, n_rb):
    """The triple-buffered loop (rb += 3 G, G = min(n_rb, 256)) at every count of trips and early breaks; ties across iterations
    of one workgroup and across the 16 row lanes."""
    dt = driver[0]
    run_groups(driver, tmp_path, [R.logits_group(dt, n_rb, K=128, N=n_rb * 16 - 5, batch=16 + n_rb % 2, nbs=2, rt=0)])


def test_logits_resident_real_vocabulary(driver, tmp_path):
    run_groups(driver, tmp_path, [R.logits_group(driver[0], 51865, K=384, N=51865, batch=17, nbs=2, rt=0, family="realistic")], timeout=180)


# ------------------------------------------------------------------------------------------ launch_act_prep
@pytest.mark.parametrize("K", (384, 1280, 2048))
def test_act_prep(driver, tmp_path, K):
    """n_part 0 - 4, LayerNorm on and off, 1 / 17 / 64 clips, part_batch > batch; x is rewritten exactly when n_part > 0."""
    groups = []
    for i, (n_part, do_ln) in enumerate((n, l) for n in range(5) for l in (1, 0)):
        batch = (1, 17, 64)[(i + K // 128) % 3]
        b = {}
        groups.append((b, [R.actprep_launch(np.random.default_rng(K + i), b, K=K, batch=batch, nbs=(batch + 15) // 16 + i % 2, n_part=n_part,
                                            do_ln=do_ln, part_batch=batch + 5)]))
    run_groups(driver, tmp_path, groups)


# ------------------------------------------------------------------------------------------ launch_decode_attention
SELF_OFFS = (0, 62, 63, 64, 127, 128, 255, 256, 447)


def test_attention_self(driver, tmp_path):
    """n_keys = -1, cap_blocks 7, nine clips at nine positions; the pair output and the partial records at 1 and 2 splits (the
    second split of a clip below 256 keys holds none: m = -inf, l = 0)."""
    dt = driver[0]
    run_groups(driver, tmp_path, [R.attn_group(dt, 1, cap=7, offs=SELF_OFFS, batch=9),
                                  R.attn_group(dt, 2, cap=7, offs=SELF_OFFS[::-1], batch=9, out="part"),
                                  R.attn_group(dt, 3, cap=7, offs=SELF_OFFS, batch=9, n_split=2, out="part"),
                                  R.attn_group(dt, 4, H=5, cap=7, offs=(447, 0, 64), batch=3, done_late=1)])


@pytest.mark.parametrize("n_keys", (1, 64, 65, 1472, 1476, 1500))
def test_attention_cross(driver, tmp_path, n_keys):
    """cap_blocks 24; the pair at one split and folded through mpart / mcnt at 2, 3, 4, 6 (mcnt zero afterwards, a second launch
    without a reset gives the same bits); partial records at 1, 2, 3, 8 splits; garbage beyond n_keys changes no bit."""
    dt = driver[0]
    groups = [R.attn_group(dt, n_keys, cap=24, n_keys=n_keys)]
    groups += [R.attn_group(dt, n_keys + s, cap=24, n_keys=n_keys, n_split=s, relaunch=True, batch=3 + s % 2) for s in (2, 3, 4, 6)]
    groups += [R.attn_group(dt, n_keys + 10 + s, cap=24, n_keys=n_keys, n_split=s, out="part", garbage_too=s == 8) for s in (1, 2, 3, 8)]
    run_groups(driver, tmp_path, groups, timeout=180)


@pytest.mark.parametrize("done_late", (0, 1))
def test_attention_done_flags(driver, tmp_path, done_late):
    """A finished clip's outputs, records and counters keep their sentinel or zero, with the early and the late look at the flag."""
    dt = driver[0]
    run_groups(driver, tmp_path, [R.attn_group(dt, 5, cap=24, n_keys=65, n_split=2, done=(0, 1, 0, 1), batch=4, done_late=done_late, relaunch=True),
                                  R.attn_group(dt, 6, cap=7, offs=(5, 70, 300), done=(1, 0, 0), done_late=done_late),
                                  R.attn_group(dt, 7, cap=24, n_keys=1500, n_split=3, out="part", done=(0, 0, 1), done_late=done_late),
                                  R.attn_group(dt, 8, H=6, cap=24, n_keys=64, mode="fused", done=(0, 1, 0), done_late=done_late),
                                  R.attn_group(dt, 9, H=6, cap=24, n_keys=64, mode="fused", n_split=2, done=(1, 1, 1), done_late=done_late)])


@pytest.mark.parametrize("qall", (None, "0"))
@pytest.mark.parametrize("d", (384, 512, 768, 1024, 640))
def test_attention_fused_query(driver, tmp_path, d, qall):
    """The up-front instantiations (d_model 384 / 512 / 768 / 1024), the generic one (640), and all of them generic under
    AX_WHISPER_ATTN_QALL=0 (read once per process: a driver process of its own); five clips so that every LayerNorm row family is
    in, and modelgen's stream; against float64 LayerNorm plus projection."""
    dt = driver[0]
    run_groups(driver, tmp_path, [R.attn_group(dt, d, H=d // 64, batch=5, cap=24, n_keys=65, mode="fused"),
                                  R.attn_group(dt, d + 1, H=d // 64, batch=3, cap=24, n_keys=1500, mode="fused", n_split=6, relaunch=True),
                                  R.attn_group(dt, d + 2, H=d // 64, batch=5, cap=24, n_keys=200, mode="fused", n_split=2, garbage_too=False)],
               timeout=180, qall=qall)


# ------------------------------------------------------------------------------------------ the packing kernels
@pytest.mark.parametrize("N, K", [(37, 96), (1152, 384), (16, 32)])
def test_weight_packing(driver, tmp_path, N, K):
    """Bit-exact against the numpy index map, tail rows of the last block zero; the split form hi == h16(w), lo == h16(w - hi)."""
    run_groups(driver, tmp_path, R.pack_groups(driver[0], N + K, N, K))


# ------------------------------------------------------------------------------------------ coverage and report
def test_every_decode_kernel_ran_every_form(driver):
    dt, _ = driver
    E = R
    want = set()
    want |= {("cgemm", e, "ln", ch, rt) for e in (E.GEPI_STORE, E.GEPI_GELU) for ch in (2, 3, 4, 5) for rt in (1, 2)}
    want |= {("cgemm", e, "pair", 0, rt) for e in (E.GEPI_STORE, E.GEPI_GELU, E.GEPI_RESID) for rt in (1, 2)}
    want |= {("cgemm", E.GEPI_QKV_CACHE, "ln", 2, rt) for rt in (1, 2)} | {("cgemm", E.GEPI_QKV_CACHE, "pair", 0, rt) for rt in (1, 2)}
    want |= {("cgemm", E.GEPI_QKV_CACHE, "foldln", 2, 1), ("cgemm", E.GEPI_QKV_CACHE, "foldln", 3, 1), ("cgemm", E.GEPI_RESID, "foldpair", 0, 1)}
    want |= {("dgemm", e, rt, nb) for e in (E.GEPI_STORE, E.GEPI_GELU, E.GEPI_RESID, E.GEPI_QKV_CACHE, E.GEPI_LOGITS) for rt in (1, 4) for nb in (1, 2, 3, 4)
             if (e, rt, nb) in {(E.GEPI_STORE, 1, 1), (E.GEPI_STORE, 4, 1), (E.GEPI_STORE, 1, 3), (E.GEPI_RESID, 1, 2), (E.GEPI_RESID, 4, 3),
                                (E.GEPI_RESID, 4, 4), (E.GEPI_GELU, 1, 4), (E.GEPI_GELU, 4, 2), (E.GEPI_GELU, 4, 1), (E.GEPI_GELU, 1, 1),
                                (E.GEPI_QKV_CACHE, 1, 2), (E.GEPI_QKV_CACHE, 4, 4), (E.GEPI_QKV_CACHE, 4, 1), (E.GEPI_QKV_CACHE, 1, 1),
                                (E.GEPI_LOGITS, 1, 1), (E.GEPI_LOGITS, 4, 4), (E.GEPI_LOGITS, 4, 2), (E.GEPI_LOGITS, 1, 3)}}
    want |= {("dgemm", E.GEPI_PARTIAL, 1, nb) for nb in (1, 2, 3, 4)}
    want |= {("logits0", nb, ch) for ch in (1, 2, 3) for nb in (1, 2, 3, 4)} | {("logits0", nb, ch) for ch in (4, 5) for nb in (1, 2, 3)}
    want |= {("actprep", ln, n) for ln in (0, 1) for n in range(5)}
    want |= {("attn", "q", 0, out, "self") for out in ("pair1", "part")} | {("attn", "q", 0, out, "cross") for out in ("pair1", "pairN", "part")}
    want |= {("attn", "fused", inst, out, "cross") for inst in (12, 16, 24, 32, 0) for out in ("pair1", "pairN")}
    want |= {("attn", "fold", 0, "pair1", "cross"), ("attn", "fold", 0, "pairN", "cross"), ("packw",), ("packw_split",)}
    assert want <= _ran[dt], sorted(want - _ran[dt], key=str)


def test_zz_report(driver):
    dt, _ = driver
    for (t, what), w in sorted(_worst.items()):
        if t == dt:
            print(f"{dt} {what}: worst error / bound {w:.3f}")
    for fam, (kappa, ratio, rel) in sorted(_facts.get((dt, "ln family"), {}).items()):
        print(f"{dt} LayerNorm prologue, {fam} rows (E[x^2] / var up to {kappa:.1f}): worst error / bound {ratio:.3f}, worst error / largest output of the row {rel:.2e}")
    if (dt, "fold |g x0|") in _facts:
        m = max(_facts[dt, "fold |g x0|"])
        print(f"{dt} query fold: largest |g . x0| of the realistic residual family {m:.1f}, headroom to 65504: {65504 / m:.0f} x")
    print(f"wall time so far {time.time() - _state['t0']:.0f} s")
