"""GPU: the GEMV decode family (gemv1_kernel, gemv_kernel: csrc/decode_gemv.hip), advance_kernel and embed_kernel alone, their WHOLE
output against float64, both builds.

tests/cpp/decode_kernels_driver.cpp is linked against the objects `make` produced for libax_whisper.so (build/decode_gemv.*.o,
build/decoder.*.o), so what runs here is the shipped code. A case is a list of groups, a group one launch_gemv / launch_advance /
launch_embed (or two launch_advance on the same buffers) with strides and offsets as Engine::enqueue_decode_step sets them. Every
buffer a launch names, inputs included, comes back whole with its guards: what the launch must write is compared with the float64
reference inside the derived bound (tests/gemv_kernel_reference.py; advance and embed bit for bit), everything else — out rows
>= N and clips >= batch, cache rows other than off[b] of the clip's own slab, amax slots >= grid, the dump beyond N, every per-clip
array beyond batch, the partials — holds a NaN sentinel before and the same bits after. tests/test_decode_kernel_reference.py shows
without a GPU that float32 emulations pass every case of CASES below and eighteen seeded defects do not.

The generators of this suite (ln_rows aside) and tools/modelgen.py draw their outlier channels from arange(1, d): family `outlier0`
is the realistic stream with its larger outlier exchanged into channel 0, where the prologues used to take the shift of a one-pass
variance. It meets the same two-pass bound as every other family since both prologues take the squares of centred values.

A driver process has its own timeout; after one that fails, nothing further is launched and the remaining cases fail at once.

NOT YET MEASURED ON MI355X: no GPU run could be obtained while this file was written (the pool had no free machine), so the worst
error / bound per launcher, prologue, epilogue and build (printed by -s and by test_zz_report) and the file's wall time are still to
be filled in here and in DESIGN.md, as are the step times of the launch-per-phase path before and after the prologue change. What
is known without a GPU: the driver compiles and links for both builds against the shipped objects; decode_gemv.hip compiles with
no scratch and its SGPR spills within 48 (tests/test_kernel_resources.py); the whole file, the form count included, passes when the
driver process is replaced by the float32 emulations of tests/test_decode_kernel_reference.py (worst error / bound, bf16 | fp16: K / V cache rows
0.945 | 0.745 — the 16-bit rounding —, LayerNorm identity rows 0.036 | 0.036, every other fp32 output below 0.02); and the emulation of the prologues' former arithmetic fails the `outlier0` cases,
and only those, at K 384, 768 and 1280 in both builds (emulated, not observed on the device).
"""
import time

import pytest

import gemv_kernel_reference as G
import kernel_driver
from decode_kernel_reference import GEPI_GELU, GEPI_LOGITS, GEPI_QKV_CACHE, GEPI_RESID, GEPI_STORE
from gemv_kernel_reference import PRO_ATTN_COMBINE as CMB
from gemv_kernel_reference import PRO_LAYERNORM as LN
from gemv_kernel_reference import PRO_PLAIN as PLAIN

pytestmark = pytest.mark.gpu

DTYPES = kernel_driver.DTYPES
_session = kernel_driver.Session()

# K -> (LPR, CH): every instantiation the Whisper sizes reach, and K = 256 for CH = 1
KS = {256: (32, 1), 384: (16, 3), 512: (32, 2), 768: (32, 3), 1024: (64, 2), 1280: (32, 5), 1536: (64, 3), 2048: (64, 4), 3072: (64, 6),
      4096: (64, 8), 5120: (64, 10)}
# the smallest N with two passes per workgroup and ONE valid row in the last pass of the last workgroup, per LPR
MULTIPASS = {64: (1024, 8197), 32: (512, 16393), 16: (384, 32785)}
g = G.gemv_group


def inst_case(K):
    """One K: N = two row passes' worth plus three (one pass per workgroup, a ragged last workgroup); gemv1_kernel under LayerNorm and
    the plain prologue, gemv_kernel<.., 1> under the attention combine, gemv_kernel<.., 4> with 2, 3 and 4 clips (masked clips)."""
    def make(dt):
        N = 2 * (256 // KS[K][0]) + 3
        pro2 = LN if K <= 2048 else PLAIN  # the LDS prologue holds K <= 2048 in registers (d_model <= 1280 in the engine)
        gs = [g(dt, K + 1, K=K, N=N, batch=1, pro=LN, epi=GEPI_STORE, ln_shift=K // 128),
              g(dt, K + 2, K=K, N=N, batch=1, pro=PLAIN, epi=GEPI_RESID, family="realistic"),
              g(dt, K + 3, K=K, N=N, batch=1, pro=CMB, epi=GEPI_STORE, n_split=2),
              g(dt, K + 4, K=K, N=N, batch=2, pro=pro2, epi=GEPI_GELU, ln_shift=K // 128 + 1),
              g(dt, K + 5, K=K, N=N, batch=3, pro=PLAIN, epi=GEPI_STORE),
              g(dt, K + 6, K=K, N=N, batch=4, pro=CMB, epi=GEPI_RESID, n_split=3)]
        if K <= 2048:
            gs.append(g(dt, K + 7, K=K, N=N, batch=4, pro=LN, epi=GEPI_STORE, ln_shift=K // 128 + 2))
        return gs
    return make


def qkv_case(d):
    """LN -> QKV_CACHE: different offsets in one launch, a K row on both sides of a 64-key block edge, the first and the last row."""
    return lambda dt: [g(dt, d + 1, K=d, N=3 * d, batch=4, pro=LN, epi=GEPI_QKV_CACHE, d_model=d, offs=(0, 63, 64, 447)),
                       g(dt, d + 2, K=d, N=3 * d, batch=1, pro=LN, epi=GEPI_QKV_CACHE, d_model=d, offs=(64,), family="realistic"),
                       g(dt, d + 3, K=d, N=3 * d, batch=2, pro=LN, epi=GEPI_QKV_CACHE, d_model=d, offs=(447, 63), family="realistic"),
                       g(dt, d + 4, K=d, N=3 * d, batch=3, pro=LN, epi=GEPI_QKV_CACHE, d_model=d, offs=(64, 0, 65))]


def combine_case(n_split):
    """COMBINE -> RESID over the score families; with 3 and 8 splits one split holds no key."""
    empty = None if n_split == 1 else 1
    return lambda dt: [g(dt, 10 * n_split + b, K=384, N=384, batch=b, pro=CMB, epi=GEPI_RESID, n_split=n_split, empty=empty) for b in (1, 2, 4)]


def multipass_case(lpr, epi):
    K, N = MULTIPASS[lpr]
    if epi == GEPI_LOGITS:  # planted exact ties: inside a workgroup, across waves, passes and workgroups, and the last row
        return lambda dt: [g(dt, lpr + 1, K=K, N=N, batch=1, pro=LN, epi=epi, ties=True),
                           g(dt, lpr + 2, K=K, N=N, batch=3, pro=LN, epi=epi, ties=True, family="realistic")]
    if epi == GEPI_RESID:   # the `first ? resid0 : out` path and the per-pass bias
        return lambda dt: [g(dt, lpr + 3, K=K, N=N, batch=1, pro=PLAIN, epi=epi), g(dt, lpr + 4, K=K, N=N, batch=2, pro=PLAIN, epi=epi, family="realistic")]
    return lambda dt: [g(dt, lpr + 5, K=K, N=N, batch=1, pro=LN, epi=epi), g(dt, lpr + 6, K=K, N=N, batch=4, pro=LN, epi=epi, family="realistic")]


def skip_case(dt):
    """skip_before_step 3: every clip below it -> nothing at all is written; one clip of four at it -> all four clips' partials."""
    gs = []
    for i, (offs, dump) in enumerate((o, d) for o in ((0, 1, 2, 2), (2, 0, 3, 1), (2,), (3,)) for d in (True, False)):
        gs.append(g(dt, 40 + i, K=384, N=83, batch=len(offs), pro=LN, epi=GEPI_LOGITS, offs=offs, skip=3, dump=dump))
    return gs


def ln_case(K, family):
    """Every LayerNorm row family through gemv1_kernel (one clip each) and gemv_kernel (four clips, the families dealt over them).
    The first K weight rows are the identity: those outputs are the prologue's own, held to the prologue's bound."""
    def make(dt):
        if family == "benign":
            return [g(dt, K + 20 + i, K=K, N=K + 9, batch=1, pro=LN, epi=GEPI_STORE, ln_shift=i, probe=True) for i in range(len(G.LN_FAMILIES))] + \
                   [g(dt, K + 30 + i, K=K, N=K + 9, batch=4, pro=LN, epi=GEPI_STORE, ln_shift=i, probe=True) for i in (0, 3)]
        if family == "outlier0":
            # how far a variance with the wrong shift strays is a matter of rounding luck: on these rows the arithmetic the prologues
            # had leaves the two-pass bound on about three rows in ten (float32 emulation, 960 rows), so each kernel gets 12 / 18 rows
            return [g(dt, K + 50 + i, K=K, N=K + 9, batch=1, pro=LN, epi=GEPI_STORE, family=family, probe=True) for i in range(12)] + \
                   [g(dt, K + 70 + i, K=K, N=K + 9, batch=(4, 4, 4, 4, 2)[i], pro=LN, epi=GEPI_STORE, family=family, probe=True) for i in range(5)]
        return [g(dt, K + 40 + b, K=K, N=K + 9, batch=b, pro=LN, epi=GEPI_STORE, family=family, probe=True) for b in (1, 2, 4)]
    return make


N_PARTS = (1, 63, 64, 65, 203)
DS = (384, 768, 1280, 2048)


def advance_case(batch):
    """1, 4, 17, 33 clips = 1, 2, 3 workgroups (a workgroup with one live wave); every n_part, d_model dealt over them; n_prefix 0
    (-> 4) and 3; done_host and max_new_clip set and null; a second launch on the same buffers."""
    bi = (1, 4, 17, 33).index(batch)
    return lambda dt: [G.advance_group(dt, 3 * batch + i, batch=batch, d=DS[(i + bi) % 4], n_part=n_part, n_prefix=(0, 3)[(i + bi) % 2],
                                       done_host=i % 2 == 0, max_new_clip=i % 3 != 1) for i, n_part in enumerate(N_PARTS)]


def advance_forced_case(dt):
    """Teacher forcing: gi < n_forced, gi == n_forced and beyond among the clips; argmax_dump set and null."""
    return [G.advance_group(dt, 70 + i, batch=batch, d=DS[i % 4], n_part=(64, 65, 1, 203)[i], n_prefix=(0, 3)[i % 2], forced=True, dump=dump)
            for i, (batch, dump) in enumerate(((4, True), (17, True), (17, False), (33, True)))]


CASES = {f"instantiation K={K}": inst_case(K) for K in KS}
CASES.update({f"LN -> QKV_CACHE d={d}": qkv_case(d) for d in (384, 1280)})
CASES.update({f"COMBINE -> RESID n_split={s}": combine_case(s) for s in (1, 3, 8)})
CASES["LN -> STORE"] = lambda dt: [g(dt, 51 + b, K=768, N=40, batch=b, pro=LN, epi=GEPI_STORE, family="realistic") for b in (1, 3)]
CASES["LN -> GELU N=4d"] = lambda dt: [g(dt, 55 + b, K=384, N=1536, batch=b, pro=LN, epi=GEPI_GELU, family="realistic") for b in (1, 2)]
CASES["PLAIN -> RESID K=4d"] = lambda dt: [g(dt, 58 + b, K=1536, N=384, batch=b, pro=PLAIN, epi=GEPI_RESID, family="realistic") for b in (1, 4)]
CASES["LN -> LOGITS"] = lambda dt: [g(dt, 61 + b, K=384, N=300, batch=b, pro=LN, epi=GEPI_LOGITS, ties=True, dump=b != 2) for b in (1, 2, 4)]
CASES.update({f"two passes LPR={lpr} epilogue={epi}": multipass_case(lpr, epi) for lpr in MULTIPASS for epi in (GEPI_LOGITS, GEPI_RESID, GEPI_STORE)})
CASES.update({f"vocabulary N={N}": (lambda N: lambda dt: [g(dt, N + b, K=384, N=N, batch=b, pro=LN, epi=GEPI_LOGITS, ties=True, family="realistic")
                                                          for b in (1, 4)])(N) for N in (51865, 51866)})
CASES["skip_before_step"] = skip_case
CASES.update({f"LayerNorm {fam} K={K}": ln_case(K, fam) for K in (384, 768, 1280) for fam in ("benign", "realistic", "outlier0")})
CASES.update({f"advance batch={b}": advance_case(b) for b in (1, 4, 17, 33)})
CASES["advance teacher forcing"] = advance_forced_case
CASES["embed"] = lambda dt: [G.embed_group(dt, d, batch=5, d=d) for d in (384, 1280)]


def wanted_forms():
    want = set()
    for K, (lpr, ch) in KS.items():
        want |= {("gemv1", lpr, ch, LN, GEPI_STORE), ("gemv1", lpr, ch, PLAIN, GEPI_RESID), ("gemv<1>", lpr, ch, CMB, GEPI_STORE),
                 ("gemv<4>", lpr, ch, LN if K <= 2048 else PLAIN, GEPI_GELU), ("gemv<4>", lpr, ch, PLAIN, GEPI_STORE), ("gemv<4>", lpr, ch, CMB, GEPI_RESID)}
    for kern in ("gemv1", "gemv<4>"):  # each epilogue with the prologue the engine pairs it with
        want |= {(kern, 16, 3, LN, GEPI_QKV_CACHE), (kern, 32, 5, LN, GEPI_QKV_CACHE), (kern, 32, 3, LN, GEPI_STORE), (kern, 16, 3, LN, GEPI_GELU),
                 (kern, 64, 3, PLAIN, GEPI_RESID), (kern, 16, 3, LN, GEPI_LOGITS)}
        want |= {(kern, lpr, MULTIPASS[lpr][0] // (8 * lpr), pro, epi) for lpr in MULTIPASS for pro, epi in ((LN, GEPI_LOGITS), (PLAIN, GEPI_RESID), (LN, GEPI_STORE))}
    want |= {("gemv<1>", 16, 3, CMB, GEPI_RESID), ("gemv<4>", 16, 3, CMB, GEPI_RESID)}
    want |= {("advance", n, "greedy") for n in (1, 2, 3)} | {("advance", n, "forced") for n in (1, 2, 3)} | {("embed",)}
    return want


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, kernel_driver.driver_exe(request.param)


@pytest.mark.parametrize("name", list(CASES))
def test_case(driver, tmp_path, name):
    kernel_driver.run_groups(_session, G.verify, G.gemv_form, G.grid_of, driver, tmp_path, CASES[name](driver[0]), timeout=120)


def test_every_gemv_kernel_ran_every_form(driver):
    dt, _ = driver
    want = wanted_forms()
    assert want <= _session.ran[dt], sorted(want - _session.ran[dt], key=str)


def test_zz_report(driver):
    dt, _ = driver
    for (t, what), w in sorted(_session.worst.items()):
        if t == dt:
            print(f"{dt} {what}: worst error / bound {w:.3f}")
    print(f"wall time so far {time.time() - _session.state['t0']:.0f} s")
