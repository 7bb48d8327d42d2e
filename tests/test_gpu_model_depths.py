"""GPU: the decode paths at the DEPTH EDGES of the persistent launch, and base / large at their advertised size.

Which decode path a call runs is decided silently at Init from the model's shape (DESIGN.md "Which decode path a model shape
gets"; tests/test_persistent_plan_host.py checks the rule and the role assignment on the host). On 256 CUs the persistent
launch has P = min(256, d_model) workgroups, L*H of them own a self-attention head, and the NS = P - L*H others take the
cross-attention units: one clip per launch needs NS >= 2*3*H, two or three clips NS >= nc*3*H (d_model <= 768). This file runs,
for every width of persist_dispatch, the deepest decoder with three clips per launch, the deepest with the persistent launch
and the first that falls back to the launch-per-phase paths (17 models, 1 encoder layer: the encoder's depth takes no part in
any of these decisions), two of them also in fp16, then `base` (6 + 6 layers, d 512) in both types and `large` (large-v3's
32-layer decoder at d 1280 behind a 2-layer encoder), which never gets the persistent launch.

Bounds. No model here had a measured logit error before, so none is invented: for every model the test computes on the CPU
D = max |logits(policy oracle) - logits(fp32 oracle)| along the policy oracle's own ids — the whole effect of 16-bit storage at
that depth, measured on the reference alone — and the engine's teacher-forced logits must be within 2*D of the POLICY oracle
(at Whisper-small the suite's bar of 6e-3 is 2.0*D, the error measured there 0.6*D). Between two engine paths on one model the
existing bounds hold: exact ids between multi-clip and one-clip persistent launches, 2e-3 abs between decode paths at a step
where their argmax differs. A differing id passes only as a measured tie (oracle's top-2 margin < 2 x the logit error at that
step + 1e-4), at most 1 + decisions // 500 per model. Seeds: the oracle's own steps with a margin below 4*D + 1e-4 (the most the
tie rule could ever accept under the 2*D bound) are counted on the CPU for clip A of every model and must stay within that cap
as well (a seed whose oracle walks along a near-tie for many steps is not kept: up to 18 of 73 steps were seen); the counts
found when the seeds were chosen stand next to them below.

Every model is built once, used by one test and freed (large: 5.6 GB of host memory, 1.8 GB on disk)."""
import contextlib
import gc
import os
import shutil
import time
from collections import namedtuple

import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

import modelgen
from conftest import ModelCase, assert_ids_equal_or_tie, load_demo_pcm
from make_model_goldens_inputs import demo_mel, synth_mel

pytestmark = pytest.mark.gpu

# name, d_model, decoder layers, then what Init must report on 256 CUs — LITERALS, not computed: persistent_decode,
# persistent_max_clips (1 where there is no persistent launch), persistent_qfold (persistent and d <= 768), then seed, dtype,
# full: the deepest persistent model of its width also runs the whole context (444 ids) against AX_WHISPER_DECODE=graph.
Spec = namedtuple("Spec", "name d layers persistent max_clips qfold seed dtype full")
DEPTH_EDGE_MODELS = [
    #                                              near = oracle steps (of 73) with margin < 4*D + 1e-4 on the CPU
    Spec("d128L55", 128, 55, 1, 3, 1, 201, "BF16", False),   # near 1
    Spec("d128L58", 128, 58, 1, 2, 1, 402, "BF16", True),   # near 0
    Spec("d128L59", 128, 59, 0, 1, 0, 103, "BF16", False),   # near 0
    Spec("d256L55", 256, 55, 1, 3, 1, 204, "BF16", False),   # near 0
    Spec("d256L58", 256, 58, 1, 2, 1, 105, "BF16", True),   # near 1
    Spec("d256L59", 256, 59, 0, 1, 0, 106, "BF16", False),   # near 1
    Spec("d384L33", 384, 33, 1, 3, 1, 507, "BF16", False),   # near 1
    Spec("d384L36", 384, 36, 1, 2, 1, 308, "BF16", True),   # near 1
    Spec("d384L37", 384, 37, 0, 1, 0, 109, "BF16", False),   # near 0
    Spec("d512L23", 512, 23, 1, 3, 1, 110, "BF16", False),   # near 1
    Spec("d512L26", 512, 26, 1, 2, 1, 211, "BF16", True),   # near 1
    Spec("d512L27", 512, 27, 0, 1, 0, 212, "BF16", False),   # near 0
    Spec("d768L12", 768, 12, 1, 3, 1, 113, "BF16", False),   # near 1
    Spec("d768L15", 768, 15, 1, 2, 1, 114, "BF16", True),   # near 1
    Spec("d768L16", 768, 16, 0, 1, 0, 115, "BF16", False),   # near 0
    Spec("d1280L6", 1280, 6, 1, 1, 0, 116, "BF16", True),   # near 0
    Spec("d1280L7", 1280, 7, 0, 1, 0, 217, "BF16", False),   # near 1
]
# the deepest persistent model at d = 768 and at d = 1280 in the IEEE-half build of every kernel
FP16_MODELS = [
    Spec("d768L15h", 768, 15, 1, 2, 1, 118, "F16", False),   # near 0
    Spec("d1280L6h", 1280, 6, 1, 1, 0, 119, "F16", False),   # near 0
]
# A workgroup of a multi-clip launch may own cross-attention units in CONSECUTIVE layers; the next unit's K tiles are then staged
# behind this layer's attention block and not ahead of it (decode_persistent2.hip). On 256 CUs that needs, for two clips, L >= 10
# at d = 768, 21 at 512, 31 at 384, 53 at 128 / 256, and for three clips L >= 4, 15, 25, 47. Per width and clips per launch, the
# model below whose equality test (_groups_equal_members) runs such a launch; test_persistent_plan_host.py verifies the claim
# with the product's own assignment function.
CONSECUTIVE_LAYER_MODELS = {
    128: {2: "d128L58", 3: "d128L55"}, 256: {2: "d256L58", 3: "d256L55"}, 384: {2: "d384L36", 3: "d384L33"},
    512: {2: "d512L26", 3: "d512L23"}, 768: {2: "d768L15", 3: "d768L12"},
}

N_ONE = 72    # ids of the one-clip and the equality checks: 76 keys, the self-attention cache crosses its first 64-key block
N_MANY = 12   # ids wherever several clips are checked against the oracle


def _g(e, key):
    return e.L.AX_WHISPER_GetConfigInt(e.h, key.encode())


@contextlib.contextmanager
def _env(key, value):
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old


@pytest.fixture(scope="module")
def cu256():
    """The literals below are those of a 256-CU device (MI355X); on any other the dispatch differs: skip, as _need_clips does."""
    n = torch.cuda.get_device_properties(0).multi_processor_count
    if n != 256:
        pytest.skip(f"the dispatch literals of this file are those of 256 CUs, this device has {n}")
    return n


class _Tally:
    """Accepted ties of one model; every one is asserted as a tie where it is found."""

    def __init__(self):
        self.ties = self.decisions = 0
        self.worst = 0.0   # logit error against the policy oracle

    def tie(self, margin, err, what):
        assert margin < 2 * err + 1e-4, (what, "margin", float(margin), "logit err", float(err))
        self.ties += 1

    def check(self, near):
        """near: the oracle's own steps with a margin below 4*D + 1e-4 — the seed must keep them within the cap as well."""
        cap = 1 + self.decisions // 500
        assert self.ties <= cap and near <= cap, (self.ties, near, self.decisions)


def _first_diff(a, b):
    return next(i for i in range(min(len(a), len(b))) if a[i] != b[i])


def _margin(row):
    srt = np.sort(row)
    return float(srt[-1] - srt[-2])


class _Ref:
    """The policy oracle's greedy ids and logits for one input; with_d: also D and the near-tie count of the docstring."""

    def __init__(self, case, mel, n, with_d=False):
        self.mel = mel
        ck, cv = case.oracle_bf16.encoder(mel)
        self.ck, self.cv = (ck, cv) if with_d else (None, None)
        self.ids, self.lg = case.oracle_bf16.greedy(ck, cv, "zh", max_new=n, want_logits=True)
        assert len(self.ids) == n and self.lg.shape[0] == n + 1
        if with_d:
            ck32, cv32 = case.oracle_fp32.encoder(mel)
            ids32, lg32 = case.oracle_fp32.greedy(ck32, cv32, "zh", forced=self.ids, want_logits=True)
            assert lg32.shape == self.lg.shape
            self.D = float(np.abs(self.lg - lg32).max())
            srt = np.sort(self.lg, axis=1)
            self.near = int((srt[:, -1] - srt[:, -2] < 4 * self.D + 1e-4).sum())
            self.std = float(self.lg.std())


def _vs_oracle(e, refs, n, D, tally, what):
    """len(refs) clips in one call: teacher-forced logits of every clip within 2*D of its policy-oracle logits, greedy ids equal
    to the oracle's or a measured tie at the first difference."""
    B = len(refs)
    e.encode_mel(np.stack([r.mel for r in refs]))
    forced = np.array([r.ids[:n] for r in refs], dtype=np.int32)
    logits, _ = e.decode_forced(B, forced)
    got = e.decode_greedy(B, max_new=n)
    worst = 0.0
    for b, r in enumerate(refs):
        err = np.abs(logits[b, : n + 1] - r.lg[: n + 1]).max(axis=1)
        worst = max(worst, float(err.max()))
        assert len(got[b]) == n, (what, b, len(got[b]))
        if got[b] != list(r.ids[:n]):
            i = _first_diff(got[b], r.ids)
            tally.tie(_margin(r.lg[i]), err[i], (what, "clip", b, "step", i))
    tally.decisions += B * n
    tally.worst = max(tally.worst, worst)
    print(f"    {what}: {B} clip(s) x {n + 1} steps, logits err vs policy oracle {worst:.3e} = {worst / D:.2f} D")
    assert worst < 2 * D, (what, worst, D)


def _single_ids(e, mels, n):
    out = []
    for m in mels:
        e.encode_mel(m)
        out.append(e.decode_greedy(1, max_new=n)[0])
        assert len(out[-1]) == n
    return out


def _groups_equal_members(e, mels, single, nc, n):
    """The contract of test_two_clip_launch_equals_one_clip_launches / test_three_clip_...: a pair or triple of different clips
    gives EXACTLY the ids of its members decoded alone, in several orders, twice (the second run starts on a used cache), and
    with per-clip budgets."""
    assert _g(e, "persistent_max_clips") >= nc
    orders = {2: ((0, 1), (1, 0), (1, 2), (2, 0)), 3: ((0, 1, 2), (2, 1, 0), (1, 2, 0), (1, 1, 2))}[nc]
    for order in orders:
        e.encode_mel(np.stack([mels[i] for i in order]))
        for _ in range(2):
            assert e.decode_greedy(nc, max_new=n) == [single[i] for i in order], (nc, order)
    cut = [n // 3, n - 1, 2][:nc]
    for order in (orders[0], orders[1]):
        e.encode_mel(np.stack([mels[i] for i in order]))
        assert e.decode_greedy(nc, max_new=n, max_new_clip=cut) == [single[i][:c] for i, c in zip(order, cut)], (nc, order, cut)
    assert _g(e, "persistent_decode") == 1 and _g(e, "persistent_giveups") == 0


def _fallback_vs_single(e, mels, single, n, tally, what):
    """More clips than one persistent launch takes: the rule of test_gpu_configs._batch_vs_single_and_oracle. ids equal the
    one-clip runs, or differ at a tie measured on the teacher-forced logits of both paths (2e-3 between the paths there)."""
    B = len(mels)
    e.encode_mel(np.stack(mels))
    got = e.decode_greedy(B, max_new=n)
    forced = np.array(single, dtype=np.int32)
    lg_b, am_b = e.decode_forced(B, forced)
    n_tied, between = 0, 0.0
    for b in range(B):
        e.encode_mel(mels[b])
        lg_1, _ = e.decode_forced(1, forced[b:b + 1])
        between = max(between, float(np.abs(lg_b[b] - lg_1[0]).max()))
        steps = [s for s in range(n) if am_b[b, s] != single[b][s]]
        for s in steps:
            err = float(np.abs(lg_b[b, s] - lg_1[0, s]).max())
            assert err < 2e-3, (what, "clip", b, "step", s, "logit error between the decode paths", err)
            tally.tie(_margin(lg_1[0, s]), err, (what, "clip", b, "step", s))
        n_tied += len(steps)
        assert len(got[b]) == n
        if got[b] != single[b]:  # the greedy runs part ways exactly at a tied step
            assert _first_diff(got[b], single[b]) in steps, (what, "clip", b, "diverges without a tie", steps)
    tally.decisions += B * n
    print(f"    {what}: {B} clips x {n} ids vs the one-clip runs, {n_tied} tied steps, logits of the two paths differ by {between:.3e}")


def _full_context(wa, spec, case, mel, ep, tally):
    """444 ids: the persistent launch against AX_WHISPER_DECODE=graph by the tie rule."""
    with _env("AX_WHISPER_DECODE", "graph"):
        eg = wa.Whisper(spec.name, case.root, "zh", device=0, max_batch=1)
    try:
        assert _g(eg, "persistent_decode") == 0
        ep.encode_mel(mel)
        eg.encode_mel(mel)
        ids_p, ids_g = ep.decode_greedy(1)[0], eg.decode_greedy(1)[0]
        assert len(ids_p) == 444 and len(ids_g) == 444
        if ids_p != ids_g:
            i = _first_diff(ids_p, ids_g)
            forced = np.array([ids_p[:i]], dtype=np.int32).reshape(1, i)
            lp, _ = ep.decode_forced(1, forced)
            lgr, _ = eg.decode_forced(1, forced)
            err = float(np.abs(lp[0, i] - lgr[0, i]).max())
            assert err < 2e-3, ("full context, step", i, "logit error between the decode paths", err)
            tally.tie(_margin(lgr[0, i]), err, ("full context, step", i))
            print(f"    full context: persistent and graph part ways at id {i} of 444 (a tie, logits differ by {err:.3e})")
        else:
            print("    full context: 444 ids identical, persistent launch and graph path")
        tally.decisions += 444
    finally:
        eg.close()


def _mels(n_mels, seed):
    # seeded weights barely listen to ordinary audio: the third input is a constant far outside the normal range, so that the
    # members of a group have different ids and a launch that mixed its clips up could not pass (test_gpu_persistent.py)
    return [demo_mel(n_mels), synth_mel(300 + seed, n_mels, 2200), np.full((n_mels, 3000), 5.0, dtype=np.float32)]


def _report(spec, e, ref, tally, t0):
    print(f"{spec.name} ({spec.dtype}, seed {spec.seed}): persistent_decode {_g(e, 'persistent_decode')} max_clips {_g(e, 'persistent_max_clips')} "
          f"qfold {_g(e, 'persistent_qfold')} grid {_g(e, 'persistent_grid')} | D {ref.D:.3e} (near-ties {ref.near}, logit std {ref.std:.2f}) | "
          f"logits err {tally.worst:.3e} = {tally.worst / ref.D:.2f} D | ties accepted {tally.ties} of {tally.decisions} decisions | "
          f"persistent_giveups = {_g(e, 'persistent_giveups')} | {time.time() - t0:.1f} s")


def _run_checks(checks):
    """Every check of a model runs, whatever an earlier one found (a model costs seconds of weight synthesis): assertion
    failures are collected and raised together. Anything else (a HIP error, a fault) ends the test at once."""
    fails = []
    for name, fn in checks:
        try:
            fn()
        except AssertionError as ex:
            fails.append(f"{name}: {ex}")
            print(f"    FAILED {name}: {ex}")
    assert not fails, "\n".join(fails)


def _depth_model(spec, wa, tmp_path_factory):
    t0 = time.time()
    modelgen.DIMS[spec.name] = modelgen.depth_dims(spec.d, spec.layers)
    root = tmp_path_factory.mktemp(spec.name)
    case = ModelCase(root, spec.name, spec.seed, dtype=spec.dtype)
    e = None
    try:
        n_mels = case.dims["n_mels"]
        mels = _mels(n_mels, spec.seed)
        ref = _Ref(case, mels[0], N_ONE, with_d=True)
        print(f"{spec.name}: D {ref.D:.3e}, near-ties {ref.near}, logit std {ref.std:.2f}, oracle side {time.time() - t0:.1f} s")
        e = wa.Whisper(spec.name, case.root, "zh", device=0, max_batch=6)
        tally = _Tally()
        single = []

        def dispatch():
            got = (_g(e, "persistent_decode"), _g(e, "persistent_max_clips"), _g(e, "persistent_qfold"), _g(e, "fp16"))
            assert got == (spec.persistent, spec.max_clips, spec.qfold, int(spec.dtype == "F16")), got
            assert _g(e, "persistent_grid") == (min(256, spec.d) if spec.persistent else 0)
            assert (e.n_text_state, e.n_text_layer) == (spec.d, spec.layers)

        def one_clip():
            _vs_oracle(e, [ref], N_ONE, ref.D, tally, "one clip")
            e.encode_mel(ref.mel)
            got = e.decode_greedy(1, max_new=N_ONE)[0]   # (again, through the helper every other file uses)
            assert_ids_equal_or_tie(e, ref.mel, got, ref.ids, ref.lg, spec.name)

        def members():
            single[:] = _single_ids(e, mels, N_ONE)
            assert single[0] != single[2] and single[1] != single[2]   # the inputs tell the clips apart

        def groups():
            for nc in range(2, spec.max_clips + 1):
                _groups_equal_members(e, mels, single, nc, N_ONE)
                print(f"    {nc}-clip launches: ids equal to their members' in every order")

        def one_clip_more():
            nc = spec.max_clips + 1
            order = (0, 2, 1)[:nc]
            _fallback_vs_single(e, [mels[i] for i in order], [single[i] for i in order], N_ONE, tally, f"{nc} clips (launch-per-phase)")

        def unsupported_side():
            ref_b = _Ref(case, mels[1], N_MANY)
            for B in (1, 2, 3, 6):
                _vs_oracle(e, [ref if b % 2 == 0 else ref_b for b in range(B)], N_MANY, ref.D, tally, f"{B} clip(s), launch-per-phase")
            assert _g(e, "persistent_decode") == 0

        def full_context():
            _full_context(wa, spec, case, mels[0], e, tally)

        def giveups():
            assert _g(e, "persistent_giveups") == 0 and _g(e, "persistent_decode") == spec.persistent
            tally.check(ref.near)

        checks = [("dispatch", dispatch), ("one clip vs oracle", one_clip)]
        if spec.persistent:
            checks.append(("members", members))
            if spec.max_clips >= 2:
                checks.append(("multi-clip launches equal one-clip launches", groups))
            if spec.max_clips < 3:
                checks.append(("one clip more than the launch takes", one_clip_more))
            if spec.full:
                checks.append(("full context", full_context))
        else:
            checks.append(("unsupported side", unsupported_side))
        checks.append(("give-ups and ties", giveups))
        try:
            _run_checks(checks)
        finally:
            _report(spec, e, ref, tally, t0)
    finally:
        if e is not None:
            e.close()
        del case
        gc.collect()
        shutil.rmtree(str(root), ignore_errors=True)


# MI355X figures: none recorded here yet. Every model prints one line (dispatch integers, D, logit error against the policy
# oracle in units of D, ties accepted, persistent_giveups, wall time); D on the CPU when the seeds were chosen: 1.4e-3 .. 2.3e-3
# at d = 128, 2.1e-3 .. 2.8e-3 at 256, 2.6e-3 .. 2.9e-3 at 384, 2.8e-3 .. 3.6e-3 at 512, 3.1e-3 .. 3.5e-3 at 768, 4.4e-3 .. 4.7e-3
# at 1280 (bf16); 4.5e-4 / 4.7e-4 for the two fp16 models; base 2.3e-3 (bf16) / 3.2e-4 (fp16); large 5.2e-3.
@pytest.mark.parametrize("spec", DEPTH_EDGE_MODELS, ids=[s.name for s in DEPTH_EDGE_MODELS])
def test_depth_edge_model(built_lib, oracle_mod, tmp_path_factory, cu256, spec):
    _depth_model(spec, built_lib, tmp_path_factory)


@pytest.mark.parametrize("spec", FP16_MODELS, ids=[s.name for s in FP16_MODELS])
def test_deepest_persistent_model_in_fp16(built_lib, oracle_mod, tmp_path_factory, cu256, spec):
    _depth_model(spec, built_lib, tmp_path_factory)


# ------------------------------------------------------------------------------------------------ base at full size
@pytest.mark.parametrize("dtype,seed", [("BF16", 220), ("F16", 121)])   # near 1 / 0 (of 21 steps)
def test_base_at_full_size(built_lib, oracle_mod, tmp_path_factory, cu256, dtype, seed):
    """`base` (6 + 6 layers, d = 512) as whisper_cli advertises it: one clip end to end and teacher-forced as
    test_gpu_fullsize.py does for small, pairs and triples equal to their members, 6 and 20 clips through the clip-block
    sequence against the oracle (the clip-block query fold at d = 512 deeper than two layers)."""
    t0 = time.time()
    spec = Spec("base", 512, 6, 1, 3, 1, seed, dtype, False)
    root = tmp_path_factory.mktemp("base_" + dtype)
    case = ModelCase(root, "base", seed, dtype=dtype)
    e = None
    try:
        pcm = load_demo_pcm()
        mel_a = oracle_mod.log_mel(pcm, 80)[0]
        mels = [mel_a] + _mels(80, seed)[1:]
        ref = _Ref(case, mel_a, 20, with_d=True)
        ref_b = _Ref(case, mels[1], N_MANY)
        print(f"base {dtype}: D {ref.D:.3e}, near-ties {ref.near}, logit std {ref.std:.2f}, oracle side {time.time() - t0:.1f} s")
        e = built_lib.Whisper("base", case.root, "zh", device=0, max_batch=20)
        tally = _Tally()
        single = []

        def dispatch():
            got = (_g(e, "persistent_decode"), _g(e, "persistent_max_clips"), _g(e, "persistent_qfold"), _g(e, "fp16"), _g(e, "batched_ln"))
            assert got == (1, 3, 1, int(dtype == "F16"), 1), got
            assert (e.n_text_state, e.n_text_layer, e.n_mels) == (512, 6, 80)

        def end_to_end():
            got = e.run_tokens(pcm, max_new=20)
            e.encode_mel(e.compute_mel(pcm))
            logits, _ = e.decode_forced(1, np.array([ref.ids], dtype=np.int32))
            k, v = e.get_cross_kv(0)
            # stored 16-bit on both sides: a value may fall on either side of a rounding boundary -> two ulps of its magnitude
            ulp2 = 2.0 ** -7 if dtype == "BF16" else 2.0 ** -10
            dk, dv = np.abs(k - ref.ck), np.abs(v - ref.cv)
            print(f"    base {dtype} cross K/V max diff {dk.max():.3e} {dv.max():.3e}, mean {dk.mean():.2e} {dv.mean():.2e}, scale {np.abs(ref.ck).max():.2f}")
            assert (dk <= ulp2 * np.maximum(np.abs(ref.ck), 1.0)).all() and (dv <= ulp2 * np.maximum(np.abs(ref.cv), 1.0)).all()
            assert dk.mean() < 2e-3 and dv.mean() < 2e-3
            err = np.abs(logits[0] - ref.lg).max(axis=1)
            tally.worst = max(tally.worst, float(err.max()))
            print(f"    end to end: logits err vs policy oracle {err.max():.3e} = {err.max() / ref.D:.2f} D")
            assert err.max() < 2 * ref.D, (float(err.max()), ref.D)
            if got != ref.ids:
                i = _first_diff(got, ref.ids)
                tally.tie(_margin(ref.lg[i]), err[i], ("end to end, step", i))
            assert len(got) == 20
            tally.decisions += 20

        def groups():
            single[:] = _single_ids(e, mels, N_ONE)
            assert single[0] != single[2] and single[1] != single[2]
            for nc in (2, 3):
                _groups_equal_members(e, mels, single, nc, N_ONE)

        def clip_blocks():
            for B in (6, 20):
                _vs_oracle(e, [ref if b % 2 == 0 else ref_b for b in range(B)], N_MANY, ref.D, tally, f"{B} clips, clip-block sequence")

        def giveups():
            assert _g(e, "persistent_giveups") == 0 and _g(e, "persistent_decode") == 1
            tally.check(ref.near)

        try:
            _run_checks([("dispatch", dispatch), ("one clip end to end", end_to_end), ("pairs and triples", groups),
                         ("6 and 20 clips", clip_blocks), ("give-ups and ties", giveups)])
        finally:
            _report(spec, e, ref, tally, t0)
    finally:
        if e is not None:
            e.close()
        del case
        gc.collect()
        shutil.rmtree(str(root), ignore_errors=True)


# ------------------------------------------------------------------------------------------------ large-v3's decoder
def test_large_decoder_takes_the_launch_per_phase_paths(built_lib, oracle_mod, tmp_path_factory, cu256):
    """`large` (modelgen.DIMS: large-v3) has 32 x 20 = 640 self-attention owners: no persistent launch on any device, by shape and
    not by a give-up. The full 32-layer decoder behind a 2-layer encoder: 1 and 2 clips (GEMV family), 6 and 20 clips (split-K
    sequence at d = 1280) teacher-forced against the policy oracle, greedy ids by the tie rule."""
    t0 = time.time()
    full = modelgen.DIMS["large"]
    assert (full["d"], full["heads"], full["enc_layers"], full["dec_layers"], full["n_mels"], full["n_vocab"], full["n_langs"]) == (1280, 20, 32, 32, 128, 51866, 100)
    name = "large32"
    modelgen.DIMS[name] = dict(full, enc_layers=2)
    spec = Spec(name, 1280, 32, 0, 1, 0, 122, "BF16", False)   # near 0 (of 13 steps)
    root = tmp_path_factory.mktemp(name)
    case = ModelCase(root, name, spec.seed)
    e = None
    try:
        mels = _mels(128, spec.seed)
        ref = _Ref(case, mels[0], N_MANY, with_d=True)
        ref_b = _Ref(case, mels[1], N_MANY)
        print(f"{name}: D {ref.D:.3e}, near-ties {ref.near}, logit std {ref.std:.2f}, oracle side {time.time() - t0:.1f} s")
        e = built_lib.Whisper(name, case.root, "zh", device=0, max_batch=20)
        tally = _Tally()

        def dispatch():
            got = (_g(e, "persistent_decode"), _g(e, "persistent_max_clips"), _g(e, "persistent_qfold"), _g(e, "persistent_grid"), _g(e, "batched_ln"))
            assert got == (0, 1, 0, 0, 0), got
            assert (e.n_text_state, e.n_text_layer, e.n_mels, e.n_vocab) == (1280, 32, 128, 51866)

        def paths():
            for B in (1, 2, 6, 20):
                _vs_oracle(e, [ref if b % 2 == 0 else ref_b for b in range(B)], N_MANY, ref.D, tally, f"{B} clip(s)")

        def giveups():
            assert _g(e, "persistent_giveups") == 0 and _g(e, "persistent_decode") == 0
            tally.check(ref.near)

        try:
            _run_checks([("dispatch", dispatch), ("1, 2, 6 and 20 clips", paths), ("give-ups and ties", giveups)])
        finally:
            _report(spec, e, ref, tally, t0)
    finally:
        if e is not None:
            e.close()
        del case
        gc.collect()
        shutil.rmtree(str(root), ignore_errors=True)
