"""GPU: the two- and three-clip persistent launch (decode_persistent2.hip) by its NUMBERS, not only its ids.

The launch takes no teacher forcing and no dumps, and seeded weights give ordinary audio clips identical greedy ids, so the id
comparisons of test_gpu_persistent.py cannot tell a clip from its neighbour. Here the three mels of
persist_cache_reference.mels (pairwise different ids, a cache that moves by ~1 under a neighbour's cross K/V) go through the
launch in every later position, and the later clips' self-attention caches (global memory, AX_WHISPER_GetPersistentSelfKV) are
compared whole against the bf16-/f16-policy oracle, teacher forced along the launch's own ids and fed the ENGINE's cross K/V
(the encoder is tested elsewhere). Row t of layer l is W_k / W_v . LN(residual stream entering layer l at step t): embedding,
every earlier layer's self-attention over this very cache, cross-attention over the clip's own slot, the query fold, the MLP.

(a) rows [0, n + 4) of clips 1 and 2 within ulp16(ref) + A of the oracle, element by element; rows >= the steps run all-zero bits
(b) the inputs discriminate: a neighbour's cross K/V moves the oracle's cache by >= 8 x the largest tolerance of (a)
(c) the cache of one mel is bit-identical as clip 1 of two, clip 1 of three and clip 2 of three
(d) ids of every clip in every order == that mel's one-clip ids, the three lists pairwise different
(e) unequal budgets: rows [0, n + 4) as in (a), ride-along rows up to the steps run finite, zero beyond

A (persist_cache_reference.A) = 4 x A0 rounded up to one digit; A0 = the largest excess of |got - ref| over ulp16(ref) of the
launch-per-phase decoder's cache (AX_WHISPER_DECODE=graph, one clip, decode_forced + get_self_kv) against the same oracle on these
cases (profiles/scripts/persist_cache_a0.py -> profiles/persist_cache_a0.txt); measured on an MI355X:
    BF16: A0 = 1.465e-3 (small/43), A = 6e-3;   F16: A0 = 4.578e-5 (tiny/44), A = 2e-4
Never taken from the multi-clip launch itself."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

import persist_cache_reference as prc
from conftest import ModelCase

pytestmark = pytest.mark.gpu

# model, seed, dtype, clips per launch, max_new (0: full context, 444 ids = 448 rows = all 7 used blocks; 68: rows up to 71, one
# crossing of the 64-key block edge). w512 runs two clips per launch at most; small with three clips is the one shape whose
# 3 x 36 cross-attention units fill the 112 workgroups without a head.
CASES = [
    ("micro", 41, "BF16", (2, 3), 0),
    ("mini", 31, "BF16", (2, 3), 68),
    ("tiny", 42, "BF16", (2, 3), 68),
    ("tiny", 44, "F16", (2, 3), 68),
    ("w512", 33, "BF16", (2,), 68),
    ("small", 43, "BF16", (3,), 68),
]
ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))   # every mel in every position; a two-clip launch takes the first two slots


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Launches:
    """One model: the one-clip ids of the three mels, then every multi-clip launch of the case (each run twice: the second starts
    from a used cache) with its ids, steps and the later clips' caches; the oracle's cache per mel, computed once."""

    def __init__(self, wa, tmpdir, model_type, seed, dtype, launches, max_new):
        self.name = "%s/%d %s" % (model_type, seed, dtype)
        self.dtype, self.a, self._ref = dtype, prc.A[dtype], {}
        self.case = ModelCase(tmpdir, model_type, seed, dtype=dtype)
        self.mels = prc.mels(self.case.dims["n_mels"])
        e = wa.Whisper(model_type, self.case.root, "zh", device=0, max_batch=3)
        try:
            have = e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_max_clips")
            if have < max(launches):  # a smaller part or a CU-masked queue decodes such groups another way (test_gpu_persistent._need_clips)
                pytest.skip(f"this device runs {have} clip(s) per persistent launch, the test needs {max(launches)}")
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"fp16") == (1 if dtype == "F16" else 0)
            self.n_ctx = e.n_text_ctx
            self.full = max_new if max_new > 0 else self.n_ctx - 4
            self.single = []
            for m in self.mels:
                e.encode_mel(m)
                self.single.append(e.decode_greedy(1, max_new=max_new)[0])
            # Every launch reads an encode of all THREE mels, a two-clip launch its first two slots: the encoder's GEMMs see other
            # shapes at another batch size, and the cross K/V of a mel then differs in its last bits, which (c) must not see.
            # Within one batch size the cross K/V of a mel is bit-equal in every slot (asserted): one oracle pass per mel.
            self.kv = [None, None, None]
            self.runs = []
            for order, m3, m2 in zip(ORDERS, ([self.full, self.full // 3, 2], [2, self.full, self.full // 3], None),
                                     ([self.full, self.full // 3], [self.full // 3, self.full], None)):
                e.encode_mel(np.stack([self.mels[i] for i in order]))
                for slot, i in enumerate(order):
                    ck, cv = e.get_cross_kv(slot)
                    if self.kv[i] is None:
                        self.kv[i] = (ck, cv)
                    assert _bits_equal(ck, self.kv[i][0]) and _bits_equal(cv, self.kv[i][1]), ("cross K/V of a mel depends on its slot", order, slot)
                for B in launches:
                    mc = m3 if B == 3 else m2
                    self.runs.append(self._launch(e, B, order[:B], max_new, None))
                    if mc is not None:
                        self.runs.append(self._launch(e, B, order[:B], max_new, mc))
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_giveups") == 0
        finally:
            e.close()

    def _launch(self, e, B, order, max_new, mc):
        out = []
        for _ in range(2):
            ids = e.decode_greedy(B, max_new=max_new, max_new_clip=mc)
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_giveups") == 0
            out.append(dict(B=B, order=order, budgets=mc, ids=ids, steps=e.timings()["steps"],
                            cache={c: e.get_persistent_self_kv(c) for c in range(1, B)}))
        a, b = out
        assert a["ids"] == b["ids"] and a["steps"] == b["steps"], (B, order, mc)
        for c in a["cache"]:   # a launch behind a used cache leaves exactly what a launch behind a fresh one does
            assert _bits_equal(a["cache"][c][0], b["cache"][c][0]) and _bits_equal(a["cache"][c][1], b["cache"][c][1]), (B, order, mc, c)
        return b

    def ref(self, i, ids):
        """Rows [0, len(ids) + 4) of the oracle's cache of mel i along ids. One oracle pass per (mel, id list); a prefix of a list
        already run is a prefix of its rows (causal; tests/test_persist_cache_reference.py)."""
        ids = list(ids)
        for key, (k, v) in self._ref.items():
            if key[0] == i and list(key[1][: len(ids)]) == ids:
                return k[:, : len(ids) + 4], v[:, : len(ids) + 4]
        k, v = prc.forced_cache(self.case.oracle_bf16, *self.kv[i], ids)
        self._ref[(i, tuple(ids))] = (k, v)
        return k, v

    def check_rows(self, run):
        """(a) / (e) for one launch -> (worst |err| / tolerance, largest tolerance used)."""
        worst = tol = 0.0
        steps = run["steps"]
        assert steps == max(len(x) for x in run["ids"]) + 4 <= self.n_ctx, (steps, [len(x) for x in run["ids"]])
        for c, (gk, gv) in run["cache"].items():
            i, ids = run["order"][c], run["ids"][c]
            n = len(ids) + 4
            rk, rv = self.ref(i, ids)
            for what, got, ref in (("K", gk, rk), ("V", gv, rv)):
                assert got.shape[1] == 512
                r = prc.worst_ratio(got[:, :n], ref, self.dtype, self.a)
                worst, tol = max(worst, r), max(tol, prc.max_tolerance(ref, self.dtype, self.a))
                assert r <= 1.0, (self.name, run["B"], run["order"], run["budgets"], "clip", c, what, "worst |err| / tolerance", r)
                assert np.isfinite(got[:, n:steps]).all(), (self.name, run["order"], run["budgets"], c, what, "ride-along rows")
                assert not got[:, steps:].view(np.uint32).any(), (self.name, run["order"], run["budgets"], c, what, "rows behind the steps run")
        return worst, tol


@pytest.fixture(scope="module", params=CASES, ids=["%s%d_%s" % (c[0], c[1], c[2].lower()) for c in CASES])
def launches(request, built_lib, oracle_mod, tmp_path_factory):
    return Launches(built_lib, tmp_path_factory.mktemp("persist_clips_" + request.param[0]), *request.param)


def test_ids_tell_the_clips_apart_and_equal_the_one_clip_ids(launches):
    """(d)"""
    s = launches.single
    assert s[0] != s[1] and s[1] != s[2] and s[0] != s[2]
    assert all(len(x) == launches.full for x in s), [len(x) for x in s]   # (benign weights: no eot; every budget is spent)
    for run in launches.runs:
        mc = run["budgets"] or [launches.full] * run["B"]
        assert run["ids"] == [s[i][: mc[c]] for c, i in enumerate(run["order"])], (launches.name, run["B"], run["order"], run["budgets"])


def test_whole_cache_against_the_oracle_and_the_inputs_discriminate(launches):
    """(a) and (b)"""
    worst = tol = 0.0
    for run in launches.runs:
        if run["budgets"] is None:
            w, t = launches.check_rows(run)
            worst, tol = max(worst, w), max(tol, t)
    assert tol > 0.0
    print("%s: worst |err| / tolerance %.3f (largest tolerance %.4f, A %.4f)" % (launches.name, worst, tol, launches.a))
    own = [launches.ref(i, launches.single[i]) for i in range(3)]
    sep_k, sep_v = prc.separation(launches.case.oracle_bf16, launches.kv, launches.single, own=own)
    print("%s: separation K %.3f V %.3f = %.1f x the largest tolerance (>= 8)" % (launches.name, sep_k, sep_v, min(sep_k, sep_v) / tol))
    assert min(sep_k, sep_v) >= 8 * tol, (launches.name, sep_k, sep_v, tol)


def test_cache_is_bit_identical_in_every_later_position(launches):
    """(c): "the same rows, same summation order" per clip (decode_persistent2.hip's header) — clip 1 of two, clip 1 of three,
    clip 2 of three hold the same bits for the same mel; where a case has one position only, nothing is compared across."""
    seen = {}
    for run in launches.runs:
        if run["budgets"] is None:
            for c, (gk, gv) in run["cache"].items():
                i = run["order"][c]
                n = len(run["ids"][c]) + 4
                seen.setdefault(i, []).append(((run["B"], c), gk[:, :n], gv[:, :n]))
    compared = 0
    for i, lst in seen.items():
        for pos, gk, gv in lst[1:]:
            compared += 1
            assert _bits_equal(gk, lst[0][1]) and _bits_equal(gv, lst[0][2]), (launches.name, "mel", i, "positions (clips, clip)", lst[0][0], pos,
                                                                              float(np.abs(gk - lst[0][1]).max()), float(np.abs(gv - lst[0][2]).max()))
    positions = sorted({p for lst in seen.values() for p, _, _ in lst})
    print("%s: bit-equal across positions %s: %d comparisons" % (launches.name, positions, compared))
    assert len(seen) == 3 and all(len(lst) == len(positions) for lst in seen.values())


def test_unequal_budgets(launches):
    """(e)"""
    worst, n = 0.0, 0
    for run in launches.runs:
        if run["budgets"] is not None:
            assert [len(x) for x in run["ids"]] == run["budgets"]
            w, _ = launches.check_rows(run)
            worst, n = max(worst, w), n + 1
    assert n == 2 * (len(launches.runs) // 5)   # two budget launches per launch size
    print("%s: unequal budgets, worst |err| / tolerance %.3f over %d launches" % (launches.name, worst, n))
