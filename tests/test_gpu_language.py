"""GPU: language detection and a language and task per clip (DESIGN.md "Language and task per clip") against tests/lang_reference.py.

1. The detection kernel alone (language_logprob_rows) against float64 from the same 16-bit weights: d 128, 256, 384, 1280, 99 and 100
   languages, 1 and 5 rows, benign / outlier-channel / equal-rows / NaN rows.
   Bound. The language logits are LayerNorm + dot, the arithmetic of the GEMV family's PRO_LAYERNORM GEPI_LOGITS launch, so the bound
   is tests/gemv_kernel_reference.py's: ea = ln_expect(two-pass), E_y = |W| ea + gamma_n |W| (|a| + ea), gamma_n over z_n + 7
   roundings (a lane's chain of at most K fused multiply-adds, 6 reduction steps; no bias here, so one to spare).
   lang_logprob[j] = x[j] - lse: logsumexp moves by at most the largest E_y (it is 1-Lipschitz in the maximum norm); in fp32 the sum
   of n_lang terms exp(x - m), each carrying the rounding of its argument (u |x - m| e^(x - m) <= 0.37 u), of expf (2 u) and of its
   addition (n_lang u in all), is relatively off by at most 4 n_lang u, logf adds 2 u and the two roundings of m + log s and of
   x - lse u (|lse| + |x[j]|) each at most:  E_lp[j] = E_y[j] + max_k E_y[k] + (4 n_lang + 8) u + 2 u (|x[j]| + |lse|).
2. Detection at stage level on both LangCase models, both routes: the measured logit error at most a quarter of the smallest kept
   margin, the index the oracle's, lang_logprob within 2 err + 1e-4 (the project's rule from "Confidence"), batches of 1, 3, all.
3. Explicit languages, one translate: ids against prompt_reference.greedy_prompted on [sot, language, task], self K/V rows 0..1.
4. Detect and decode in one call, one clip prompted with P = 61 (L = 64).
5. Long-form: two 45 s files that detect different languages, budget 8: the per-file language, every window's ids under it, the
   log without languages= unchanged.
6. Two engines on one GPU: bit-equal to one engine on the same blocks of clips, within 2 err + 1e-4 of one engine on all of them.
7. Refusals. 8. The zh text pass follows the clip's language."""
import os

import numpy as np
import pytest

import lang_reference as lr
import longform_reference as lfr
import prompt_reference as pr
from conftest import GOLDEN
from decode_kernel_reference import ln_expect
from encoder_kernel_reference import U32

pytestmark = pytest.mark.gpu

KV_BAR = 2e-2  # test_gpu_prompt.KV_BAR: self K/V after the prefill against the oracle's
BUDGET = 12
BUDGET_DETECT = 3  # test_detect_and_decode_in_one_call says why
BUDGET_LONG = 8
ROUTES = ("prefill", "step")


def make_engine(lib, model_type, root, route=None, max_batch=16, **kw):
    env = {"AX_WHISPER_PREFILL": route}
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        return lib.Whisper(model_type, root, "zh", max_batch=max_batch, **({"device": 0} if "devices" not in kw else {}), **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ------------------------------------------------------------------------------------------ 1. the kernel alone
KERNEL_MODELS = (("micro", "BF16", 128, 99), ("miniturbo", "F16", 256, 100), ("tiny", "BF16", 384, 99), ("w1280", "F16", 1280, 100))
TIE = (10, 40)  # two languages whose embedding rows are made equal


@pytest.fixture(scope="module", params=KERNEL_MODELS, ids=lambda p: "%s_%s" % (p[0], p[1].lower()))
def kernel_model(request, built_lib, tmp_path_factory):
    import modelgen

    model_type, dtype, d, n_lang = request.param
    dims = modelgen.DIMS[model_type]
    assert dims["d"] == d and dims["n_langs"] == n_lang
    w = modelgen.synth_weights(dims, 31, bf16=(dtype != "F16"))
    if dtype == "F16":
        w = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
    cfg = modelgen.make_config(model_type, dims)
    tok = lr.lang_tokens(cfg)
    emb = w["decoder.token_embedding.weight"].copy()
    emb[tok] = lr._round16(emb[tok] * np.float32(32.0), dtype)  # language logits of order 10, as a trained model's
    emb[tok[TIE[1]]] = emb[tok[TIE[0]]]
    w["decoder.token_embedding.weight"] = emb
    root = str(tmp_path_factory.mktemp("lang_kernel_" + model_type))
    modelgen.write_model_dir(root, model_type, dims, weights=w, dtype=dtype, tiktoken_path=os.path.join(GOLDEN, "multilingual.tiktoken"))
    e = make_engine(built_lib, model_type, root, max_batch=1)
    yield dict(e=e, d=d, n_lang=n_lang, W=emb[tok].astype(np.float64), g=w["decoder.ln.weight"], b=w["decoder.ln.bias"], zh=lr.lang_codes(cfg).index("zh"))
    e.close()


def kernel_expect(m, x):
    """float64 language logits and log-probs of rows x [n][d] with their per-element bounds."""
    y, ea, _ = ln_expect(x.astype(np.float64), m["g"], m["b"], onepass=False)
    W = m["W"]
    z = (W != 0).sum(1) + 7
    gamma = (z * U32 / (1 - z * U32))[None, :]
    ref = y @ W.T
    bound = ea @ np.abs(W).T + gamma * ((np.abs(y) + ea) @ np.abs(W).T) + 1e-300
    mx = ref.max(1, keepdims=True)
    lse = mx + np.log(np.exp(ref - mx).sum(1, keepdims=True))
    lp = ref - lse
    lp_bound = bound + bound.max(1, keepdims=True) + (4 * m["n_lang"] + 8) * U32 + 2 * U32 * (np.abs(ref) + np.abs(lse))
    return ref, bound, lp, lp_bound


def check_rows(m, x, what):
    lp, idx, lg = m["e"].language_logprob_rows(x)
    ref, bound, rlp, lp_bound = kernel_expect(m, x)
    worst = float((np.abs(lg - ref) / bound).max())
    worst_lp = float((np.abs(lp - rlp) / lp_bound).max())
    print("%s d %d n_lang %d rows %d: logit error %.3g of its bound (largest bound %.3g), log-prob error %.3g of its bound"
          % (what, m["d"], m["n_lang"], len(x), worst, float(bound.max()), worst_lp))
    assert worst <= 1.0 and worst_lp <= 1.0, (what, worst, worst_lp)
    for r in range(len(x)):
        assert idx[r] == int(np.argmax(lg[r])), (what, r)  # the first maximum of the kernel's own logits
        srt = np.sort(ref[r])
        if srt[-1] - srt[-2] > 2 * bound[r].max():
            assert idx[r] == int(np.argmax(ref[r])), (what, r)
    return lp, idx, lg


@pytest.mark.parametrize("rows", [1, 5])
def test_kernel_alone_against_float64(kernel_model, rows):
    m = kernel_model
    d = m["d"]
    rng = np.random.default_rng(100 + d + rows)
    benign = rng.standard_normal((rows, d)).astype(np.float32) * np.float32(3.0) + np.float32(0.5)
    check_rows(m, benign, "benign")
    out = benign.copy()
    out[:, 7 + (d // 2)] += np.float32(400.0)  # an outlier channel beyond the first 256 elements where the width has them
    out[rows - 1, 0] -= np.float32(300.0)      # ... and one row with its outlier in channel 0
    check_rows(m, out, "outlier")
    # a row along the two equal embedding rows: they are the maximum, the lower index wins, the two log-probs are bit-equal
    tie = benign.copy()
    tie[0] = (m["W"][TIE[0]] / m["g"].astype(np.float64) * 50.0).astype(np.float32)
    lp, idx, lg = check_rows(m, tie, "tie")
    assert idx[0] == TIE[0] and lg[0, TIE[0]] == lg[0, TIE[1]] and lp[0, TIE[0]].tobytes() == lp[0, TIE[1]].tobytes()
    assert lg[0, TIE[0]] == lg[0].max()
    # a row containing NaN: every logit is NaN -> the handle's language, all -inf; the other rows are untouched by it
    bad = benign.copy()
    bad[0, 5] = np.nan
    lp, idx, lg = m["e"].language_logprob_rows(bad)
    assert idx[0] == m["zh"] and np.isneginf(lp[0]).all() and np.isnan(lg[0]).all()
    if rows > 1:
        lp_ok, idx_ok, lg_ok = m["e"].language_logprob_rows(benign)
        assert np.array_equal(lp[1:], lp_ok[1:]) and np.array_equal(idx[1:], idx_ok[1:])
    # nothing finite although not everything is NaN (an infinite input: the LayerNorm's mean is inf, inf - inf is NaN, and whatever
    # the products make of it is NaN or an infinity): the kernel's answer is lang_reference.pick's on the kernel's own logits
    for val in (np.inf, -np.inf):
        bad = benign.copy()
        bad[0, 9] = val
        lp, idx, lg = m["e"].language_logprob_rows(bad)
        assert not np.isfinite(lg[0]).any()
        want_idx, want_lp = lr.pick(lg[0], m["zh"])
        assert idx[0] == want_idx == m["zh"] and np.array_equal(lp[0], want_lp) and np.isneginf(lp[0]).all()


# ------------------------------------------------------------------------------------------ 2 - 7: LangCase models
class Model:
    def __init__(self, lib, tmp, model_type, seed, dtype):
        self.lib = lib
        self.case = lr.LangCase(model_type, seed, dtype)
        self.root = self.case.write(tmp)
        self.cfg, self.orc = self.case.cfg, self.case.oracle
        self.kept = self.case.kept()
        self.ex = {i: self.case.expect(i) for i in self.kept}
        self.min_margin = min(self.ex[i]["margin"] for i in self.kept)
        self.clips = self.case.clips()
        self.engines = {}
        self.err = {}  # route -> the largest stage-level logit error measured over the kept clips
        self._decode = {}

    def engine(self, route=None, **kw):
        key = (route, tuple(sorted(kw.items(), key=str)))
        if key not in self.engines:
            self.engines[key] = make_engine(self.lib, self.case.model_type, self.root, route, **kw)
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()

    def oracle_ids(self, i, lang_index, task=0, prompt=(), budget=BUDGET):
        """(ids, smallest decision margin, (self_k, self_v)) of the oracle on clip i under a language, a task and a prompt."""
        key = (i, lang_index, task, tuple(prompt), budget)
        if key not in self._decode:
            e = self.case.expect(i)
            ids, infos, (sk, sv, _) = pr.greedy_prompted(self.orc, e["ck"], e["cv"], lr.context(self.cfg, prompt, lang_index, task), max_new=budget,
                                                         want_cache=True)
            self._decode[key] = (ids, min(x["margin"] for x in infos), (sk, sv))
        return self._decode[key]


@pytest.fixture(scope="module", params=lr.MODELS, ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("lang_" + request.param[0]), *request.param)
    yield m
    m.close()


def test_language_index_and_code_against_the_config(model):
    e = model.engine()
    codes = lr.lang_codes(model.cfg)
    assert e.n_lang == len(codes) == model.case.n_lang
    for j, c in enumerate(codes):
        assert e.language_index(c) == j and e.language_code(j) == c
    assert e.language_index("xx") == -1 and e.language_code(-1) is None and e.language_code(len(codes)) is None
    assert e.get_config_int("lang_index") == codes.index("zh")


def stage_error(model, route):
    """The largest |lang_logit_gpu - lang_logit_oracle| over the kept clips, all of them in one batch (measured once per route)."""
    if route not in model.err:
        e = model.engine(route)
        e.encode_mel(np.stack([model.ex[i]["mel"] for i in model.kept]))
        lg = e.detect_language_stage(len(model.kept))[2]
        model.err[route] = max(float(np.abs(lg[b] - model.ex[i]["lang_logit"]).max()) for b, i in enumerate(model.kept))
    return model.err[route]


@pytest.mark.parametrize("route", ROUTES)
def test_detection_at_stage_level(model, route):
    """Measured on MI355X, largest logit error over the kept clips / smallest kept margin (the bar is a quarter):
        micro bf16      0.070 / 0.501 = 0.14      miniturbo fp16  0.018 / 0.717 = 0.026      on both routes
    (both take the [sot] position through the layers of one decoder step; the prefill route picks in language_detect_kernel from the
    residual rows, the step-fed route on the host from the dumped logits rows). A one-row prefill pass in front of the kernel, which
    stores attention outputs in 16 bits, measured 1.51 and 0.35 here and was replaced: DESIGN.md "Language and task per clip"."""
    e = model.engine(route)
    kept, ex = model.kept, model.ex
    alone = {}
    worst = 0.0
    for size in (1, 3, len(kept)):
        groups = [kept[k:k + size] for k in range(0, len(kept), size)] if size < len(kept) else [kept]
        if size == 3:
            groups = [g for g in groups if len(g) == 3][:2]
        for g in groups:
            e.encode_mel(np.stack([ex[i]["mel"] for i in g]))
            idx, lp, lg = e.detect_language_stage(len(g))
            for b, i in enumerate(g):
                err = float(np.abs(lg[b] - ex[i]["lang_logit"]).max())
                worst = max(worst, err)
                print("%s %s clip %d in a batch of %d: logit err %.3g, margin %.3g, index %d (oracle %d)"
                      % (model.case.model_type, route, i, len(g), err, ex[i]["margin"], idx[b], ex[i]["index"]))
                assert idx[b] == ex[i]["index"], (route, i, len(g))
                assert np.abs(lp[b] - ex[i]["lang_logprob"]).max() <= 2 * err + 1e-4, (route, i, len(g), err)
                if size == 1:
                    alone[i] = (int(idx[b]), lp[b].copy(), err)
                else:  # a clip alone and inside a batch: the same index, the log-probs within the same bound
                    assert idx[b] == alone[i][0]
                    assert np.abs(lp[b] - alone[i][1]).max() <= 2 * err + 1e-4, (route, i, len(g), err)
    print("%s %s: largest |lang_logit_gpu - lang_logit_oracle| over the kept clips %.3g, smallest kept margin %.3g (ratio %.3g)"
          % (model.case.model_type, route, worst, model.min_margin, worst / model.min_margin))
    assert worst <= model.min_margin / 4


def test_routes_agree_on_the_index(model):
    a, b = model.engine("prefill"), model.engine("step")
    mels = np.stack([model.ex[i]["mel"] for i in model.kept])
    a.encode_mel(mels)
    ia = a.detect_language_stage(len(model.kept))[0]
    b.encode_mel(mels)
    ib = b.detect_language_stage(len(model.kept))[0]
    assert ia.tolist() == ib.tolist() == [model.ex[i]["index"] for i in model.kept]


def explicit_cases(model):
    """Four (clip, language, task) with four different languages, one of them translate, whose oracle decisions keep
    prompt_reference.MARGIN over the budget (as find_case selects)."""
    out, used = [], set()
    zh = model.case.handle_index
    for i in model.kept:
        task = 1 if len(out) == 2 else 0
        for j in range(model.case.n_lang):
            if j == zh or j in used:
                continue
            if model.oracle_ids(i, j, task)[1] >= pr.MARGIN:
                out.append((i, j, task))
                used.add(j)
                break
        if len(out) == 4:
            return out
    raise AssertionError("too few (clip, language) pairs keep the margin")


@pytest.mark.parametrize("route", ROUTES)
def test_explicit_languages(model, route):
    e = model.engine(route)
    cases = explicit_cases(model)
    codes = lr.lang_codes(model.cfg)
    clips = [model.clips[i] for i, _, _ in cases]
    langs = [codes[j] for _, j, _ in cases]
    tasks = ["translate" if t else "transcribe" for _, _, t in cases]
    got = e.run_timestamp_lang_batch(clips, languages=langs, tasks=tasks, max_new=BUDGET)
    for (i, j, t), o in zip(cases, got):
        want = model.oracle_ids(i, j, t)[0]
        print("%s clip %d language %s task %d: ids %s" % (route, i, codes[j], t, o["ids"]))
        assert o["ids"] == want and o["language"] == codes[j], (route, i, j, t, o["ids"], want)
        assert "lang_logprob" not in o and np.isfinite(o["token_logprob"]).all() and np.isfinite(o["no_speech_logprob"])
    # the cached context rows [sot, language] against the oracle's cache
    e.encode_mel(np.stack([model.ex[i]["mel"] for i, _, _ in cases]))
    _, lout, _ = e.prefill_contexts(4, languages=langs, tasks=tasks)
    assert lout.tolist() == [j for _, j, _ in cases]
    for b, (i, j, t) in enumerate(cases):
        sk, sv = model.oracle_ids(i, j, t)[2]
        k, v = e.get_self_kv(b, 2)
        dk, dv = float(np.abs(k - sk[:, :2]).max()), float(np.abs(v - sv[:, :2]).max())
        print("%s clip %d: self K err %.3g, V err %.3g" % (route, i, dk, dv))
        assert dk < KV_BAR and dv < KV_BAR
    # the handle's own language given explicitly, beside clips that force a context: the unprompted call's ids, scores included
    langs0 = ["zh"] + langs[1:]
    tasks0 = ["transcribe"] + tasks[1:]
    beside = e.run_timestamp_lang_batch(clips, languages=langs0, tasks=tasks0, max_new=BUDGET)
    plain = e.run_timestamp_tokens_batch(clips, max_new=BUDGET)
    scored = e.run_timestamp_scores_batch(clips, max_new=BUDGET)
    assert beside[0]["ids"] == plain[0] and beside[0]["language"] == "zh"
    assert np.array_equal(beside[0]["token_logprob"], scored[0]["token_logprob"]) and beside[0]["no_speech_logprob"] == scored[0]["no_speech_logprob"]
    for b in range(1, 4):
        assert beside[b]["ids"] == got[b]["ids"]
    # nothing asked: the unprompted call, clip for clip
    none = e.run_timestamp_lang_batch(clips, max_new=BUDGET)
    for a, b in zip(none, scored):
        assert a["ids"] == b["ids"] and np.array_equal(a["token_logprob"], b["token_logprob"]) and a["language"] == "zh"


@pytest.mark.parametrize("route", ROUTES)
def test_detect_and_decode_in_one_call(model, route):
    """Budget: 3 ids (four decisions). The text logits of a LangCase model barely move with the language (the coordinates that carry
    it reach no other logit), so over 12 decisions no micro clip and three miniturbo clips keep prompt_reference.MARGIN under their
    detected language; over four decisions five and more do, with at least three languages among them. What is under test here is the
    hand-over behind a detected language — the patched context row, the offset, the task id — and the first decision already depends
    on all of it."""
    e = model.engine(route)
    codes = lr.lang_codes(model.cfg)
    sel = [i for i in model.kept if model.oracle_ids(i, model.ex[i]["index"], budget=BUDGET_DETECT)[1] >= pr.MARGIN]
    assert len(sel) >= 4 and len({model.ex[i]["index"] for i in sel}) >= 3, sel
    got = e.run_timestamp_lang_batch([model.clips[i] for i in sel], languages=["auto"] * len(sel), max_new=BUDGET_DETECT)
    for i, o in zip(sel, got):
        assert o["language"] == codes[model.ex[i]["index"]], (route, i, o["language"])
        assert o["ids"] == model.oracle_ids(i, model.ex[i]["index"], budget=BUDGET_DETECT)[0], (route, i)
        assert len(o["token_logprob"]) == len(o["ids"]) + 1 and np.isfinite(o["token_logprob"]).all() and np.isfinite(o["no_speech_logprob"])
        assert int(np.argmax(o["lang_logprob"])) == model.ex[i]["index"]
    # one clip prompted AND detecting, P = 61: L = 64, a key-block edge; beside it a clip that only detects and one left alone
    E = int(model.cfg["eot"])
    i = next(i for i in sel if model.ex[i]["index"] != model.case.handle_index)
    prompt = next(p for p in (pr.case_prompt(E, 61, sd) for sd in range(32))
                  if model.oracle_ids(i, model.ex[i]["index"], 0, p, budget=BUDGET_DETECT)[1] >= pr.MARGIN)
    other = next(k for k in sel if k != i)
    three = e.run_timestamp_lang_batch([model.clips[i], model.clips[other], model.clips[other]], languages=["auto", "auto", None],
                                       prompts=[prompt, [], []], max_new=BUDGET_DETECT)
    assert three[0]["language"] == codes[model.ex[i]["index"]]
    assert three[0]["ids"] == model.oracle_ids(i, model.ex[i]["index"], 0, prompt, budget=BUDGET_DETECT)[0]
    assert three[1]["language"] == codes[model.ex[other]["index"]]
    assert three[1]["ids"] == model.oracle_ids(other, model.ex[other]["index"], budget=BUDGET_DETECT)[0]
    assert three[2]["language"] == "zh" and three[2]["ids"] == e.run_timestamp_tokens_batch([model.clips[other]] * 3, max_new=BUDGET_DETECT)[2]
    # detection alone, from PCM, against the stage-level call on the engine's own log-mel of the same three clips: the oracle's
    # index, the log-probs within 2 err + 1e-4 with err the clip's logit error measured at that stage-level call
    det = e.detect_language([model.clips[k] for k in sel[:3]])
    e.encode_mel(np.stack([e.compute_mel(model.clips[k]) for k in sel[:3]]))
    _, slp, slg = e.detect_language_stage(3)
    for b, (k, (code, lp)) in enumerate(zip(sel[:3], det)):
        err = float(np.abs(slg[b] - model.ex[k]["lang_logit"]).max())
        assert code == codes[model.ex[k]["index"]] and np.abs(lp - slp[b]).max() <= 2 * err + 1e-4, (route, k, err)


def test_two_engines_on_one_gpu(model):
    """Sharded results against the one-engine results: six clips, three per engine. Against one engine on the same two blocks of
    three (the same batch composition): bit-equal. Against one engine on all six: the same language and ids, the log-probs within
    2 err + 1e-4, err the clip's logit error against the oracle measured on that engine."""
    old = os.environ.get("AX_WHISPER_ALLOW_DUPLICATE_DEVICES")
    os.environ["AX_WHISPER_ALLOW_DUPLICATE_DEVICES"] = "1"
    try:
        two = model.engine(None, devices=(0, 0), max_batch=4)
    finally:
        os.environ.pop("AX_WHISPER_ALLOW_DUPLICATE_DEVICES") if old is None else os.environ.__setitem__("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", old)
    assert two.n_devices == 2
    one = model.engine(None)
    sel = model.kept[:6]
    clips = [model.clips[i] for i in sel]
    a, b = two.detect_language(clips), one.detect_language(clips)
    blocks = one.detect_language(clips[:3]) + one.detect_language(clips[3:])
    one.encode_mel(np.stack([model.ex[i]["mel"] for i in sel]))
    lg = one.detect_language_stage(6)[2]
    for k, (i, (ca, la), (cb, lb), (cc, lc)) in enumerate(zip(sel, a, b, blocks)):
        err = float(np.abs(lg[k] - model.ex[i]["lang_logit"]).max())
        print("%s clip %d: sharded against one engine %.3g (err %.3g)" % (model.case.model_type, i, float(np.abs(la - lb).max()), err))
        assert ca == cc and la.tobytes() == lc.tobytes(), i
        assert ca == cb and np.abs(la - lb).max() <= 2 * err + 1e-4, (i, err)
    langs = ["auto", "en", None, "auto", "de", "auto"]
    tasks = ["transcribe", "translate", "transcribe", "transcribe", "transcribe", "translate"]
    ga = two.run_timestamp_lang_batch(clips, languages=langs, tasks=tasks, max_new=BUDGET_DETECT)
    gb = one.run_timestamp_lang_batch(clips, languages=langs, tasks=tasks, max_new=BUDGET_DETECT)
    gc = one.run_timestamp_lang_batch(clips[:3], languages=langs[:3], tasks=tasks[:3], max_new=BUDGET_DETECT) + \
        one.run_timestamp_lang_batch(clips[3:], languages=langs[3:], tasks=tasks[3:], max_new=BUDGET_DETECT)
    for x, y, z in zip(ga, gb, gc):
        assert x["language"] == y["language"] == z["language"] and x["ids"] == y["ids"] == z["ids"]
        assert np.array_equal(x["token_logprob"], z["token_logprob"]) and x["no_speech_logprob"] == z["no_speech_logprob"]
        assert ("lang_logprob" in x) == ("lang_logprob" in z) and ("lang_logprob" not in x or x["lang_logprob"].tobytes() == z["lang_logprob"].tobytes())
    # long-form: the files are split, the per-file language travels with them
    files, want = long_files(model)
    l2, c2 = two.run_long_windows(files, max_new=BUDGET_LONG, languages=["auto", "auto"])
    l1, c1 = one.run_long_windows(files, max_new=BUDGET_LONG, languages=["auto", "auto"])
    assert c2 == c1 == [lr.lang_codes(model.cfg)[j] for j in want]
    assert [[w[:4] for w in f] for f in l2] == [[w[:4] for w in f] for f in l1]


def test_refusals_leave_the_handle_usable(model, built_lib, tmp_path):
    import modelgen

    e = model.engine(None)
    clip = [model.clips[model.kept[0]]]
    want = e.detect_language(clip)[0][0]

    def refused(fn, *words):
        with pytest.raises(RuntimeError) as r:
            fn()
        assert any(w in str(r.value) for w in words), str(r.value)
        assert e.detect_language(clip)[0][0] == want  # the handle is usable

    n = e.n_lang
    refused(lambda: e.run_timestamp_lang_batch(clip, languages=[n]), "outside")
    refused(lambda: e.run_timestamp_lang_batch(clip, languages=[-3]), "outside")
    e.encode_mel(model.ex[model.kept[0]]["mel"])
    refused(lambda: e.prefill_contexts(1, languages=[n + 5]), "outside")
    refused(lambda: e.decode_forced_timestamp_lang(np.zeros((1, 0), dtype=np.int32), languages=[-7]), "outside")
    # a task outside 0 / 1 (an integer goes to the C ABI as it is)
    refused(lambda: e.run_timestamp_lang_batch(clip, tasks=[2]), "neither 0")
    refused(lambda: e.run_timestamp_lang_batch(clip, tasks=[-1]), "neither 0")
    refused(lambda: e.prefill_contexts(1, tasks=[5]), "neither 0")
    # long-form: the same refusals, per file
    refused(lambda: e.run_long_windows(clip, max_new=2, languages=[n]), "outside")
    refused(lambda: e.run_long_windows(clip, max_new=2, tasks=[3]), "neither 0")
    refused(lambda: e.run_long_text(clip[0], languages=[-9]), "outside")
    # an open Stream* session
    e.stream_open(2)
    try:
        for fn in (lambda: e.run_timestamp_lang_batch(clip, languages=["auto"]), lambda: e.detect_language(clip), lambda: e.detect_language_stage(1)):
            with pytest.raises(RuntimeError) as r:
                fn()
            assert "stream" in str(r.value).lower(), str(r.value)
    finally:
        e.stream_close()
    assert e.detect_language(clip)[0][0] == want
    # translate on a config without a translate id inside the vocabulary
    import json
    import shutil

    src = os.path.join(model.root, model.case.model_type)
    dst = tmp_path / "no_translate" / model.case.model_type
    shutil.copytree(src, str(dst))
    cfg_file = next(f for f in os.listdir(str(dst)) if f.endswith("_config.json"))
    with open(str(dst / cfg_file)) as f:
        cfg = json.load(f)
    cfg["translate"] = -1
    with open(str(dst / cfg_file), "w") as f:
        json.dump(cfg, f)
    e0 = built_lib.Whisper(model.case.model_type, str(tmp_path / "no_translate"), "zh", device=0, max_batch=1)
    try:
        with pytest.raises(RuntimeError) as r:
            e0.run_timestamp_lang_batch(clip, tasks=["translate"], max_new=2)
        assert "translate" in str(r.value)
        with pytest.raises(RuntimeError) as r:
            e0.run_long_windows(clip, max_new=2, tasks=["translate"])
        assert "translate" in str(r.value)
        assert e0.run_timestamp_lang_batch(clip, languages=["auto"], max_new=2)[0]["language"] == want  # still usable
    finally:
        e0.close()
    # detection on a one-language config (a micro model with one language and the vocabulary that goes with it)
    dims = dict(modelgen.DIMS["micro"], n_langs=1, n_vocab=51865 - 98)
    modelgen.DIMS["micro1"] = dims
    try:
        modelgen.write_model_dir(str(tmp_path), "micro1", dims, seed=3, tiktoken_path=os.path.join(GOLDEN, "multilingual.tiktoken"))
        e1 = built_lib.Whisper("micro1", str(tmp_path), "zh", device=0, max_batch=1)
    finally:
        del modelgen.DIMS["micro1"]
    try:
        assert e1.n_lang == 1
        with pytest.raises(RuntimeError) as r:
            e1.detect_language(clip)
        assert "more than one language" in str(r.value)
        with pytest.raises(RuntimeError) as r:
            e1.run_timestamp_lang_batch(clip, languages=["auto"])
        assert "more than one language" in str(r.value)
        with pytest.raises(RuntimeError) as r:
            e1.run_long_windows(clip, max_new=2, languages=["auto"])
        assert "more than one language" in str(r.value)
        out = e1.run_timestamp_lang_batch(clip, languages=[0], tasks=["translate"], max_new=4)  # still usable: its one language, translate
        assert out[0]["language"] == e1.language_code(0)
    finally:
        e1.close()


# ------------------------------------------------------------------------------------------ 5. long-form
def long_files(model):
    """Two 45 s files, each a kept clip repeated, whose windows at seek 0 detect different languages on the oracle with
    lang_reference.MARGIN to spare -> (files, [language index per file]). The window is the whole-file front-end's (one maximum
    over the file), so it is detected on its own, not taken from the clip's result. Computed once per model."""
    if not hasattr(model, "_long"):
        n = 45 * 16000
        files, want, norms = [], [], []
        for i in model.kept:
            c = model.clips[i]
            pcm = np.tile(c, n // len(c) + 1)[:n].astype(np.float32)
            norm = lfr.file_log_mel(pcm, model.case.dims["n_mels"])[0]
            ck, cv = model.orc.encoder(lfr.window_of(norm, 0))
            idx, _, lg = lr.detect(model.orc, ck, cv, model.case.handle_index)
            top = np.sort(lg)
            if top[-1] - top[-2] < lr.MARGIN or idx in want:
                continue
            files.append(pcm); want.append(idx); norms.append(norm)
            if len(files) == 2:
                break
        assert len(files) == 2, "too few files detect different languages with the margin"
        model._long = (files, want, norms)
    return model._long[0], model._long[1]


def check_long_log(model, e, pcm, norm, log, lang_index):
    """One file's log, window by window: the seek chain and the ids of the oracle under the file's language (a differing id is
    excused only as a measured tie: the oracle's margin at that step below 2 err + 1e-4, err the logit error at that step; the chain
    goes on from the engine's own ids)."""
    T, E = int(model.cfg["no_timestamps"]) + 1, int(model.cfg["eot"])
    seek = 0
    for w in log:
        s, wf, adv, ids = w[:4]
        assert s == seek and wf == min(3000, len(pcm) // 160 - s)
        ck, cv = model.orc.encoder(lfr.window_of(norm, s))
        want, infos, rows = pr.greedy_prompted(model.orc, ck, cv, lr.context(model.cfg, (), lang_index, 0), max_new=BUDGET_LONG, want_logits=True)
        if ids != want:
            i = next((i for i in range(min(len(ids), len(want))) if ids[i] != want[i]), min(len(ids), len(want)))
            e.encode_mel(lfr.window_of(norm, s))
            lg = e.decode_forced_timestamp_lang(np.array([want[:i]], dtype=np.int32).reshape(1, i), languages=[lang_index])[0]
            err = float(np.abs(lg[0, i] - rows[i]).max())
            assert infos[i]["margin"] < 2 * err + 1e-4, ("seek", s, "step", i, infos[i], err, want, ids)
        assert not w[8] and w[-1] == 0  # nothing skipped, nothing prompted
        assert adv == lfr.split_window(ids, T, E, wf)[1]
        seek += adv
    assert seek == len(pcm) // 160 and len(log) >= 2


@pytest.mark.parametrize("route", ROUTES)
def test_long_form_language_per_file(model, route):
    e = model.engine(route)
    codes = lr.lang_codes(model.cfg)
    files, want = long_files(model)
    norms = model._long[2]
    assert want[0] != want[1]
    before = e.run_long_windows(files, max_new=BUDGET_LONG, scores=True)
    logs, langs = e.run_long_windows(files, max_new=BUDGET_LONG, languages=["auto", "auto"])
    print("%s %s: files detect %s (oracle %s), windows %s" % (model.case.model_type, route, langs, [codes[j] for j in want], [len(l) for l in logs]))
    assert langs == [codes[j] for j in want]
    for f in range(2):
        check_long_log(model, e, files[f], norms[f], logs[f], want[f])
    # the detected language given explicitly, and one file alone: the same windows (the language is the file's, not the call's)
    explicit, lang2 = e.run_long_windows(files, max_new=BUDGET_LONG, languages=[codes[want[0]], "auto"])
    assert lang2 == langs and [[w[:4] for w in l] for l in explicit] == [[w[:4] for w in l] for l in logs]
    alone, lang1 = e.run_long_windows(files[1:], max_new=BUDGET_LONG, languages=["auto"])
    assert lang1 == langs[1:]
    if [w[:4] for w in alone[0]] != [w[:4] for w in logs[1]]:  # (ties apart: the log alone follows the rule too)
        check_long_log(model, e, files[1], norms[1], alone[0], want[1])
    # translate is fed: the first window's ids are the oracle's under [sot, language, translate]
    tr, _ = e.run_long_windows(files[:1], max_new=BUDGET_LONG, max_passes=1, languages=["auto"], tasks=["translate"])
    ck, cv = model.orc.encoder(lfr.window_of(norms[0], 0))
    wt, infos, rows = pr.greedy_prompted(model.orc, ck, cv, lr.context(model.cfg, (), want[0], 1), max_new=BUDGET_LONG, want_logits=True)
    if tr[0][0][3] != wt:
        i = next((i for i in range(min(len(tr[0][0][3]), len(wt))) if tr[0][0][3][i] != wt[i]), min(len(tr[0][0][3]), len(wt)))
        e.encode_mel(lfr.window_of(norms[0], 0))
        lg = e.decode_forced_timestamp_lang(np.array([wt[:i]], dtype=np.int32).reshape(1, i), languages=[want[0]], tasks=["translate"])[0]
        assert infos[i]["margin"] < 2 * float(np.abs(lg[0, i] - rows[i]).max()) + 1e-4
    # without languages= the log is what it was, before and after; through the new entry point with nothing asked, too
    after = e.run_long_windows(files, max_new=BUDGET_LONG, scores=True)
    assert after == before
    nothing, lang0 = e.run_long_windows(files, max_new=BUDGET_LONG, languages=[None, None])
    assert lang0 == ["zh", "zh"] and [[w[:9] for w in l] for l in nothing] == before
    assert [[w[:6] for w in l] for l in before] == e.run_long_windows(files, max_new=BUDGET_LONG)
    # text: the whole text is the segments' text under the file's language
    text = e.run_long_text(files[1][: 12 * 16000], languages=["auto"])
    segs, code = e.run_long_scored(files[1][: 12 * 16000], languages=["auto"])
    assert isinstance(text, str) and text == "".join(s[2] for s in segs) and code in codes


# ------------------------------------------------------------------------------------------ 8. text follows the clip's language
def test_zh_text_pass_follows_the_clips_language(model, built_lib, tmp_path, monkeypatch):
    """A handle whose language is en: the text of ids decoded under zh goes through the Traditional-to-Simplified pass (the
    dictionaries are looked for when the first zh text arrives), under any other language, and through Transcript, it does not."""
    import base64

    from test_t2s import opencc_t2s_dir

    monkeypatch.setenv("AX_WHISPER_OPENCC_DIR", os.path.dirname(opencc_t2s_dir(str(tmp_path))))
    rank = {}
    with open(os.path.join(GOLDEN, "multilingual.tiktoken"), "rb") as f:
        for line in f:
            if line.strip():
                b, r = line.split()
                rank[base64.b64decode(b)] = int(r)
    trad, simp = "甚至出現交易幾乎停止的情況", "甚至出现交易几乎停止的情况"
    ids = [rank[bytes([c])] for c in trad.encode()]
    e = built_lib.Whisper(model.case.model_type, model.root, "en", device=0, max_batch=1)
    try:
        assert e.get_config_int("t2s") == 0 and e.transcript(ids) == trad
        assert e.transcript_lang(ids, "en") == trad and e.transcript_lang(ids, "ja") == trad
        assert e.transcript_lang(ids, "zh") == simp
    finally:
        e.close()


def test_cli_detect_language_and_task(model, built_lib, tmp_path):
    """whisper_cli --detect_language / --task with --timestamps and with --long: the Detected language: line in front of Result:,
    with the code and probability of detect_language on the same samples, and the text of the call under that language."""
    import re
    import subprocess
    import wave

    e = model.engine(None)
    i = next(k for k in model.kept if model.ex[k]["index"] != model.case.handle_index)
    pcm16 = np.clip(np.round(model.clips[i] * 32768.0), -32768, 32767).astype(np.int16)
    wav = str(tmp_path / "clip.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm16.tobytes())
    pcm = pcm16.astype(np.float32) / np.float32(32768.0)
    code, lp = e.detect_language([pcm])[0]
    assert code == lr.lang_codes(model.cfg)[model.ex[i]["index"]]
    cli = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_cli")
    args = [cli, "-w", wav, "-t", model.case.model_type, "-p", model.root, "--language", "zh"]
    for mode in ("--timestamps", "--long"):
        r = subprocess.run(args + [mode, "--detect_language", "--task", "translate"], capture_output=True, timeout=120)
        out = r.stdout.decode("utf-8", "replace")
        assert r.returncode == 0, (out[-400:], r.stderr[-400:])
        m = re.search(r"(?m)^Detected language: (\S+) \(p = ([0-9.]+)\)\n", out)
        assert m and m.group(1) == code and abs(float(m.group(2)) - float(np.exp(lp.max()))) < 1e-3, out[-400:]
        assert m.end() <= out.index("Result: ")
        if mode == "--timestamps":
            got = e.run_timestamp_lang_batch([pcm], languages=[code], tasks=["translate"])[0]
            text = e.transcript_lang([t for t in got["ids"] if t < int(model.cfg["eot"])], code)
        else:
            text = e.run_long_text(pcm, languages=[code], tasks=["translate"])
        assert out[out.index("Result: ") + 8:].startswith(text + "\n"), (mode, out[-400:])
