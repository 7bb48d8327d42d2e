"""GPU: the slot stream in the scored timestamp mode (DESIGN.md "Slot stream in timestamp mode"): AX_WHISPER_StreamOpenMode(mode 1),
a language and task per slot, detection inside the step, scores per slot.

A  stream_rules_kernel alone (AX_WHISPER_StreamRulesStage) on rows of the 99- and the 100-language vocabulary, 1 and 5 slots
B  32 clips through 8 slots against the batched scored call, the stand-alone runs and score_reference on the oracle's rows
C  a language and task per slot on the lang_reference.LangCase model, detection included
D  72 slots (three graph branches, the vocabulary projection as two launches)
E  one and two slots, a clip that runs to the end of the context, a slot reused six times
F  stale state: three clips through ONE slot (detect, then the handle's language, then an explicit language and translate)
G  the fp16 build and the d_model 1280 step sequence
H  the refusals, each of which leaves a running slot intact; a mode-0 stream opened through StreamOpenMode

Ties. conftest.assert_ids_equal_or_tie teacher-forces behind the plain prefix, which timestamp-mode ids do not follow; the same rule
is restated here for them (equal_or_tie): where the engine's ids leave the oracle's, the oracle's own decision margin at that step must
be below twice the logit error measured at that very step + 1e-4."""
import numpy as np
import pytest

import lang_reference as lr
import prompt_reference as pr
import score_reference as sr
from conftest import GOLDEN, ModelCase
from encoder_kernel_reference import U32

pytestmark = pytest.mark.gpu


def _clips_and_budgets(n):
    """test_gpu_stream.py's clips and budgets (20 .. 140, no order)."""
    import modelgen

    lens = [480000, 200000, 77777, 480000, 123457, 16000, 300000, 480000]
    clips = [modelgen.synth_clip(40 + i, lens[i % len(lens)]) for i in range(n)]
    budgets = [20 + (37 * i) % 121 for i in range(n)]
    return clips, budgets


def _ctx(cfg, lang_code="zh", task=0):
    return lr.context(cfg, [], lr.lang_codes(cfg).index(lang_code), task)


def equal_or_tie(e, orc, cfg, mel, got, budget, lang_code=None, task=0, what=""):
    """True: `got` are the oracle's ids behind [sot, language, task]. False: they leave them at a numerical tie. Anything else fails."""
    ck, cv = orc.encoder(mel)
    ids, infos, rows = pr.greedy_prompted(orc, ck, cv, _ctx(cfg, lang_code or "zh", task), max_new=budget, want_logits=True)
    n = min(len(ids), len(got))
    if list(got[:n]) == list(ids[:n]):
        assert len(got) == len(ids), (what, len(got), len(ids))
        return True
    i = next(i for i in range(n) if ids[i] != got[i])
    e.encode_mel(np.stack([mel] * 3))  # the clip-block step sequence, as in the stream
    f = np.array([list(ids[:i])] * 3, dtype=np.int32).reshape(3, i)
    if lang_code is None and task == 0:
        logits = e.decode_forced_timestamp_scores(3, f, want_logits0=False)[0]
    else:
        logits = e.decode_forced_timestamp_lang(f, languages=[lang_code] * 3, tasks=[task] * 3)[0]
    err = float(np.abs(logits[0, i] - rows[i]).max())
    assert infos[i]["margin"] < 2 * err + 1e-4, (what, "step", i, "margin", infos[i]["margin"], "logit err", err, list(ids), list(got))
    return False


# ------------------------------------------------------------------------------------------ A. the rules kernel alone
@pytest.fixture(scope="module", params=[("micro", "BF16", 99), ("miniturbo", "F16", 100)], ids=["99_languages", "100_languages"])
def rules_model(request, built_lib, tmp_path_factory):
    import modelgen

    model_type, dtype, n_lang = request.param
    dims = modelgen.DIMS[model_type]
    assert dims["n_langs"] == n_lang
    w = modelgen.synth_weights(dims, 5, bf16=(dtype != "F16"))
    if dtype == "F16":
        w = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
    cfg = modelgen.make_config(model_type, dims)
    root = str(tmp_path_factory.mktemp("stream_rules_" + model_type))
    modelgen.write_model_dir(root, model_type, dims, weights=w, dtype=dtype, tiktoken_path=__import__("os").path.join(GOLDEN, "multilingual.tiktoken"))
    e = built_lib.Whisper(model_type, root, "zh", device=0, max_batch=1)
    yield dict(e=e, cfg=cfg, tok=lr.lang_tokens(cfg), zh=lr.lang_codes(cfg).index("zh"), n_lang=n_lang)
    e.close()


S, SI = -7.0, -7  # Whisper.stream_rules_stage's sentinels
CTX0 = [11, 22, 33, 44]


def _untouched(o, b, what):
    assert o["chosen"][b] == SI and o["logprob"][b] == np.float32(S), (what, b)
    assert o["no_speech"][b] == np.float32(S) and o["lang_out"][b] == SI and (o["lang_logprob"][b] == np.float32(S)).all(), (what, b)
    assert o["slot_ctx"][b].tolist() == CTX0, (what, b)


def _check_detect(m, o, b, row, ns_want, what):
    tok, n_lang = m["tok"], m["n_lang"]
    lg = row[tok]
    want, want_lp = lr.pick(lg, m["zh"])
    assert o["lang_out"][b] == want, (what, b, int(o["lang_out"][b]), want)
    assert o["slot_ctx"][b].tolist() == [CTX0[0], tok[want], CTX0[2], CTX0[3]], (what, b)
    assert o["no_speech"][b].tobytes() == ns_want.tobytes(), (what, b)
    assert o["chosen"][b] == SI and o["logprob"][b] == np.float32(S), (what, b)
    got = o["lang_logprob"][b]
    fin = np.isfinite(want_lp)
    assert np.array_equal(got[~fin], want_lp[~fin]), (what, b)  # -inf for NaN and -inf entries, everywhere when nothing is finite
    if fin.any():
        x = lg.astype(np.float64)
        ok = ~np.isnan(x)
        mx = x[ok].max()
        lse = mx + np.log(np.exp(x[ok] - mx).sum())
        bound = (4 * n_lang + 8) * U32 + 2 * U32 * (np.abs(x[fin]) + abs(lse))  # test_gpu_language.kernel_expect's, with exact inputs
        worst = float((np.abs(got[fin].astype(np.float64) - (x[fin] - lse)) / bound).max())
        assert worst <= 1.0, (what, b, worst)
        return worst
    return 0.0


@pytest.mark.parametrize("n", [1, 5])
def test_rules_kernel_alone(rules_model, n):
    m = rules_model
    e, tok, n_lang = m["e"], m["tok"], m["n_lang"]
    nv, T = e.n_vocab, e.timestamp_begin
    rng = np.random.default_rng(300 + n + n_lang)
    base = (rng.standard_normal((5, nv)) * 3.0).astype(np.float32)
    base[:, tok] = (rng.standard_normal((5, n_lang)) * 6.0).astype(np.float32)  # language logits of order 10
    ctx = lambda k: [CTX0] * k
    # ---- offsets >= 2: the scored kernel's decision, bit for bit (it is the same body), nothing else written
    hists = [[T, 5], [T, 5, 9, T + 40, T + 40], [], [T], [T, 7, 8, 9]][:n]
    offs = [len(h) + 2 for h in hists]
    o = e.stream_rules_stage(base[:n], offs, [0] * n, [1] * n, hists, ctx(n))
    want, want_lp = e.score_timestamp_rules(base[:n], hists)
    assert o["chosen"].tolist() == want and o["logprob"].tobytes() == want_lp.tobytes()
    for b in range(n):
        assert o["no_speech"][b] == np.float32(S) and o["lang_out"][b] == SI and o["slot_ctx"][b].tolist() == CTX0
        assert (o["lang_logprob"][b] == np.float32(S)).all()
    # ---- offset 0 with detect: lang_reference.pick of the gathered logits
    tie = base[1].copy()
    tie[tok[40]] = tie[tok[10]] = np.float32(np.abs(tie[tok]).max() + 1.0)  # two equal maxima: the first wins
    some_nan = base[2].copy()
    some_nan[[tok[0], tok[17], tok[n_lang - 1]]] = np.nan
    some_nan[tok[3]] = -np.inf
    all_nan = base[3].copy()
    all_nan[tok] = np.nan
    nan_max = base[4].copy()
    nan_max[tok[int(np.argmax(nan_max[tok]))]] = np.nan  # where the maximum was: NaN never wins
    variants = [("plain", base[0]), ("tie", tie), ("some_nan", some_nan), ("all_nan", all_nan), ("nan_at_max", nan_max)]
    worst = 0.0
    groups = [[v] for v in variants] if n == 1 else [variants]
    for g in groups:
        rows = np.stack([r for _, r in g])
        ns = e.no_speech_logprob(rows)
        o = e.stream_rules_stage(rows, [0] * len(g), [0] * len(g), [1] * len(g), [[]] * len(g), ctx(len(g)))
        for b, (name, r) in enumerate(g):
            worst = max(worst, _check_detect(m, o, b, r, ns[b], name))
            if name == "tie":
                assert o["lang_out"][b] == 10 and o["lang_logprob"][b, 10].tobytes() == o["lang_logprob"][b, 40].tobytes()
            if name == "all_nan":
                assert o["lang_out"][b] == m["zh"] and np.isneginf(o["lang_logprob"][b]).all()
    print("%d languages, %d slot(s): lang_logprob error at most %.3g of its bound" % (n_lang, n, worst))
    # ---- a done slot is not touched whatever its offset; offset 1 writes nothing; without detect only no_speech is written
    if n == 1:
        cases = [dict(off=0, done=1, det=1), dict(off=5, done=1, det=0), dict(off=1, done=0, det=1), dict(off=0, done=0, det=0)]
        for c in cases:
            o = e.stream_rules_stage(base[:1], [c["off"]], [c["done"]], [c["det"]], [[T, 5, 6][: max(c["off"] - 2, 0)]], ctx(1))
            if c["done"] or c["off"] == 1:
                _untouched(o, 0, c)
            else:
                assert o["no_speech"][0].tobytes() == e.no_speech_logprob(base[:1])[0].tobytes()
                assert o["slot_ctx"][0].tolist() == CTX0 and o["lang_out"][0] == SI and (o["lang_logprob"][0] == np.float32(S)).all()
                assert o["chosen"][0] == SI and o["logprob"][0] == np.float32(S)
    else:  # all of it in one launch, beside a slot that samples and one that detects
        offs, done, det = [0, 5, 1, 0, 4], [1, 1, 0, 0, 0], [1, 0, 1, 0, 1]
        hists = [[], [T, 5, 6], [], [], [T, 5]]
        o = e.stream_rules_stage(base, offs, done, det, hists, ctx(5))
        for b in (0, 1, 2):
            _untouched(o, b, "mixed")
        ns = e.no_speech_logprob(base)
        assert o["no_speech"][3].tobytes() == ns[3].tobytes() and o["slot_ctx"][3].tolist() == CTX0 and o["lang_out"][3] == SI
        assert (o["lang_logprob"][3] == np.float32(S)).all() and o["chosen"][3] == SI
        w, wl = e.score_timestamp_rules(base[4:5], [hists[4]])
        assert o["chosen"][4] == w[0] and o["logprob"][4].tobytes() == wl[0].tobytes() and o["no_speech"][4] == np.float32(S)
        assert o["slot_ctx"][4].tolist() == CTX0 and o["lang_out"][4] == SI


# ------------------------------------------------------------------------------------------ B. refill in timestamp mode
def _check_scores_against_oracle(e, case, clip, r, what):
    """token_logprob and no_speech_logprob of one collected clip against score_reference on the oracle's rows, the oracle teacher-forced
    with the ENGINE's ids: |value - ref| <= 2 err + 1e-4 with err the logit error measured at that step (test_gpu_scores.py's rule)."""
    T, E, NS = e.timestamp_begin, e.eot, e.no_speech
    orc = case.oracle_bf16
    mel = e.compute_mel(clip)
    ck, cv = orc.encoder(mel)
    ids, n = r[1], len(r[1])
    lps = r[2]
    assert len(lps) == n + 1
    r0, rows = sr.oracle_rows(orc, ck, cv, orc.sot_seq("zh")[:3], ids)
    e.encode_mel(np.stack([mel] * 3))
    glog, _, _, _, l0 = e.decode_forced_timestamp_scores(3, np.array([ids] * 3, dtype=np.int32).reshape(3, n))
    ref = sr.clip_scores(rows, ids, T, E)
    left_out = 0
    worst = 0.0
    for i in range(n + 1):
        c = sr.token_logprob(rows[i], ids[:i], T, E)
        decision = ids[i] if i < n else None
        if decision is not None and decision != c[0]:
            assert c[2]["margin"] < 1e-4, (what, i, decision, c[0], c[2])
            left_out += 1
            continue
        if decision is None and not np.isfinite(ref["token_logprob"][i]):
            continue
        err = float(np.abs(glog[0, i] - rows[i]).max())
        if decision is None and c[0] == E:
            continue  # the oracle ends at eot where the engine's budget dropped an id (or the reverse): another decision, not a score
        d = abs(float(lps[i]) - float(ref["token_logprob"][i]))
        assert d <= 2 * err + 1e-4, (what, i, float(lps[i]), float(ref["token_logprob"][i]), "logit err", err)
        worst = max(worst, d)
    assert left_out * 49 <= n + 1, (what, left_out)
    err0 = float(np.abs(l0[0] - r0).max())
    assert abs(r[4] - float(sr.no_speech_logprob(r0, NS))) <= 2 * err0 + 1e-4, (what, r[4], err0)
    return worst


def test_refill_in_timestamp_mode(built_lib, micro_case):
    n_slots, n_clips = 8, 32
    clips, budgets = _clips_and_budgets(n_clips)
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=n_slots)
    try:
        got = e.run_stream_timestamps(clips, n_slots, max_new=budgets, steps_per_call=4)
        assert all(g is not None for g in got) and e.get_config_int("stream_mode") == 0
        T = e.timestamp_begin
        assert all(g[5] == "zh" and g[6] is None for g in got) and any(t >= T for g in got for t in g[1])
        # the same clips as ordinary ragged batches of 8 through the batched scored call
        bit_equal = 0
        for g0 in range(0, n_clips, n_slots):
            want = e.run_timestamp_scores_batch(clips[g0:g0 + n_slots], max_new=140, max_new_clip=budgets[g0:g0 + n_slots])
            for i in range(n_slots):
                g, w = got[g0 + i], want[i]
                assert g[1] == w["ids"], (g0 + i, g[1][:8], w["ids"][:8])
                same = np.array_equal(g[2], w["token_logprob"]) and g[4] == w["no_speech_logprob"] and g[3] == w["avg_logprob"]
                bit_equal += bool(same)
        print(f"{n_clips} clips through {n_slots} timestamp slots: scores bit-equal to the batched call for {bit_equal}/{n_clips} clips")
        # every clip on its own: a difference must be a numerical tie
        differ = []
        for i in range(n_clips):
            alone = e.run_timestamp_scores_batch([clips[i]], max_new=budgets[i])[0]["ids"]
            if alone != got[i][1]:
                differ.append(i)
                equal_or_tie(e, micro_case.oracle_bf16, micro_case.cfg, e.compute_mel(clips[i]), got[i][1], budgets[i], what=f"clip {i} through the slot stream")
        print(f"{n_clips - len(differ)}/{n_clips} identical to the stand-alone runs")
        assert len(differ) <= 2, differ
        worst = max(_check_scores_against_oracle(e, micro_case, clips[i], got[i], f"clip {i}") for i in range(n_clips))
        print("largest |token_logprob - oracle reference| %.3g" % worst)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ C. languages per slot
@pytest.fixture(scope="module")
def lang_model(built_lib, oracle_mod, tmp_path_factory):
    case = lr.LangCase("micro", 11, "BF16")
    root = case.write(tmp_path_factory.mktemp("stream_lang_micro"))
    e = built_lib.Whisper("micro", root, "zh", device=0, max_batch=6)
    yield dict(case=case, e=e, root=root)
    e.close()


BUDGET_C = 12


def test_languages_per_slot(lang_model):
    case, e = lang_model["case"], lang_model["e"]
    codes, zh = case.codes, case.handle_index
    kept = case.kept()
    ex = {i: case.expect(i) for i in kept}
    # the measured logit error of the detection position, every kept clip in one batch (test_gpu_language.stage_error)
    e.encode_mel(np.stack([ex[i]["mel"] for i in kept]))
    lg = e.detect_language_stage(len(kept))[2]
    err = max(float(np.abs(lg[b] - ex[i]["lang_logit"]).max()) for b, i in enumerate(kept))
    # detecting clips: the oracle alone must decide them (margin above four times the measured error) — checked here, nobody is excused
    det = []
    for i in kept:
        if ex[i]["index"] not in {ex[k]["index"] for k in det}:
            det.append(i)
    det = det[:5]
    assert len(det) >= 3 and len({ex[i]["index"] for i in det}) == len(det), det
    for i in det:
        assert ex[i]["margin"] > 4 * err, (i, ex[i]["margin"], err)
    others = [j for j in range(case.n_lang) if j != zh][:4]
    plan = [(kept[0], codes[others[0]], "transcribe"), (kept[1], codes[others[1]], "transcribe"), (kept[2], codes[others[2]], "transcribe"),
            (kept[3 % len(kept)], codes[others[3]], "translate"), (kept[0], None, "transcribe"), (kept[1], "zh", "transcribe")]
    plan += [(i, "auto", "transcribe") for i in det]
    while len(plan) < 12:
        plan.append((kept[len(plan) % len(kept)], codes[others[len(plan) % 4]], "transcribe"))
    plan = plan[:12]
    clips = [case.clips()[i] for i, _, _ in plan]
    got = e.run_stream_timestamps(clips, 6, max_new=BUDGET_C, languages=[l for _, l, _ in plan], tasks=[t for _, _, t in plan])
    ties = 0
    for (i, lang, task), g in zip(plan, got):
        want_lang = codes[ex[i]["index"]] if lang == "auto" else (lang or "zh")
        assert g[5] == want_lang, (i, lang, g[5])
        if lang == "auto":
            want_lp = ex[i]["lang_logprob"]
            assert g[6] is not None and np.abs(g[6] - want_lp).max() <= 2 * err + 1e-4, (i, float(np.abs(g[6] - want_lp).max()), err)
        else:
            assert g[6] is None
        t = 1 if task == "translate" else 0
        ok = equal_or_tie(e, case.oracle, case.cfg, ex[i]["mel"], g[1], BUDGET_C, want_lang, t, what=f"clip {i} language {lang} task {task}")
        ties += not ok
        assert len(g[2]) == len(g[1]) + 1 and np.isfinite(g[4])
    print("12 clips, 6 slots: measured logit error %.3g, smallest detecting margin %.3g, %d tie(s)" % (err, min(ex[i]["margin"] for i in det), ties))


# ------------------------------------------------------------------------------------------ D. 72 slots
def test_stream_ts_beyond_64_slots(built_lib, micro_case):
    n_slots, n_clips = 72, 150
    clips8, _ = _clips_and_budgets(8)
    clips = [clips8[i % 8] for i in range(n_clips)]
    budgets = [6 + (11 * i) % 23 for i in range(n_clips)]  # 6 .. 28
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=n_slots)
    try:
        got = e.run_stream_timestamps(clips, n_slots, max_new=budgets, steps_per_call=4)
        assert all(g is not None for g in got)
        alone = [e.run_timestamp_scores_batch([c], max_new=28)[0]["ids"] for c in clips8]
        diff = [i for i in range(n_clips) if got[i][1] != alone[i % 8][:budgets[i]]]
        print(f"{n_clips} clips through {n_slots} timestamp slots: {n_clips - len(diff)}/{n_clips} identical to the stand-alone runs")
        mels = {}
        for i in diff:
            mels.setdefault(i % 8, e.compute_mel(clips[i]))
            equal_or_tie(e, micro_case.oracle_bf16, micro_case.cfg, mels[i % 8], got[i][1], budgets[i], what=f"clip {i} through 72 slots")
        assert len({i % 8 for i in diff}) <= 2, sorted({i % 8 for i in diff})
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ E. smallest streams, the context edge
def test_stream_ts_one_and_two_slots_and_full_context(built_lib, micro_case):
    import modelgen

    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=2)
    try:
        clips = [modelgen.synth_clip(70 + i, 160000) for i in range(7)]
        budgets = [0, 9, 17, 3, 30, 12, 25]  # clip 0: no budget -> n_text_ctx - 3 ids
        got = e.run_stream_timestamps(clips, 2, max_new=budgets)
        ref = [e.run_timestamp_scores_batch([c], max_new=b)[0] for c, b in zip(clips, budgets)]
        assert len(ref[0]["ids"]) == e.n_text_ctx - 3 or ref[0]["ended_eot"]
        assert len(got[0][1]) == len(ref[0]["ids"])
        same = sum(r["ids"] == g[1] for r, g in zip(ref, got))
        for i, (r, g) in enumerate(zip(ref, got)):
            assert len(g[2]) == len(g[1]) + 1
            if r["ids"] != g[1]:
                equal_or_tie(e, micro_case.oracle_bf16, micro_case.cfg, e.compute_mel(clips[i]), g[1], budgets[i], what=f"clip {i}, two slots")
        assert same >= 6
        got1 = e.run_stream_timestamps(clips[1:], 1, max_new=budgets[1:])  # one slot, reused six times
        for a, b in zip(got1, got[1:]):
            assert a[1] == b[1] and a[5] == b[5] == "zh" and len(a[2]) == len(b[2])
            assert np.abs(a[2] - b[2]).max() <= 1e-3 and abs(a[4] - b[4]) <= 1e-3  # (the same kernels at the same slot count: in fact equal)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ F. stale state
def test_one_slot_inherits_nothing(lang_model):
    case, e = lang_model["case"], lang_model["e"]
    codes, zh = case.codes, case.handle_index
    kept = case.kept()
    x = next(i for i in kept if case.expect(i)["index"] != zh)  # detects a language other than the handle's
    y = next(j for j in range(case.n_lang) if j not in (zh, case.expect(x)["index"]))
    clips = [case.clips()[x], case.clips()[kept[1] if kept[1] != x else kept[2]], case.clips()[kept[-1]]]
    langs, tasks = ["auto", None, codes[y]], ["transcribe", "transcribe", "translate"]
    chain = e.run_stream_timestamps(clips, 1, max_new=[5, 9, 7], languages=langs, tasks=tasks)
    assert chain[0][5] == codes[case.expect(x)["index"]] and chain[1][5] == "zh" and chain[2][5] == codes[y]
    assert chain[0][6] is not None and chain[1][6] is None and chain[2][6] is None
    for k in range(3):
        fresh = e.run_stream_timestamps([clips[k]], 1, max_new=[[5, 9, 7][k]], languages=[langs[k]], tasks=[tasks[k]])[0]
        assert chain[k][1] == fresh[1] and chain[k][5] == fresh[5], (k, chain[k][1], fresh[1])
        assert chain[k][4] == fresh[4] and len(chain[k][2]) == len(fresh[2]) and np.array_equal(chain[k][2], fresh[2]), k
        assert chain[k][3] == fresh[3]
    # the raw collect: a slot that did not detect reports zeros, not the previous clip's language log-probabilities
    e.stream_open(1, timestamps=True)
    try:
        for k in range(2):
            e.stream_admit_batch([0], [clips[k]], [4], languages=[langs[k]], tasks=[tasks[k]])
            fin = []
            for _ in range(60):
                fin = e.stream_step(2)
                if fin:
                    break
            assert fin == [0]
            r = e.stream_collect_scored(0)
            assert (np.abs(r["lang_logprob"]).max() > 0) == (k == 0)
    finally:
        e.stream_close()


# ------------------------------------------------------------------------------------------ G. other models
def test_stream_ts_fp16_and_turbo_width(built_lib, oracle_mod, tmp_path):
    import modelgen

    for model_type, seed, dtype, n_slots, n in (("miniturbo", 21, "F16", 3, 5), ("w1280", 3, "BF16", 4, 9)):
        case = ModelCase(tmp_path / model_type, model_type, seed, dtype=dtype)
        e = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=n_slots)
        try:
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"fp16") == (1 if dtype == "F16" else 0)
            clips = [modelgen.synth_clip(150 + i, 90000 + 40000 * i) for i in range(n)]
            budgets = [7, 33, 12, 40, 5, 21, 30, 9, 16][:n]
            got = e.run_stream_timestamps(clips, n_slots, max_new=budgets, steps_per_call=3)
            for g0 in range(0, n, n_slots):
                grp = clips[g0:g0 + n_slots]
                if len(grp) < 3:  # fewer than three clips take another step sequence: pad the batch, the stream ran three slots too
                    grp = grp + [clips[0]] * (3 - len(grp))
                want = e.run_timestamp_scores_batch(grp, max_new=40, max_new_clip=(budgets[g0:g0 + n_slots] + [5] * 3)[:len(grp)])
                for i in range(min(n_slots, n - g0)):
                    g, w = got[g0 + i], want[i]
                    if g[1] != w["ids"]:
                        equal_or_tie(e, case.oracle_bf16, case.cfg, e.compute_mel(clips[g0 + i]), g[1], budgets[g0 + i], what=f"{model_type} clip {g0 + i}")
                    else:
                        assert np.abs(g[2] - w["token_logprob"]).max() <= 1e-3 and abs(g[4] - w["no_speech_logprob"]) <= 1e-3
        finally:
            e.close()


# ------------------------------------------------------------------------------------------ H. refusals
def test_refusals_leave_running_slots_intact(built_lib, micro_case, tmp_path):
    import json
    import os
    import shutil

    clips, _ = _clips_and_budgets(4)
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=4)
    try:
        want = [e.run_timestamp_scores_batch([c] * 3, max_new=10)[0]["ids"] for c in clips[:2]]
        plain = e.run_tokens_batch(clips[:3], max_new=10)

        def finish(slot):
            for _ in range(80):
                if slot in e.stream_step(2):
                    return
            raise AssertionError("the slot never finished")

        with pytest.raises(RuntimeError, match="unknown mode"):
            e.stream_open(4, timestamps=2)
        assert e.run_tokens(clips[0], max_new=3) is not None  # the handle is usable, no stream is open
        # ---- a mode-0 stream: language / task arguments and the scored collect are refused, the running slot finishes with its ids
        e.stream_open(4, timestamps=0)  # StreamOpenMode(mode 0)
        assert e.get_config_int("stream_mode") == 0
        e.stream_admit(1, clips[0], 10)
        with pytest.raises(RuntimeError, match="timestamp mode"):
            e.stream_admit_batch([2], [clips[1]], [10], languages=["en"])
        with pytest.raises(RuntimeError, match="timestamp mode"):
            e.stream_admit_batch([2], [clips[1]], [10], tasks=["translate"])
        finish(1)
        with pytest.raises(RuntimeError, match="timestamp mode"):
            e.stream_collect_scored(1)
        assert e.stream_collect(1) == plain[0]
        e.stream_close()
        # ---- a mode-1 stream
        e.stream_open(4, timestamps=True)
        assert e.get_config_int("stream_mode") == 1
        e.stream_admit(0, clips[0], 10)
        for bad in (dict(languages=[-3]), dict(languages=[e.n_lang]), dict(tasks=[2]), dict(tasks=[-1])):
            with pytest.raises(RuntimeError):
                e.stream_admit_batch([2], [clips[1]], [10], **bad)
        e.stream_admit_batch([2], [clips[1]], [10], languages=[None], tasks=["transcribe"])  # slot 2 was left idle by the refusals
        finish(0)
        finish(2)
        assert e.stream_collect(0) == want[0]  # StreamCollect on a mode-1 stream: the ids with their timestamp tokens
        assert e.stream_collect_scored(2)["ids"] == want[1]
        e.stream_close()
        assert e.get_config_int("stream_mode") == 0
        # ---- a mode-0 stream opened through StreamOpenMode gives what StreamOpen gives (test_gpu_stream.py's first assertions)
        n_slots, n_clips = 8, 32
    finally:
        e.close()
    clips32, budgets = _clips_and_budgets(n_clips)
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=n_slots)
    try:
        orig = e.stream_open
        e.stream_open = lambda n, timestamps=False: orig(n, timestamps=0)  # run_stream opens through StreamOpenMode(mode 0)
        got, _ = e.run_stream(clips32, n_slots, max_new=budgets, steps_per_call=4)
        del e.stream_open
        assert all(g is not None and len(g) == b for g, b in zip(got, budgets)), [len(g) for g in got]
        for g0 in range(0, n_clips, n_slots):
            mels = np.stack([e.compute_mel(c) for c in clips32[g0:g0 + n_slots]])
            e.encode_mel(mels)
            want8 = e.decode_greedy(n_slots, max_new=140, max_new_clip=budgets[g0:g0 + n_slots])
            for i in range(n_slots):
                assert got[g0 + i] == want8[i], (g0 + i, got[g0 + i][:8], want8[i][:8])
    finally:
        e.close()
    # ---- translate without a translate id, detection on a one-language config
    root = str(tmp_path / "one_language")
    shutil.copytree(micro_case.root, root)
    cfg_path = next(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith("_config.json"))
    cfg = json.load(open(cfg_path))
    cfg.pop("translate")
    first = cfg["all_language_tokens"].split(",")[lr.lang_codes(cfg).index("zh")]
    cfg["all_language_tokens"], cfg["all_language_codes"] = first, "zh"
    json.dump(cfg, open(cfg_path, "w"))
    e = built_lib.Whisper("micro", root, "zh", device=0, max_batch=3)
    try:
        e.stream_open(3, timestamps=True)
        e.stream_admit(0, clips[0], 10)
        with pytest.raises(RuntimeError, match="translate"):
            e.stream_admit_batch([1], [clips[1]], [10], tasks=["translate"])
        with pytest.raises(RuntimeError, match="more than one language"):
            e.stream_admit_batch([1], [clips[1]], [10], languages=["auto"])
        finish_ids = None
        for _ in range(80):
            if 0 in e.stream_step(2):
                finish_ids = e.stream_collect(0)
                break
        assert finish_ids == want[0]
        e.stream_close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ I. whisper_srv --timestamps
def _start_server(built_lib, root, *flags):
    import json
    import os
    import socket
    import subprocess
    import time
    import urllib.request

    srv = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_srv")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    proc = subprocess.Popen([srv, "--port", str(port), "-t", "micro", "-p", root, "-l", "zh", "--max_batch", "4", *flags],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    base = f"http://127.0.0.1:{port}"
    for _ in range(200):
        if proc.poll() is not None:
            return proc, base
        try:
            if json.load(urllib.request.urlopen(base + "/health", timeout=2))["status"] == "ok":
                return proc, base
        except Exception:
            time.sleep(0.1)
    proc.kill()
    raise AssertionError("server did not come up")


def _post(base, body, **headers):
    """(status, raw reply bytes) of POST /asr."""
    import urllib.error
    import urllib.request

    req = urllib.request.Request(base + "/asr", data=body, headers={"Content-Type": "application/octet-stream", **headers}, method="POST")
    try:
        r = urllib.request.urlopen(req, timeout=120)
        return r.status, r.read()
    except urllib.error.HTTPError as err:
        return err.code, err.read()


def test_server_timestamps(built_lib, lang_model):
    import json
    import threading

    case, e = lang_model["case"], lang_model["e"]
    root = lang_model["root"]
    codes, zh = case.codes, case.handle_index
    kept = case.kept()
    other = next(codes[j] for j in range(case.n_lang) if j != zh)
    reqs = [(kept[0], {"X-Timestamps": "1", "X-Language": other}), (kept[1], {"X-Timestamps": "1", "X-Language": "auto"}),
            (kept[2], {"X-Task": "translate", "X-Timestamps": "0"}), (kept[3 % len(kept)], {"x-language": "ZH", "X-Timestamps": "1", "X-Task": "transcribe"})]
    clips = [case.clips()[i] for i, _ in reqs]
    langs = [h.get("X-Language", h.get("x-language")) for _, h in reqs]
    langs = [None if l is None else l.lower() for l in langs]
    tasks = ["translate" if h.get("X-Task") == "translate" else "transcribe" for _, h in reqs]
    want = e.run_stream_timestamps(clips, 4, languages=langs, tasks=tasks)
    proc, base = _start_server(built_lib, root, "--timestamps")
    try:
        assert proc.poll() is None
        out = [None] * 4
        th = [threading.Thread(target=lambda k=k: out.__setitem__(k, _post(base, clips[k].tobytes(), **reqs[k][1]))) for k in range(4)]
        [t.start() for t in th]
        [t.join() for t in th]
        load = lambda raw: json.loads(raw.decode("utf-8", errors="replace"))  # (ids of a synthetic model need not be whole characters)
        for k, (st, raw) in enumerate(out):
            js = load(raw)
            segs, ids, _, avg, nsp, language, _ = want[k]
            assert st == 200 and js["success"] is True, (k, st, raw)
            # "text": the segments' bytes one after the other (no OpenCC data beside these models: the transcript is the detokenised ids)
            cuts = built_lib.split_segments(ids, e.timestamp_begin, e.eot, min(len(clips[k]) / 16000.0, 30.0))
            text = b"".join(e.detokenize(ids[t0:t1]) for _, _, t0, t1 in cuts).decode("utf-8", errors="replace")
            assert js["text"] == text and js["language"] == language, (k, js, language)
            if reqs[k][1].get("X-Timestamps") == "1":
                assert [(s["start"], s["end"], s["text"]) for s in js["segments"]] == [(round(a, 2), round(b, 2), t) for a, b, t in segs], (k, js["segments"], segs)
                assert abs(js["avg_logprob"] - avg) <= 1e-6 * max(1.0, abs(avg)) and abs(js["no_speech_prob"] - float(np.exp(np.float64(nsp)))) <= 1e-6
            else:
                assert "segments" not in js and "avg_logprob" not in js and "no_speech_prob" not in js
        # the 400s, each with its fixed string; a plain request on a --timestamps server is served in the handle's language
        pcm = clips[0].tobytes()
        for hdr, msg in (({"X-Timestamps": "2"}, "X-Timestamps must be 0 or 1"), ({"X-Language": "e1"}, "X-Language must be a language code or auto"),
                         ({"X-Language": "qq"}, "X-Language names a language the model does not list"),
                         ({"X-Task": "summarise"}, "X-Task must be transcribe or translate")):
            st, raw = _post(base, pcm, **hdr)
            assert st == 400 and json.loads(raw) == {"error": msg}, (hdr, st, raw)
        st, raw = _post(base, pcm)
        assert st == 200 and load(raw)["language"] == "zh" and set(load(raw)) == {"success", "text", "language"}
    finally:
        proc.kill()
    # micro-batches and --timestamps: refused at start-up
    proc, _ = _start_server(built_lib, root, "--timestamps", "--scheduler", "batches")
    assert proc.wait(timeout=30) == 1 and "--timestamps needs --scheduler slots" in proc.stdout.read()
    # a server without the flag: a plain request byte for byte as before, the new headers a 400 that says so
    proc, base = _start_server(built_lib, root)
    try:
        st, raw = _post(base, clips[0].tobytes())
        assert st == 200 and raw.startswith(b'{\n  "success": true,\n  "text": "') and raw.endswith(b'"\n}')
        js = json.loads(raw.decode("utf-8", errors="replace"))
        assert set(js) == {"success", "text"} and js["text"] == e.run(clips[0])
        for hdr in ({"X-Timestamps": "1"}, {"X-Language": "en"}, {"X-Task": "translate"}, {"X-Timestamps": "0"}):
            st, raw = _post(base, clips[0].tobytes(), **hdr)
            assert st == 400 and json.loads(raw) == {"error": "X-Timestamps, X-Language and X-Task need a server started with --timestamps"}, (hdr, raw)
    finally:
        proc.kill()
