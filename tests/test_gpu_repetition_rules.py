"""GPU: the repetition rules (DESIGN.md "Repetition rules") — the stage-level rules calls on hand-made rows and histories against
tests/repetition_reference.py (ids exact, log-probabilities within the bound it derives), the off state, and the decode loops."""
import math

import numpy as np
import pytest

import beam_reference as br
import repetition_reference as rr
import sample_reference as smp
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

SEED, TEMP, MAX_NEW = 0x5EED, 0.7, 24


@pytest.fixture(scope="module")
def model(built_lib, oracle_mod, tmp_path_factory):
    case = ModelCase(tmp_path_factory.mktemp("rep"), "micro", 11)
    e = built_lib.Whisper("micro", case.root, "zh", device=0, max_batch=12)
    e.case = case
    assert e.repetition_rules == (1.0, 0) and e.get_config_int("repetition_rules") == 0 and e.get_config_int("no_repeat_ngram_size") == 0
    yield e
    e.close()


def _row(e, seed, boosts, text=None):
    """low noise (timestamps far below the text), then the ids a case is about; text: the value of every other text id"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(e.n_vocab) * 0.3).astype(np.float32)
    x[e.timestamp_begin:] -= np.float32(20.0)
    if text is not None:
        x[: e.eot] = text
    for i, v in boosts.items():
        x[i] = v
    return x


def _cases(e):
    """config name -> (penalty, ngram, suppress set, [(history, row)])"""
    T, E, inf = e.timestamp_begin, e.eot, math.inf
    two = [T, 5, 9, 5, 7, 5]  # g = 2: 9 and 7 are banned
    lh = [T] + [100 + i for i in range(299)]  # 300 ids: the last 15 also stand at 10 and at 261 (past one round of the 256-stride scan)
    lh[261:276] = lh[-15:] = lh[10:25]
    return {
        "penalty": (1.5, 0, [], [
            ([T, 5, 9, 5, 7, 5, 11], _row(e, 1, {5: 12.0, 20: 7.0, 9: -3.0, 7: 0.0})),       # 5 occurs 3 times: 8 once, 3.6 if thrice
            ([T, 5, 9, 5, 7, 5, 11], _row(e, 2, {9: -0.5, 20: -0.6, E: -3.0}, text=-5.0)),    # a negative winner: -0.75 loses to -0.6
            ([T, 5, E, 6], _row(e, 3, {E: 10.0, 30: 9.0, 6: 12.0})),                          # eot in the history stays 10
            ([T, 5, T + 10], _row(e, 4, {T + 10: 10.0, T + 11: 9.0})),                        # an open pair: T + 10 stays 10
            (lh, _row(e, 7, {lh[290]: 12.0, 30: 10.0}))]),                                    # an id seen only past position 256
        "ngram2": (1.0, 2, [], [
            (two, _row(e, 11, {9: 12.0, 7: 11.0, 30: 10.0})),                                 # two matches, both continuations
            ([T, 5, E, 7, 5], _row(e, 12, {E: 12.0, 30: 10.0})),                              # eot as continuation
            ([T, 5, T + 5, T + 5, 5], _row(e, 13, {T + 6: 12.0, 30: 10.0})),                  # a timestamp as continuation
            ([T, 5, 6, 7], _row(e, 14, {5: 12.0, 30: 10.0})),                                 # no match
            ([], _row(e, 15, {T + 3: 5.0})), ([T], _row(e, 16, {30: 9.0})), ([5, 5], _row(e, 17, {5: 12.0, 30: 10.0})),  # n = 0, g - 1, g
            (two, _row(e, 18, {9: 12.0, 7: 11.0, E: 4.0}, text=-inf)),                        # every finite text id banned: eot
            (two, _row(e, 19, {9: 12.0, 7: 11.0, E: 4.0, T + 20: 15.0}, text=-inf))]),        # ... or the timestamps
        "ngram3": (1.0, 3, [], [
            ([T, 5, 6, 9, 5, 6], _row(e, 21, {9: 12.0, 30: 10.0})),
            ([T, 5, 5, 5], _row(e, 22, {5: 12.0, 30: 10.0}))]),                               # a match that overlaps the tail
        "ngram16": (1.1, 16, [], [
            (lh, _row(e, 31, {lh[25]: 12.0, lh[276]: 11.5, 30: 10.0})),                       # matches at 10 and 261
            (lh[:15], _row(e, 32, {30: 10.0})), (lh[:16], _row(e, 33, {30: 10.0}))]),
        "both_and_a_set": (1.3, 2, [30, 31], [
            (two, _row(e, 41, {9: 12.0, 30: 11.5, 5: 13.0, 40: 9.0})),                        # 9 banned, 30 suppressed, 5 scaled to 10
            ([T, 5, 6, 7], _row(e, 42, {31: 12.0, 6: 11.0, 40: 8.0}))]),
    }


def _close(got, want, bound):
    return float(got) == float(want) or abs(float(got) - float(want)) <= bound


@pytest.mark.parametrize("name", ["penalty", "ngram2", "ngram3", "ngram16", "both_and_a_set"])
def test_rules_kernels_against_the_reference(model, name):
    e, T, E = model, model.timestamp_begin, model.eot
    p, g, S, cases = _cases(e)[name]
    hists, x = [h for h, _ in cases], np.stack([r for _, r in cases])
    n = len(cases)
    if name == "ngram16":
        assert len(rr.banned(hists[0], E, g)) == 2 and len(hists[0]) > 256
    streams = [(b * 7 + 1) | ((b % 3) << 32) for b in range(n)]
    e.set_suppress_tokens(S)
    e.set_repetition_rules(p, g)
    try:
        assert e.repetition_rules == (float(np.float32(p)), g) and e.get_config_int("repetition_rules") == 1 and e.get_config_int("no_repeat_ngram_size") == g
        plain = e.apply_timestamp_rules(x, hists)
        scored = e.score_timestamp_rules(x, hists)
        sampled = e.sample_timestamp_rules(x, hists, TEMP, streams, SEED)
        o = e.stream_rules_stage(x, [len(h) + 2 for h in hists], [0] * n, [0] * n, hists, [[11, 22, 33, 44]] * n)
        cid, clp, nc = e.beam_candidates(x, hists, 3)
    finally:
        e.set_repetition_rules(1.0, 0)
        e.set_suppress_tokens([])
    for b in range(n):
        c, lp, info = rr.decide(x[b], hists[b], T, E, p, g, S)
        assert plain[b] == c and scored[0][b] == c and int(o["chosen"][b]) == c, (name, b)
        assert _close(scored[1][b], lp, info["bound"]) and _close(o["logprob"][b], lp, info["bound"]), (name, b, float(scored[1][b]), float(lp))
        cs, lps, si = smp.sample(info["row"], hists[b], T, E, TEMP, streams[b], SEED)  # the Gumbel-max draw over the edited row
        assert not si["near_tie"] and sampled[0][b] == cs and _close(sampled[1][b], lps, rr.logprob_bound(info["row"], si)), (name, b, si)
        ids, lps, bi = br.candidates(info["row"], hists[b], T, E, 3)  # the hypothesis' candidates: the best ids of the same edited row
        assert [int(v) for v in cid[b, : nc[b]]] == ids and not br.rule5_near_tie(bi), (name, b, cid[b], ids)
        bounds = [rr.logprob_bound(info["row"], dict(x_chosen=float(info["row"][i]), lse_allowed=bi["lse_allowed"])) for i in ids]
        assert np.all(np.abs(clp[b, : len(ids)] - lps) <= bounds), (name, b, clp[b], lps)


def test_setter_refusals_and_the_off_state(model):
    e = model
    hists, x = map(list, zip(*_cases(e)["ngram2"][3]))
    fresh = (e.apply_timestamp_rules(x, hists), e.score_timestamp_rules(x, hists))
    for p, g, text in ((0.0, 0, "repetition_penalty"), (-1.0, 0, "repetition_penalty"), (math.inf, 0, "repetition_penalty"), (math.nan, 0, "repetition_penalty"),
                       (1.0, 1, "no_repeat_ngram_size"), (1.0, 17, "no_repeat_ngram_size"), (1.0, -2, "no_repeat_ngram_size")):
        with pytest.raises(RuntimeError, match=text):
            e.set_repetition_rules(p, g)
        assert e.repetition_rules == (1.0, 0)
    e.set_repetition_rules(1.2, 3)
    e.stream_open(2, timestamps=True)
    try:
        with pytest.raises(RuntimeError, match="stream"):
            e.set_repetition_rules(1.0, 0)
        assert e.repetition_rules == (float(np.float32(1.2)), 3)
    finally:
        e.stream_close()
    assert e.score_timestamp_rules(x, hists)[1].tobytes() != fresh[1][1].tobytes()  # (the rules were on)
    e.set_repetition_rules()
    assert e.repetition_rules == (1.0, 0) and e.get_config_int("repetition_rules") == 0 and e.get_config_int("no_repeat_ngram_size") == 0
    again = (e.apply_timestamp_rules(x, hists), e.score_timestamp_rules(x, hists))
    assert again[0] == fresh[0] and again[1][0] == fresh[1][0] and again[1][1].tobytes() == fresh[1][1].tobytes()


def test_one_clip_decode_leaves_the_persistent_rules_launch(model, built_lib, monkeypatch):
    monkeypatch.setenv("AX_WHISPER_PERSIST_TS", "1")
    e = built_lib.Whisper("micro", model.case.root, "zh", device=0, max_batch=1)
    monkeypatch.delenv("AX_WHISPER_PERSIST_TS")
    try:
        for rules, launches in (((1.25, 4), 0), ((1.0, 0), 1)):  # counted only once the rules are off again
            e.set_repetition_rules(*rules)
            e.run_timestamp_scores_batch([load_demo_pcm()], max_new=8)
            assert e.get_config_int("persistent_ts") == 1 and e.persistent_ts_launches == launches
    finally:
        e.close()


def test_loops_never_repeat_a_text_bigram(model):
    """The scored loop under no_repeat_ngram_size = 2 against the reference on the raw rows of a forced decode without rules; no text
    bigram occurs twice; the slot stream and beam search of one hypothesis decode the same ids, and five hypotheses repeat none either."""
    e, T, E = model, model.timestamp_begin, model.eot
    pcm = load_demo_pcm()
    n = len(pcm)
    clips = [pcm, pcm[: n * 2 // 3] * np.float32(0.7), pcm[n // 5:], np.concatenate([pcm[n // 3:], pcm[: n // 3]]) * np.float32(1.3)]
    before = e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
    e.set_repetition_rules(1.0, 2)
    try:
        got = e.run_timestamp_scores_batch(clips, max_new=MAX_NEW)
        e.set_repetition_rules(1.0, 0)  # the slots still hold this call's cross K/V
        n = [len(r["ids"]) for r in got]
        f = np.array([r["ids"] + [0] * (max(n) - len(r["ids"])) for r in got], dtype=np.int32)
        logits, _, _, _, _ = e.decode_forced_timestamp_scores(len(clips), f)
        e.set_repetition_rules(1.0, 2)
        stream = e.run_stream_timestamps(clips, 2, max_new=MAX_NEW)
        beam1, beam5 = e.run_beam_batch(clips[:2], 1, MAX_NEW), e.run_beam_batch(clips[:2], 5, MAX_NEW)
    finally:
        e.set_repetition_rules(1.0, 0)
    left_out = 0
    bigrams = lambda ids: [(u, v) for u, v in zip(ids, ids[1:]) if u < E and v < E]
    assert any(len(bigrams(r["ids"])) != len(set(bigrams(r["ids"]))) for r in before)  # (without the rule the clips do loop)
    assert [r["ids"] for r in beam1] == [r["ids"] for r in got[:2]]
    for b, r in enumerate(got + beam5):
        assert len(bigrams(r["ids"])) == len(set(bigrams(r["ids"]))), (b, r["ids"])
    for b, r in enumerate(got):
        ids = r["ids"]
        for i in range(n[b] + 1):
            c, lp, info = rr.decide(logits[b, i], ids[:i], T, E, 1.0, 2, min_margin=None)
            if info["margin"] < 2 * 0.0 + 1e-4:  # tests/conftest.py's logit error rule, 2 * err + 1e-4: the rows are the engine's own, err = 0
                left_out += 1
                continue
            assert (ids[i] if i < n[b] else c) == c, (b, i, ids, c)
            assert _close(r["token_logprob"][i], lp, info["bound"]), (b, i, float(r["token_logprob"][i]), float(lp))
    assert left_out * 20 <= sum(n) + len(n), (left_out, n)  # (at most 5 % of the steps)
    assert [list(s[1]) for s in stream] == [r["ids"] for r in got]
