"""GPU: prompt conditioning (DESIGN.md "Prompt conditioning") — the prefill pass and the step-fed route against the oracle's
step-fed caches, prompted ids against tests/prompt_reference.greedy_prompted under the tie rule, ragged batches, the context end,
isolation from the unprompted entry points, the long-form carry against a Python loop over the oracle, two engines, the CLI.

Models micro (bf16) and miniturbo (fp16), demo.wav's first window, the prompt cases of tests/test_prompt_reference.py (lengths on
both sides of every 64-key block edge), budgets of at most 12 ids.

Bars. Self K/V after the prefill against the oracle's: 2e-2, the cross-K/V bar of test_gpu_parity.py (the same arithmetic class:
16-bit-activation MFMA GEMMs feeding a 16-bit cache); the step-fed route meets it on the same cases. Ids: equal, or the first
divergence is a measured tie (the oracle's decision margin below twice the logit error at that step, the engine teacher-forced under
the same prompt, + 1e-4), at most 2 of the 16 cases per route and batch size. No-speech: twice the measured error of the sot row +
1e-4. The first forced row behind the hand-over (it depends on off, tok and n_out of the hand-over and on every cached row): 2e-2,
the cache bar, and a fifth of the row's own spread — a wrong offset or token moves the row by the order of its spread."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import longform_reference as lfr
import prompt_reference as pr
import score_reference as sr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

KV_BAR = 2e-2
BUDGET = pr.N_DECISIONS
EXCUSED = {}  # (route, batch) -> {(model, P)}: the cases the tie rule excused, over both models


class Model:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        import oracle

        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.orc = self.case.oracle_bf16
        self.cfg = self.case.cfg
        self.pcm = load_demo_pcm()
        self.mel = oracle.log_mel(self.pcm, self.case.dims["n_mels"])[0]
        self.ck, self.cv = self.orc.encoder(self.mel)
        self.prefix = self.orc.sot_seq("zh")[:3]
        self.T, self.E, self.NS = int(self.cfg["no_timestamps"]) + 1, int(self.cfg["eot"]), int(self.cfg["no_speech"])
        self.engines = {}
        # the cases: computed once, shared by every test, never changed
        self.cases = {}
        for P in pr.LENGTHS:
            sd, prompt, _, _ = pr.find_case(self.orc, self.ck, self.cv, self.prefix, P)
            ids, infos, rows, (sk, sv, sot_row) = pr.greedy_prompted(self.orc, self.ck, self.cv, pr.context(self.cfg, prompt, self.prefix),
                                                                     max_new=BUDGET, want_logits=True, want_cache=True)
            self.cases[P] = dict(prompt=prompt, ids=ids, infos=infos, rows=rows, sk=sk[:, : P + 3].copy(), sv=sv[:, : P + 3].copy(), sot_row=sot_row)
        self.plain = tsr.greedy_ts(self.orc, self.ck, self.cv, self.prefix, max_new=BUDGET)[0]

    def engine(self, route, max_batch=8, **env):
        """One engine per (route, environment); both are read when the engine is made. route None: AX_WHISPER_PREFILL unset."""
        key = (route, max_batch, tuple(sorted(env.items())))
        if key not in self.engines:
            env = dict(env, AX_WHISPER_PREFILL=route)
            old = {k: os.environ.get(k) for k in env}
            for k, v in env.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            try:
                self.engines[key] = self.lib.Whisper(self.case.model_type, self.case.root, "zh", device=0, max_batch=max_batch)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            assert self.engines[key].get_config_int("prefill") == (1 if route == "step" else 0)  # (unset: the pass, which measured faster)
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()

    def ids_equal_or_tie(self, e, P, got, what, batch=1):
        """True: equal to the oracle's ids. False: the first divergence is a measured tie. Anything else fails."""
        c = self.cases[P]
        ids = c["ids"]
        if list(got) == list(ids):
            return True
        n = min(len(got), len(ids))
        i = next((i for i in range(n) if got[i] != ids[i]), n)
        assert i < len(c["rows"]), (what, P, ids, got)
        e.encode_mel(np.stack([self.mel] * batch))
        lg = e.decode_forced_timestamp_prompted([c["prompt"]] * batch, np.array([ids[:i]] * batch, dtype=np.int32).reshape(batch, i))[0]
        err = float(np.abs(lg[0, i] - c["rows"][i]).max())
        print("%s P %d: diverges at %d, margin %.3g, logit err %.3g" % (what, P, i, c["infos"][i]["margin"], err))
        assert c["infos"][i]["margin"] < 2 * err + 1e-4, (what, P, "step", i, c["infos"][i], "logit err", err, ids, got)
        return False


@pytest.fixture(scope="module", params=pr.MODELS, ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("prompt_" + request.param[0]), *request.param)
    yield m
    m.close()


@pytest.mark.parametrize("route", ["prefill", "step"])
def test_caches_no_speech_and_hand_over_against_the_oracle(model, route):
    """Test 2: self K/V of the context rows, the no-speech value and the first row behind the hand-over, on the eight lengths."""
    e = model.engine(route)
    worst_k = worst_v = worst_row = 0.0
    for P in pr.LENGTHS:
        c = model.cases[P]
        L = P + 3
        e.encode_mel(model.mel)
        nsp, rows = e.prefill_prompts([c["prompt"]], want_sot_logits=True)
        k, v = e.get_self_kv(0, L)
        dk, dv = float(np.abs(k - c["sk"]).max()), float(np.abs(v - c["sv"]).max())
        worst_k, worst_v = max(worst_k, dk), max(worst_v, dv)
        print("%s L %d: self K err %.3g, V err %.3g" % (route, L, dk, dv))
        assert dk < KV_BAR and dv < KV_BAR, (route, P, dk, dv)
        row_err = float(np.abs(rows[0] - c["sot_row"]).max())
        want = sr.no_speech_logprob(c["sot_row"], model.NS)
        print("%s L %d: sot row err %.3g, no-speech %.6f (oracle %.6f)" % (route, L, row_err, float(nsp[0]), float(want)))
        assert abs(float(nsp[0]) - float(want)) <= 2 * row_err + 1e-4, (route, P, float(nsp[0]), float(want), row_err)
        # the engine's value is log-softmax of the engine's own row
        assert abs(float(nsp[0]) - float(sr.no_speech_logprob(rows[0], model.NS))) <= 1e-4 + 1e-6 * float(np.abs(rows[0]).max())
        # off, tok and n_out: the first forced row is the oracle's first decision row, its decision made on an empty history
        lg, ch, _lp, nsp2 = e.decode_forced_timestamp_prompted([c["prompt"]], np.zeros((1, 0), dtype=np.int32))
        err = float(np.abs(lg[0, 0] - c["rows"][0]).max())
        worst_row = max(worst_row, err)
        assert err < KV_BAR and err < 0.2 * float(c["rows"][0].std()), (route, P, err, float(c["rows"][0].std()))
        assert int(ch[0, 0]) == tsr.decide(lg[0, 0], [], model.T, model.E)[0]
        assert float(nsp2[0]) == float(nsp[0])
    print("%s %s: worst self K err %.3g, V err %.3g, first row err %.3g" % (model.case.model_type, route, worst_k, worst_v, worst_row))


@pytest.mark.parametrize("batch", [1, 2, 5], ids=["gemv1", "gemv2", "clip_block5"])
@pytest.mark.parametrize("route", ["prefill", "step"])
def test_prompted_ids_against_the_oracle(model, route, batch):
    """Test 3: every case, alone (GEMV family), in pairs (GEMV family) and in fives (clip-block sequence) of different lengths."""
    e = model.engine(route)
    excused = EXCUSED.setdefault((route, batch), set())
    n = len(pr.LENGTHS)
    for i in range(n):
        Ps = [pr.LENGTHS[(i + 3 * j) % n] for j in range(batch)]  # lengths from different 64-key blocks side by side
        out = e.run_timestamp_prompted_batch([model.pcm] * batch, [model.cases[P]["prompt"] for P in Ps], max_new=BUDGET)
        for P, o in zip(Ps, out):
            if not model.ids_equal_or_tie(e, P, o["ids"], "%s batch %d" % (route, batch), batch):
                excused.add((model.case.model_type, P))
    print("%s %s batch %d: cases excused by the tie rule so far: %s" % (model.case.model_type, route, batch, sorted(excused)))
    assert len(excused) <= 2, excused  # at most 2 of the 16 cases (8 lengths, two models)


@pytest.mark.parametrize("route", ["prefill", "step"])
def test_ragged_batch(model, route):
    """Test 4: P = 0, 1, 61, 0, 223 side by side (clip-block sequence), on both routes (on the step-fed one the unprompted slots ride
    along and are set back). An unprompted clip is bit-equal to the unprompted call on the same input. A prompted clip against itself
    alone: the issue says "equals". Alone the clip is ENCODED alone too (one clip: the encoder's split-K residual GEMMs, other
    cross K/V in their last 16-bit place) and decodes through the GEMV family, so bits differ: the ids are equal or both pass the tie
    rule; and the no-speech values, each within the issue's bar of the oracle's (twice the error of its own sot row + 1e-4), agree
    within the sum of the two bars, with both row errors measured here at the stage level."""
    e = model.engine(route)
    Ps = [0, 1, 61, 0, 223]
    clips = [model.pcm] * 5
    prompts = [model.cases[P]["prompt"] if P else [] for P in Ps]
    got = e.run_timestamp_prompted_batch(clips, prompts, max_new=BUDGET)
    plain = e.run_timestamp_scores_batch(clips, max_new=BUDGET)
    for b, P in enumerate(Ps):
        if P == 0:
            assert got[b]["ids"] == plain[b]["ids"] and got[b]["no_speech_logprob"] == plain[b]["no_speech_logprob"], b
            assert np.array_equal(got[b]["token_logprob"], plain[b]["token_logprob"]) and got[b]["avg_logprob"] == plain[b]["avg_logprob"]
            assert got[b]["ended_eot"] == plain[b]["ended_eot"]
            continue
        alone = e.run_timestamp_prompted_batch([clips[b]], [prompts[b]], max_new=BUDGET)[0]
        if got[b]["ids"] != alone["ids"]:
            model.ids_equal_or_tie(e, P, got[b]["ids"], "ragged", 5)
            model.ids_equal_or_tie(e, P, alone["ids"], "ragged, alone", 1)
        assert np.isfinite(got[b]["token_logprob"]).all() and np.isfinite(got[b]["no_speech_logprob"])
    # the no-speech values, stage level (the rows they were taken from come back with them)
    e.encode_mel(np.stack([model.mel] * 5))
    nsp5, rows5 = e.prefill_prompts(prompts, want_sot_logits=True)
    for b, P in enumerate(Ps):
        if P == 0:
            assert nsp5[b] == 0.0 and not rows5[b].any()
            continue
        e.encode_mel(model.mel)
        nsp1, rows1 = e.prefill_prompts([prompts[b]], want_sot_logits=True)
        ref = model.cases[P]["sot_row"]
        err5, err1 = float(np.abs(rows5[b] - ref).max()), float(np.abs(rows1[0] - ref).max())
        want = float(sr.no_speech_logprob(ref, model.NS))
        print("%s ragged P %d: no-speech beside the others %.6f (row err %.3g), alone %.6f (row err %.3g), oracle %.6f"
              % (route, P, float(nsp5[b]), err5, float(nsp1[0]), err1, want))
        assert abs(float(nsp5[b]) - want) <= 2 * err5 + 1e-4 and abs(float(nsp1[0]) - want) <= 2 * err1 + 1e-4
        assert abs(float(nsp5[b]) - float(nsp1[0])) <= 2 * (err5 + err1) + 2e-4
    # all five unprompted through the prompted entry point: the unprompted call, bit for bit
    none = e.run_timestamp_prompted_batch(clips, [[]] * 5, max_new=BUDGET)
    for a, b in zip(none, plain):
        assert a["ids"] == b["ids"] and np.array_equal(a["token_logprob"], b["token_logprob"]) and a["no_speech_logprob"] == b["no_speech_logprob"]


@pytest.mark.parametrize("seq", ["split_k", "multi_branch"])
def test_the_other_step_sequences(model, seq):
    """The untouched step graphs behind the hand-over, verified for the sequences test 3 does not reach: AX_WHISPER_BATCHED_LN=0 (the
    split-K sequence, five clips) and the multi-branch clip-block step (22 clips: two branches). Prompted and unprompted slots mixed:
    ids against the oracle under the tie rule, unprompted clips bit-equal to the unprompted call of the same engine."""
    if seq == "split_k":
        e, batch = model.engine("prefill", AX_WHISPER_BATCHED_LN="0"), 5
        assert e.get_config_int("batched_ln") == 0
    else:
        e, batch = model.engine("prefill", max_batch=24), 22
        assert e.get_config_int("decode_branches") == 2
    Ps = [(0 if b % 4 == 2 else pr.LENGTHS[b % len(pr.LENGTHS)]) for b in range(batch)]
    clips = [model.pcm] * batch
    got = e.run_timestamp_prompted_batch(clips, [model.cases[P]["prompt"] if P else [] for P in Ps], max_new=BUDGET)
    plain = e.run_timestamp_scores_batch(clips, max_new=BUDGET)
    excused = 0
    for b, P in enumerate(Ps):
        if P == 0:
            assert got[b]["ids"] == plain[b]["ids"] and np.array_equal(got[b]["token_logprob"], plain[b]["token_logprob"]), (seq, b)
            assert got[b]["no_speech_logprob"] == plain[b]["no_speech_logprob"]
        elif not model.ids_equal_or_tie(e, P, got[b]["ids"], seq, batch):
            excused += 1
    print("%s %s: %d of %d prompted clips excused by the tie rule" % (model.case.model_type, seq, excused, sum(1 for P in Ps if P)))
    assert excused <= 2


def test_context_end(model):
    """Test 5: P = 223, no budget: the clip ends after exactly n_text_ctx - 1 - L ids (no case here decodes an early eot)."""
    e = model.engine("prefill")
    L = 226
    o = e.run_timestamp_prompted_batch([model.pcm], [model.cases[223]["prompt"]], max_new=0)[0]
    want = pr.greedy_prompted(model.orc, model.ck, model.cv, pr.context(model.cfg, model.cases[223]["prompt"], model.prefix))[0]
    assert len(want) == e.n_text_ctx - 1 - L == 221  # the oracle's loop under the same rule: no eot before the context end
    assert len(o["ids"]) == 221 and not o["ended_eot"]
    assert np.isfinite(o["token_logprob"]).all() and len(o["token_logprob"]) == 222 and np.isfinite(o["avg_logprob"])
    model.ids_equal_or_tie(e, 223, o["ids"][:BUDGET], "context end")


def test_bad_prompts_are_refused(model):
    e = model.engine("prefill")
    for bad in ([model.E], [model.T - 1], [e.n_vocab], [-1]):
        with pytest.raises(RuntimeError):
            e.run_timestamp_prompted_batch([model.pcm], [bad], max_new=2)
    ok = e.run_timestamp_prompted_batch([model.pcm], [[model.T + 10, 5, model.T + 20]], max_new=2)[0]  # timestamps are carried text
    assert len(ok["ids"]) == 2
    # a prompt longer than 223 ids: its last 223
    long_prompt = list(range(300, 340)) + model.cases[223]["prompt"]
    assert e.run_timestamp_prompted_batch([model.pcm], [long_prompt], max_new=BUDGET)[0]["ids"] == \
        e.run_timestamp_prompted_batch([model.pcm], [model.cases[223]["prompt"]], max_new=BUDGET)[0]["ids"]


def test_isolation(model):
    """Test 6: unprompted calls are what they were after prompted ones; long-form with both options off is run_long_windows."""
    e = model.engine("prefill")
    demo = model.pcm
    clips = [demo, demo[: len(demo) // 2]]
    f3 = lfr.make_file(demo, 3)
    before = (e.run_tokens_batch(clips, max_new=BUDGET), e.run_timestamp_scores_batch(clips, max_new=BUDGET), e.run_long_windows([f3], max_new=BUDGET, scores=True))
    e.run_timestamp_prompted_batch(clips, [model.cases[124]["prompt"], model.cases[1]["prompt"]], max_new=BUDGET)
    e.run_long_windows([f3], max_new=BUDGET, condition_on_previous_text=True)
    after = (e.run_tokens_batch(clips, max_new=BUDGET), e.run_timestamp_scores_batch(clips, max_new=BUDGET), e.run_long_windows([f3], max_new=BUDGET, scores=True))
    assert before[0] == after[0] and before[2] == after[2]
    for a, b in zip(before[1], after[1]):
        assert a["ids"] == b["ids"] and np.array_equal(a["token_logprob"], b["token_logprob"]) and a["no_speech_logprob"] == b["no_speech_logprob"]
    # both options off: the scored loop's log, bit for bit (an empty initial prompt is no prompt)
    off = e.run_long_windows([f3], max_new=BUDGET, initial_prompt_ids=[[]], condition_on_previous_text=False)  # the *Prompted entry point
    assert [[w[:9] for w in f] for f in off] == before[2] and all(w[9] == 0 for w in off[0])
    plain_log = e.run_long_windows([f3], max_new=BUDGET)
    assert [w[:6] for w in before[2][0]] == plain_log[0]


def _oracle_window(model, norm, seek, prompt):
    ck, cv = model.orc.encoder(lfr.window_of(norm, seek))
    return pr.greedy_prompted(model.orc, ck, cv, pr.context(model.cfg, prompt, model.prefix), max_new=BUDGET, want_logits=True)


def _check_carry_log(model, e, pcm, log, initial, condition=True):
    """One file's prompted log, window by window, against the Python rule: the seek chain, the prompt lengths, the ids under the
    oracle (tie rule per window; the state is carried on the engine's own ids, so an excused window does not cascade)."""
    norm = lfr.file_log_mel(pcm, model.case.dims["n_mels"])[0]
    all_ids, rs, seek, excused = list(initial), 0, 0, 0
    for w in log:
        s, wf, adv, ids = w[:4]
        assert s == seek and wf == min(3000, len(pcm) // 160 - s)
        prompt = pr.window_prompt(all_ids, rs)
        assert w[-1] == len(prompt), (s, w[-1], len(prompt))
        want, infos, rows = _oracle_window(model, norm, s, prompt)
        if ids != want:
            i = next((i for i in range(min(len(ids), len(want))) if ids[i] != want[i]), min(len(ids), len(want)))
            e.encode_mel(lfr.window_of(norm, s))
            if prompt:
                lg = e.decode_forced_timestamp_prompted([prompt], np.array([want[:i]], dtype=np.int32).reshape(1, i))[0]
            else:
                lg = e.decode_forced_timestamps(1, np.array([want[:i]], dtype=np.int32).reshape(1, i))[0]
            err = float(np.abs(lg[0, i] - rows[i]).max())
            assert infos[i]["margin"] < 2 * err + 1e-4, ("seek", s, "step", i, infos[i], err, want, ids)
            excused += 1
        assert not w[8]  # (no threshold: nothing is skipped)
        assert adv == lfr.split_window(ids, model.T, model.E, wf)[1]
        all_ids, rs = pr.carry(all_ids, rs, ids, model.T, model.E, condition_on_previous_text=condition, temperature=w[10] if len(w) > 10 else 0.0)
        seek += adv
    assert seek == len(pcm) // 160
    return excused


def test_long_form_carry(model):
    """Test 7: the 45 s and 75 s files, budget 12, conditioned on previous text, with and without an initial prompt (215 ids, so
    that the second window's prompt overflows 223); side by side and alone."""
    e = model.engine("prefill")
    files = [lfr.make_file(model.pcm, 3), lfr.make_file(model.pcm, 4)]
    initial = pr.case_prompt(model.E, 215, 7)
    for init in (None, [initial, []]):
        logs = e.run_long_windows(files, max_new=BUDGET, initial_prompt_ids=init, condition_on_previous_text=True)
        excused = 0
        for f in range(2):
            excused += _check_carry_log(model, e, files[f], logs[f], init[f] if init else [])
            alone = e.run_long_windows([files[f]], max_new=BUDGET, initial_prompt_ids=[init[f]] if init else None, condition_on_previous_text=True)[0]
            if [w[:4] + w[-1:] for w in alone] != [w[:4] + w[-1:] for w in logs[f]]:  # (ties apart: the alone log follows the rule too)
                assert _check_carry_log(model, e, files[f], alone, init[f] if init else []) + excused > 0
        lens = [[w[-1] for w in log] for log in logs]
        print("%s initial %s: prompt lengths %s, windows excused %d" % (model.case.model_type, bool(init), lens, excused))
        assert all(l[0] == (min(len(init[f]), pr.KEEP) if init else 0) for f, l in enumerate(lens))
        assert all(len(l) >= 2 and l[1] > 0 for l in lens)
        if init:
            assert lens[0][1] == pr.KEEP  # 215 + the first window's ids: truncated
    # the prompts matter: the second window's ids differ from the unconditioned loop's
    cond = e.run_long_windows(files[:1], max_new=BUDGET, condition_on_previous_text=True)[0]
    plain = e.run_long_windows(files[:1], max_new=BUDGET, scores=True)[0]
    assert cond[0][:4] == plain[0][:4] and cond[1][3] != plain[1][3]
    # initial prompt only, conditioning off: window 0 is prompted, the others are not
    only = e.run_long_windows(files[:1], max_new=BUDGET, initial_prompt_ids=[initial], condition_on_previous_text=False)[0]
    assert [w[-1] for w in only] == [215] + [0] * (len(only) - 1)
    _check_carry_log(model, e, files[0], only, initial, condition=False)


def test_long_form_prompt_reset_under_fallback(model):
    """Test 7, fallback: every window is kept at its last attempt; kept above 0.5 the next window starts without a prompt, kept at
    0.4 it is conditioned. (Ids do not depend on the audio on synthetic weights: the thresholds steer, as in test_gpu_sampling.py.)"""
    e = model.engine("prefill")
    f3 = lfr.make_file(model.pcm, 3)
    for temps, resets in (([0.0, 1.0], True), ([0.0, 0.4], False)):
        log = e.run_long_windows([f3], max_new=BUDGET, logprob_threshold=-1.0, temperatures=temps, seed=5, condition_on_previous_text=True)[0]
        kept = [w for w in log if w[12]]
        assert len(kept) >= 2 and all(w[9] == 1 for w in kept) and len(log) == 2 * len(kept)
        all_ids, rs = [], 0
        for w in log:
            assert w[-1] == len(pr.window_prompt(all_ids, rs)), (temps, w[0], w[9])  # every attempt of a window: the same prompt
            if w[12]:
                all_ids, rs = pr.carry(all_ids, rs, w[3], model.T, model.E, skipped=w[8], temperature=w[10])
        assert all(w[-1] == 0 for w in log) == resets
        if not resets:
            assert kept[1][-1] > 0
    # the ratio branch (test_gpu_sampling.py's construction: any text compresses by more than 0), and the ids drawn under a prompt:
    # the reference sampler on the engine's own rows (the window teacher-forced under its prompt) draws the engine's ids
    import sample_reference as smp

    seed, temps = 5, [0.0, 0.4]
    log = e.run_long_windows([f3], max_new=BUDGET, compression_ratio_threshold=0.0, temperatures=temps, seed=seed, condition_on_previous_text=True)[0]
    assert [w[12] for w in log] == [False, True] * (len(log) // 2) and all(w[11] > 0.0 for w in log)
    norm = lfr.file_log_mel(f3, model.case.dims["n_mels"])[0]
    all_ids, rs, checked, near = [], 0, 0, 0
    for w in log:
        prompt = pr.window_prompt(all_ids, rs)
        assert w[-1] == len(prompt)
        if w[12] and prompt:
            ids, t = w[3], w[10]
            stream = (w[0] & 0xFFFFFFFF) | ((0 * 16 + w[9]) << 32)  # (seek, file id * 16 + attempt)
            e.encode_mel(lfr.window_of(norm, w[0]))
            lg = e.decode_forced_timestamp_prompted([prompt], np.array([ids], dtype=np.int32).reshape(1, len(ids)))[0]
            for i in range(len(ids)):
                c, _lp, info = smp.sample(lg[0, i], ids[:i], model.T, model.E, t, stream, seed)
                near += bool(info["near_tie"])
                assert c == ids[i] or info["near_tie"], (w[0], i, c, ids[i], info["key_gap"])
                checked += 1
        if w[12]:
            all_ids, rs = pr.carry(all_ids, rs, w[3], model.T, model.E, skipped=w[8], temperature=w[10])
    print("%s: %d sampled decisions under a prompt checked, %d near ties" % (model.case.model_type, checked, near))
    assert checked >= BUDGET and near <= 1


def test_two_engines_on_one_device(model, monkeypatch):
    """Test 8: prompted results sharded over two engines (3 + 2 clips) equal one engine's (five at once) — other decode sequences,
    so: or both pass the tie rule."""
    e = model.engine("prefill")
    Ps = [1, 61, 124, 223, 62]
    clips, prompts = [model.pcm] * 5, [model.cases[P]["prompt"] for P in Ps]
    one = e.run_timestamp_prompted_batch(clips, prompts, max_new=BUDGET)
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    two = model.lib.Whisper(model.case.model_type, model.case.root, "zh", devices=[0, 0], max_batch=4)
    try:
        assert two.get_config_int("n_devices") == 2
        got = two.run_timestamp_prompted_batch(clips, prompts, max_new=BUDGET)
    finally:
        two.close()
    for P, a, b in zip(Ps, one, got):
        if a["ids"] != b["ids"]:
            model.ids_equal_or_tie(e, P, a["ids"], "one engine", 5)
            model.ids_equal_or_tie(e, P, b["ids"], "two engines", 2)


def test_cli_prompt_flags(model, tmp_path):
    """Test 9: --long --condition_on_previous_text --prompt_ids prints the lines of the Python-side result."""
    e = model.engine("prefill")
    cli = os.path.join(os.path.dirname(model.lib.LIB_PATH), "whisper_cli")
    wav = str(tmp_path / "f45.wav")
    pcm16 = np.clip(np.round(lfr.make_file(model.pcm, 3) * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(pcm16.tobytes())
    prompt = model.cases[61]["prompt"]
    args = [cli, "-w", wav, "-t", model.case.model_type, "-p", model.case.root, "--language", "zh", "--long"]
    r = subprocess.run(args + ["--condition_on_previous_text", "--prompt_ids", ",".join(str(t) for t in prompt)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    text = r.stdout.decode("utf-8", "replace").split("\nResult: ", 1)[1]
    want = e.run_long_text(wav, initial_prompt_ids=prompt, condition_on_previous_text=True)
    assert want and text.startswith(want + "\n")
    assert want != e.run_long_text(wav)
    segs = e.run_long_scored(pcm16.astype(np.float32) / np.float32(32768.0), initial_prompt_ids=prompt, condition_on_previous_text=True)
    lines = re.findall(r"(?m)^\[\d\d+:\d\d\.\d\d\d --> \d\d+:\d\d\.\d\d\d\] ", text)
    assert len(lines) == len(segs) >= 1
    bad = subprocess.run(args[:-1] + ["--condition_on_previous_text"], capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"--long" in bad.stderr
