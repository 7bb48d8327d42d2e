"""CPU: prompt conditioning's host side (DESIGN.md "Prompt conditioning").

The carry rule: AX_WHISPER_CarryPrompt against tests/prompt_reference.carry on crafted windows. The prompt cases the GPU tests
decode: for every prompt length and both models the oracle's prompted ids differ from its unprompted ids, so a decode that ignored
its prompt cannot pass the GPU id test, and the case's decision margins leave room for the 16-bit storage error."""
import numpy as np
import pytest

import prompt_reference as pr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

E, T = 50257, 50364
W = 3000


def _ts(sec):
    return T + int(round(sec / 0.02))


WINDOWS = {
    # two closed segments, then an open one whose ids are dropped
    "cuts": [_ts(0.0), 11, 12, _ts(2.0), _ts(2.0), 13, _ts(4.5), _ts(4.5), 14, 15],
    # the ids end in a single timestamp: the last segment closes there
    "single_end": [_ts(0.0), 11, _ts(1.0), _ts(1.0), 12, 13, _ts(7.0)],
    "no_cuts": [_ts(0.0), 11, 12, 13, _ts(3.0)],
    "no_cuts_no_timestamp": [11, 12, 13],
    # the middle segment has no text id: it adds nothing
    "empty_text_segment": [_ts(0.0), 11, _ts(1.0), _ts(1.0), _ts(2.0), _ts(2.0), 12, _ts(3.0), _ts(3.0)],
    "only_timestamps": [_ts(0.0), _ts(0.0)],
    "empty": [],
}


def _check(built_lib, all_ids, rs, win, **kw):
    want = pr.carry(all_ids, rs, win, T, E, **kw)
    got = built_lib.carry_prompt(all_ids, rs, win, T, E, W, keep=pr.KEEP, **kw)
    assert (got[0], got[1]) == want, (all_ids, rs, win, kw, got, want)
    assert got[2] == len(pr.window_prompt(*want))
    return want


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_carry_appends_the_emitted_segments(built_lib, name):
    win = WINDOWS[name]
    all_ids, rs = _check(built_lib, [5, 6, 7], 0, win)
    expect = {"cuts": win[:7], "single_end": win, "no_cuts": win, "no_cuts_no_timestamp": win,
              "empty_text_segment": win[:3] + win[5:8], "only_timestamps": [], "empty": []}[name]
    assert all_ids == [5, 6, 7] + expect and rs == 0
    # the ranges are the segments AX_WHISPER_SplitWindow emits
    segs, _ = built_lib.split_window(win, T, E, W)
    assert len(segs) == len(pr.segment_ranges(win, T, E))
    for (lo, hi), (_s, _e, tb, te) in zip(pr.segment_ranges(win, T, E), segs):
        assert lo <= tb < te <= hi


def test_carry_skipped_window_appends_nothing(built_lib):
    assert _check(built_lib, [5, 6], 0, WINDOWS["cuts"], skipped=True) == ([5, 6], 0)
    # ... but the reset still applies
    assert _check(built_lib, [5, 6], 0, WINDOWS["cuts"], skipped=True, temperature=0.6) == ([5, 6], 2)


def test_carry_prompt_reset_above_half(built_lib):
    win = WINDOWS["no_cuts"]
    assert _check(built_lib, [5], 0, win, temperature=0.4)[1] == 0
    assert _check(built_lib, [5], 0, win, temperature=0.5)[1] == 0  # strictly above
    assert _check(built_lib, [5], 0, win, temperature=0.6)[1] == 1 + len(win)
    # float32 on both sides: the fallback list's 0.6 is float32(0.6)
    assert _check(built_lib, [5], 0, win, temperature=float(np.float32(0.2) * 3))[1] == 1 + len(win)


def test_carry_condition_off_resets_every_window(built_lib):
    all_ids, rs = _check(built_lib, [5, 6, 7], 0, WINDOWS["cuts"], condition_on_previous_text=False)
    assert rs == len(all_ids) and pr.window_prompt(all_ids, rs) == []


def test_carry_overflow_keeps_the_last_223(built_lib):
    all_ids, rs = list(range(100, 300)), 10
    win = [_ts(0.0)] + list(range(1000, 1100)) + [_ts(9.0)]
    all_ids, rs = _check(built_lib, all_ids, rs, win)
    assert len(all_ids) == 302 and rs == 10
    p = pr.window_prompt(all_ids, rs)
    assert len(p) == pr.KEEP and p == all_ids[-pr.KEEP:]
    # a second window: the state keeps growing, the prompt stays the tail
    all_ids, rs = _check(built_lib, all_ids, rs, WINDOWS["single_end"])
    assert pr.window_prompt(all_ids, rs)[-len(WINDOWS["single_end"]):] == WINDOWS["single_end"]


def test_carry_rejects_bad_arguments(built_lib):
    with pytest.raises(RuntimeError):
        built_lib.carry_prompt([1, 2], 3, [], T, E, W)  # reset_since beyond the list


@pytest.fixture(scope="module", params=pr.MODELS, ids=[m[0] for m in pr.MODELS])
def oracle_case(request, oracle_mod, tmp_path_factory):
    model_type, seed, dtype = request.param
    case = ModelCase(tmp_path_factory.mktemp("pr_" + model_type), model_type, seed, dtype=dtype)
    orc = case.oracle_bf16
    mel = oracle_mod.log_mel(load_demo_pcm(), case.dims["n_mels"])[0]
    ck, cv = orc.encoder(mel)
    prefix = orc.sot_seq("zh")[:3]
    plain = tsr.greedy_ts(orc, ck, cv, prefix, max_new=pr.N_DECISIONS)[0]
    return model_type, orc, ck, cv, prefix, plain


def test_greedy_prompted_without_a_prompt_is_greedy_ts(oracle_case):
    _, orc, ck, cv, prefix, plain = oracle_case
    assert pr.context(orc.cfg, [], prefix) == list(prefix)
    assert pr.greedy_prompted(orc, ck, cv, list(prefix), max_new=pr.N_DECISIONS)[0] == plain


@pytest.mark.parametrize("P", pr.LENGTHS)
def test_prompt_cases_change_the_ids(oracle_case, P):
    """What makes the GPU id test meaningful: under every case's prompt the oracle decodes other ids than without it."""
    model_type, orc, ck, cv, prefix, plain = oracle_case
    sd, prompt, ids, infos = pr.find_case(orc, ck, cv, prefix, P)
    assert sd == (3 if (model_type, P) == ("micro", 125) else 0)  # checked on this code base
    assert len(pr.context(orc.cfg, prompt, prefix)) == P + 4
    assert min(i["margin"] for i in infos[:pr.N_DECISIONS]) >= pr.MARGIN
    assert ids != plain, (model_type, P, ids)
