"""CPU: the float64 teacher-forced decoder of tests/word_reference.py against the oracle, and the pieces of find_alignment that
need no engine. The forward is what the GPU word tests measure the engine against, so it is proven here first: its logits on a forced
id list are the oracle's (pure fp32) to fp32-against-fp64 rounding."""
import numpy as np
import pytest

import word_reference as wr
from conftest import ModelCase, load_demo_pcm

# measured here against the oracle: 5.2e-7 (micro) and 7.9e-7 (miniturbo) on logits of magnitude ~1; the bound leaves a factor
# of five for another libm or thread count
FORWARD_TOL = 4e-6


@pytest.fixture(scope="module", params=wr.MODELS, ids=[m[0] for m in wr.MODELS])
def oracle_case(request, oracle_mod, tmp_path_factory):
    model_type, seed, dtype = request.param
    case = ModelCase(tmp_path_factory.mktemp("wr_" + model_type), model_type, seed, dtype=dtype)
    orc = case.oracle_fp32
    mel = oracle_mod.log_mel(load_demo_pcm(), case.dims["n_mels"])[0]
    ck, cv = orc.encoder(mel)
    return case, orc, ck, cv


def test_forward_logits_are_the_oracles(oracle_case):
    case, orc, ck, cv = oracle_case
    forced = wr.case_ids(int(case.cfg["eot"]), 0, 12)
    ids, lg = orc.greedy(ck, cv, "zh", forced=forced, want_logits=True)
    sot = orc.sot_seq("zh")
    logits, q = wr.decoder_forward(case.cfg, case.weights, ck, cv, sot + forced)
    assert q.shape == (int(case.cfg["n_text_layer"]), len(forced) + 4, int(case.cfg["n_text_state"]))
    n = lg.shape[0]
    assert n == len(forced) + 1
    err = float(np.abs(logits[3: 3 + n] - lg).max())
    print(f"{case.model_type}: float64 forward against the oracle {err:.3e}, logits up to {float(np.abs(lg).max()):.3f}")
    assert err < FORWARD_TOL


def test_find_alignment_shapes_and_rules(oracle_case):
    case, orc, ck, cv = oracle_case
    cfg = case.cfg
    lang = orc.sot_seq("zh")[1]
    assert wr.find_alignment(cfg, case.weights, ck, cv, [], 3000, lang) is None  # no ids: no words
    with pytest.raises(ValueError):
        wr.find_alignment(cfg, case.weights, ck, cv, [1] * (int(cfg["n_text_ctx"]) - 4), 3000, lang)
    ids = wr.case_ids(int(cfg["eot"]), 1, 6)
    for frames in (100, 7, 5):  # F = 50; F = 3 and F = 2: the median filter is skipped
        ref = wr.find_alignment(cfg, case.weights, ck, cv, ids, frames, lang)
        F = frames // 2
        assert ref["matrix"].shape == (len(ids) + 5, F) and ref["jump"].shape == (len(ids) + 1,)
        assert ref["jump"][0] == 0 and (np.diff(ref["jump"]) >= 0).all() and ref["jump"][-1] < F
        assert (ref["token_logprob"] < 0).all()
        # every head and frame was normalised over all L rows: the head mean keeps a zero column mean where no median moved it
        if F <= 3:
            assert np.abs(ref["matrix"].mean(0)).max() < 1e-9
    other = wr.find_alignment(cfg, case.weights, ck, cv, ids, 100, lang, heads=[(0, 0)])
    assert not np.allclose(other["matrix"], wr.find_alignment(cfg, case.weights, ck, cv, ids, 100, lang)["matrix"])


def test_median_filter_is_reflect_padded():
    z = np.arange(10.0)[None] ** 2
    got = wr.median7(z)[0]
    pad = np.concatenate([z[0, 3:0:-1], z[0], z[0, -2:-5:-1]])
    assert np.array_equal(got, [np.sort(pad[i: i + 7])[3] for i in range(10)])
    assert np.array_equal(wr.median7(z[:, :3]), z[:, :3])


@pytest.mark.parametrize("model", wr.MODELS, ids=[m[0] for m in wr.MODELS])
def test_every_model_has_an_admissible_case(model, oracle_mod, tmp_path_factory):
    """What makes the GPU jump comparison of tests/test_gpu_words.py meaningful: on the models it runs (realistic weights) some seed
    of case_ids gives a float64 matrix whose jumps do not move under perturbations of the size of the engine's measured error."""
    model_type, seed, dtype = model
    case = ModelCase(tmp_path_factory.mktemp("wra_" + model_type), model_type, seed, dtype=dtype, kind="realistic")
    orc = case.oracle_bf16
    demo = load_demo_pcm()
    found = []
    for pcm in (demo, demo[16000:32000]):
        ck, cv = orc.encoder(oracle_mod.log_mel(pcm, case.dims["n_mels"])[0])
        hit = wr.find_case(case.cfg, case.weights, ck, cv, min(len(pcm) // 160, 3000), orc.sot_seq("zh")[1], wr.MATRIX_EPS[model_type])
        if hit:
            found.append(hit[0])
    print(f"{model_type}: admissible seeds {found}")
    assert found
