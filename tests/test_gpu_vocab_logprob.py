"""GPU: the fused vocabulary log-probability kernel alone (csrc/vocab_logprob.hip through AX_WHISPER_VocabLogProbRows) on micro bf16
(d = 128) and miniturbo fp16 (d = 256) with modelgen.realistic_weights, at 1, 17, 64, 65 and 200 rows: every output against float64
within the bound derived in tests/vocab_logprob_reference.py, two runs bit-equal, and the rows route on the same inputs inside its
own bound. The inputs (tests/vocab_logprob_reference.case) hold ids at 0, at eot - 1, in the ragged tile and at both ends of a
vocabulary split, a row whose target dominates, a zero row and a row whose mass sits on column eot.

Measured on MI355X, worst error / bound over all rows: fused 0.59 (micro), 0.54 (miniturbo); rows 0.005 (micro), 0.003 (miniturbo);
worst absolute error: fused 6.1e-1 / 1.3e-1 (on the rows steered to one column, logits of several hundred), rows 5.1e-5 / 5.1e-5.
The other row tiles with two chunks per split: micro 330 rows 0.42 of the bound, w1024 170 rows 0.09, w1280 fp16 100 rows 0.08."""
import types

import numpy as np
import pytest

import vocab_logprob_reference as vr
import word_reference as wr
from conftest import ModelCase

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=wr.MODELS, ids=[m[0] for m in wr.MODELS])
def model(request, tmp_path_factory, built_lib, oracle_mod):
    model_type, seed, dtype = request.param
    case = ModelCase(tmp_path_factory.mktemp("vlp_" + model_type), model_type, seed, dtype=dtype, kind="realistic")
    eng = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=1)
    w = case.weights
    yield types.SimpleNamespace(case=case, cfg=case.cfg, eng=eng, dt=vr.dtype_of(dtype), W=w["decoder.token_embedding.weight"],
                                g=w["decoder.ln.weight"], b=w["decoder.ln.bias"])
    eng.close()


@pytest.mark.parametrize("rows", vr.ROWS)
def test_both_routes_against_float64(model, rows):
    m = model
    d, eot = int(m.cfg["n_text_state"]), int(m.cfg["eot"])
    x, ids, _ = vr.case(m.case.weights, m.cfg, rows, seed=rows)
    ref = vr.reference(x, m.g, m.b, m.W, ids, eot)
    fused = m.eng.vocab_logprob_rows(x, ids, "fused")
    again = m.eng.vocab_logprob_rows(x, ids, "fused")
    by_rows = m.eng.vocab_logprob_rows(x, ids, "rows")
    for route, got in (("fused", fused), ("rows", by_rows)):
        bnd = vr.bound(ref, m.W, ids, eot, m.dt, route, vr.chain(route, d, rows, eot))
        err = np.abs(got.astype(np.float64) - ref["lp"])
        print(f"{m.case.model_type} rows {rows} {route}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bnd).max()):.3f}")
        assert np.isfinite(got).all()
        assert (err <= bnd).all(), (route, int(np.argmax(err / bnd)), float(err.max()))
    assert np.array_equal(fused.view(np.uint32), again.view(np.uint32))


# The other instantiations and the fold across chunks. At 203 one-chunk splits (the cases above) a workgroup sweeps its row tile
# once; from 6 row tiles on a split holds two 256-column chunks and the online (max, sum) runs across them. 32 rows per tile is the
# kernel of d = 768 and 1024, 16 rows that of d = 1280: w1024 and w1280 are the full widths at reduced depth (N(0, 0.02) weights: the
# kernel alone does not care what the layers hold).
WIDE = (("micro", 11, "BF16", "realistic", 330, 64), ("w1024", 5, "BF16", "benign", 170, 32), ("w1280", 6, "F16", "benign", 100, 16))


@pytest.mark.parametrize("model_type,seed,dtype,kind,rows,row_tile", WIDE, ids=[w[0] for w in WIDE])
def test_other_row_tiles_and_two_chunks_per_split(built_lib, oracle_mod, tmp_path, model_type, seed, dtype, kind, rows, row_tile):
    case = ModelCase(tmp_path, model_type, seed, dtype=dtype, kind=kind)
    d, eot = int(case.cfg["n_text_state"]), int(case.cfg["eot"])
    rt, n_splits, split_cols = vr.plan(d, rows, eot)
    assert rt == row_tile and split_cols == 2 * vr.CHUNK and rows % rt != 0
    W, g, b = (case.weights[k] for k in ("decoder.token_embedding.weight", "decoder.ln.weight", "decoder.ln.bias"))
    x, ids, _ = vr.case(case.weights, case.cfg, rows, seed=rows)
    ref = vr.reference(x, g, b, W, ids, eot)
    eng = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=1)
    try:
        fused, again = eng.vocab_logprob_rows(x, ids, "fused"), eng.vocab_logprob_rows(x, ids, "fused")
    finally:
        eng.close()
    bnd = vr.bound(ref, W, ids, eot, vr.dtype_of(dtype), "fused", vr.chain("fused", d, rows, eot))
    err = np.abs(fused.astype(np.float64) - ref["lp"])
    print(f"{model_type} rows {rows} (tile {rt}, {n_splits} splits of 2 chunks): worst error {float(err.max()):.3e}, worst error / bound {float((err / bnd).max()):.3f}")
    assert np.isfinite(fused).all() and (err <= bnd).all(), (int(np.argmax(err / bnd)), float(err.max()))
    assert np.array_equal(fused.view(np.uint32), again.view(np.uint32))


def test_refusals(model):
    m = model
    d, eot = int(m.cfg["n_text_state"]), int(m.cfg["eot"])
    x = np.zeros((2, d), dtype=np.float32)
    with pytest.raises(RuntimeError):
        m.eng.vocab_logprob_rows(x, [0, eot], "fused")  # not below eot
    with pytest.raises(RuntimeError):
        m.eng.vocab_logprob_rows(x, [-1, 0], "rows")
    assert m.eng.get_config_int("word_logprob") == 0
