"""CPU: the float64 reference and the error bound of the fused vocabulary log-probability kernel (tests/vocab_logprob_reference.py)
on the inputs of the GPU test: a numpy emulation of the kernel's rounding stays inside the bound, two deliberately wrong variants
(column eot inside the sum; the ragged last tile dropped) land outside it, and the Python statement of the tiling is the library's."""
import numpy as np
import pytest

import vocab_logprob_reference as vr
import word_reference as wr


@pytest.fixture(scope="module", params=wr.MODELS, ids=[m[0] for m in wr.MODELS])
def model(request):
    import modelgen

    model_type, seed, dtype = request.param
    dims = modelgen.DIMS[model_type]
    return model_type, modelgen.make_config(model_type, dims), modelgen.realistic_weights(dims, seed, dtype=dtype), vr.dtype_of(dtype)


def test_plan_is_the_librarys(built_lib):
    for d in (128, 256, 384, 512, 768, 1024, 1280):
        for rows in (1, 17, 64, 65, 200, 1760, 14080):
            assert built_lib.vocab_logprob_plan(d, rows, 51864) == vr.plan(d, rows, 51864), (d, rows)
    rt, n_splits, split_cols = vr.plan(768, 1760, 51864)
    assert rt == 32 and split_cols % vr.CHUNK == 0 and (n_splits - 1) * split_cols < 51864 <= n_splits * split_cols
    with pytest.raises(ValueError):
        built_lib.vocab_logprob_plan(192, 4, 51864)
    assert built_lib.load_library().AX_WHISPER_VocabLogProbRows(None, None, 1, None, None, 1) == -1


@pytest.mark.parametrize("rows", vr.ROWS)
def test_emulation_inside_the_bound_wrong_variants_outside(model, rows):
    model_type, cfg, weights, dt = model
    d, eot = int(cfg["n_text_state"]), int(cfg["eot"])
    W, g, b = weights["decoder.token_embedding.weight"], weights["decoder.ln.weight"], weights["decoder.ln.bias"]
    assert eot % 16 != 0 and W.shape[0] > eot  # the last column tile is ragged, and column eot exists to be left out
    x, ids, roles = vr.case(weights, cfg, rows, seed=rows)
    ref = vr.reference(x, g, b, W, ids, eot)
    bnd = vr.bound(ref, W, ids, eot, dt, "fused", vr.chain("fused", d, rows, eot))
    assert np.isfinite(ref["lp"]).all() and np.isfinite(bnd).all() and (bnd > 0).all()
    err = np.abs(vr.emulate(x, g, b, W, ids, eot, dt).astype(np.float64) - ref["lp"])
    print(f"{model_type} rows {rows}: emulation error / bound, worst row {float((err / bnd).max()):.3f}; bound {float(bnd.min()):.2e} .. {float(bnd.max()):.2e}")
    assert (err <= bnd).all(), (np.argmax(err / bnd), err.max())
    # the ids the issue names are there
    _, n_splits, split_cols = vr.plan(d, rows, eot)
    assert ids[0] == 0
    if rows >= 17:
        assert {eot - 1, eot // 16 * 16, split_cols - 1, (n_splits - 1) * split_cols} <= set(ids.tolist())
        assert ref["lp"][roles["dominant"]] > -1e-2                                           # lp ~ 0
        assert np.allclose(ref["y"][roles["zero"]], np.asarray(b, dtype=np.float64), atol=0)  # the bias alone
        for variant, row in (("include_eot", roles["eot_heavy"]), ("drop_ragged", roles["dominant"])):
            bad = np.abs(vr.emulate(x, g, b, W, ids, eot, dt, variant=variant).astype(np.float64) - ref["lp"])
            assert bad[row] > bnd[row], (variant, bad[row], bnd[row])
    # the rows route's own bound is the tighter one: no 16-bit narrowing of the activations
    assert (vr.bound(ref, W, ids, eot, dt, "rows", 2) <= bnd).all()
