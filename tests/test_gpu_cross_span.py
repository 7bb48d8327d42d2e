"""GPU: cross-attention over each slot's own audio span (AX_WHISPER_CROSS_SPAN=audio; DESIGN.md "Cross-attention spans").

  kernel alone   cross_span_attention (plan kernel + span kernel, query from a buffer) against float64 softmax(q . K^T / 8) . V over
                 the first `span` keys of each slot, K and V as the handle stores them (get_cross_kv; on an FP8 handle the
                 dequantised codes, so the kernel and not the quantiser is measured). Tolerance: the per-element bound
                 decode_kernel_reference.softmax_expect derives for the single-query kernels, with the span kernel's own chain of
                 rescales (a wave's blocks, the wave merge, up to six pieces), plus the output pair's rounding. Spans come from
                 {1, 63, 64, 65, 300, 1499, 1500}; a call of 16 slots holds all seven, a call of 5 a one-key span, a block edge on each
                 side and a full clip plus one drawn; a call of 3 slots cannot hold those four kinds at once, so that case runs
                 three calls that together hold all seven values.
  bookkeeping    spans follow min(1500, ceil(samples / 320) + margin) through run_tokens_batch and through a slot refill
  full spans     with a margin of 1500 frames every span is 1500 and the ids are the oracle's, as test_gpu_parity.py asks of a
                 default handle
"""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

import cross_fp8_reference as R
from conftest import ModelCase, assert_ids_equal_or_tie, load_demo_pcm
from decode_kernel_reference import pair_err, softmax_expect

pytestmark = pytest.mark.gpu
SPANS = (1, 63, 64, 65, 300, 1499, 1500)
N_SLOTS = 16
CHAIN = 24 // 4 + 6 + 2  # a wave's blocks of a 24-block piece, the pieces of a (slot, head), the wave merge and the division


def span_of(n_samples, margin=100):
    return min(1500, -(-n_samples // 320) + margin)


@pytest.fixture(scope="module", params=["BF16", "F16"], ids=["bf16", "fp16"])
def case(request, tmp_path_factory, oracle_mod):
    return ModelCase(tmp_path_factory.mktemp("span_" + request.param), "micro", 11, dtype=request.param)


@pytest.fixture(scope="module", params=["h16", "fp8"])
def loaded(request, built_lib, case):
    """(handle, K, V): 16 slots encoded once, their stored K and V as float64 [slot][L][1500][d]."""
    from make_model_goldens_inputs import synth_mel

    e = built_lib.Whisper("micro", case.root, "zh", device=0, max_batch=N_SLOTS, cross_span="audio", cross_kv=request.param)
    e.encode_mel(np.stack([synth_mel(40 + i, 80, 3000 - 97 * i) + np.float32(0.5 * (i % 5)) for i in range(N_SLOTS)]))
    ks, vs = [], []
    for slot in range(N_SLOTS):
        if request.param == "fp8":
            kc, vc, sc = e.get_cross_kv_fp8(slot)
            L, T, d = kc.shape
            k, v = R.dequantize(kc, sc[:, :, 0, :].reshape(L, d)), R.dequantize(vc, sc[:, :, 1, :].reshape(L, d))
        else:
            k, v = e.get_cross_kv(slot)
        ks.append(np.asarray(k, dtype=np.float64))
        vs.append(np.asarray(v, dtype=np.float64))
    yield e, np.stack(ks), np.stack(vs)
    e.close()


@pytest.mark.parametrize("n", [3, 5, 16])
def test_kernel_against_float64(loaded, case, n):
    e, K, V = loaded
    dt = "f16" if case.dtype == "F16" else "bf16"
    d, H = e.n_text_state, e.n_text_state // 64
    rng = np.random.default_rng(1234 + n)
    assert e.get_config_int("cross_span") == 1
    worst = 0.0
    for call in range(3 if n == 3 else 1):
        if n == 3:
            spans = [SPANS[(3 * call + i) % len(SPANS)] for i in range(n)]
        else:  # a one-key span, a block edge on each side and a full clip in every call, the rest drawn
            must = [1, 63, 65, 1500] if n == 5 else list(SPANS)
            spans = [int(s) for s in rng.permutation(must + list(rng.choice(SPANS, n - len(must))))]
        layer = call % e.n_text_layer
        q = rng.standard_normal((n, d)).astype(np.float32) * np.float32(2.0)
        n0 = e.get_config_int("cross_span_launches")
        out = e.cross_span_attention(layer, q, spans)
        assert e.get_config_int("cross_span_launches") == n0 + 1
        for b in range(n):
            for h in range(H):
                c = slice(64 * h, 64 * h + 64)
                o, err, _, _ = softmax_expect(q[b, c].astype(np.float64), np.zeros(64), K[b, layer, :spans[b], c], V[b, layer, :spans[b], c], CHAIN)
                bound = err + pair_err(np.abs(o) + err, dt) + 2.0 ** -24 * np.abs(o)  # (hi + lo is summed in fp32 on the host)
                ratio = float((np.abs(out[b, c] - o) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (n, call, b, h, spans[b], ratio, float(np.abs(out[b, c] - o).max()))
    print(f"span kernel, {n} slots: worst error / bound {worst:.3f}")


def test_spans_follow_the_clips(built_lib, micro_case):
    import modelgen

    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=4, cross_span="audio")
    plain = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=4)
    try:
        assert e.get_config_int("cross_span") == 1 and e.get_config_int("cross_span_margin") == 100
        assert list(e.cross_spans()) == [1500] * 4  # nothing known yet
        clips = [modelgen.synth_clip(i, n) for i, n in enumerate((8000, 48000, 480000, 160001))]
        n0 = e.get_config_int("cross_span_launches")
        got = e.run_tokens_batch(clips, max_new=6)
        assert list(e.cross_spans()) == [span_of(len(c)) for c in clips] == [125, 250, 1500, 601]
        assert e.get_config_int("cross_span_launches") > n0 and all(len(g) == 6 for g in got)
        assert plain.run_tokens_batch(clips, max_new=6) is not None
        assert plain.get_config_int("cross_span") == 0 and plain.get_config_int("cross_span_launches") == 0
        with pytest.raises(RuntimeError):
            plain.cross_spans()
        # a 4-slot stream: the long clip of slot 0 finishes, a short one takes its place
        e.stream_open(4)
        try:
            for sl, c in enumerate((clips[2], clips[0], clips[1], clips[3])):
                e.stream_admit(sl, c, 4 if sl == 0 else 40)
            done = []
            while 0 not in done:
                done += list(e.stream_step(2))
            assert list(e.cross_spans()) == [1500, 125, 250, 601]
            e.stream_collect(0)
            e.stream_admit(0, clips[1], 4)
            done = []
            while 0 not in done:
                done += list(e.stream_step(2))
            assert list(e.cross_spans()) == [250, 125, 250, 601]
            assert len(e.stream_collect(0)) == 4
        finally:
            e.stream_close()
    finally:
        e.close()
        plain.close()


def test_full_spans_give_the_oracles_ids(built_lib, micro_case, oracle_mod, monkeypatch):
    monkeypatch.setenv("AX_WHISPER_CROSS_SPAN_MARGIN", "1500")
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=4, cross_span="audio")
    try:
        pcm = load_demo_pcm()
        clips = [pcm, pcm[8000:], 0.5 * pcm, pcm[:48000]]
        n0 = e.get_config_int("cross_span_launches")
        got = e.run_tokens_batch(clips, max_new=10)
        assert list(e.cross_spans()) == [1500] * 4 and e.get_config_int("cross_span_launches") > n0
        mels = [oracle_mod.log_mel(c, 80)[0] for c in clips]
        for b, mel in enumerate(mels):
            ck, cv = micro_case.oracle_bf16.encoder(mel)
            ids, lg = micro_case.oracle_bf16.greedy(ck, cv, "zh", max_new=10, want_logits=True)
            assert_ids_equal_or_tie(e, mel, got[b], ids, lg, f"clip {b}", batch_mels=np.stack(mels), slot=b)
    finally:
        e.close()
