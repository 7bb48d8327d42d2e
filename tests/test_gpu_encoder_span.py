"""GPU: the encoder over each clip's own audio span (AX_WHISPER_CROSS_SPAN=encoder; DESIGN.md "Encoder spans").

  kernel alone   encoder_span_attention (work list + encoder_attention_span_kernel) against float64 softmax(q k^T / 8) v over the
                 first `span` keys for the query rows below the span, both builds, both block heights, 1 / 3 / 5 clips whose spans
                 together are {1, 63, 64, 65, 127, 128, 129, 300, 1499, 1500}. Every row of q, k, v at or beyond a clip's span is NaN
                 (the engine fills V^T's padding columns with NaN patterns as well). Bound: encoder_kernel_reference.attention_expect
                 applied to `span` keys in ceil(span / 64) tiles. Output rows at or beyond the span are exactly zero.
  whole pass     get_cross_kv of a truncated pass against a float64 encoder over each clip's first `span` frames, held to the default
                 handle's full pass against the same float64 encoder over 1500 frames
  routing        with a margin of 1500 frames a 5-clip call runs a truncated pass (of all 1500 rows) and gives the oracle's ids; a
                 2-clip call and a prompted call leave the counter alone and give the default handle's ids; a truncated slot holds
                 zeros behind its span in get_cross_kv and refuses the stage-level readers of all frames, beam search among them
  FP8            codes and scales from the frames below the span alone, after a louder full-length clip in the same slots
  regression     full and audio handles: no truncated pass, the oracle's ids, unchanged launch counters
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

import cross_fp8_reference as F8
import encoder_kernel_reference as R
from conftest import ModelCase, assert_ids_equal_or_tie, load_demo_pcm

pytestmark = pytest.mark.gpu
SPAN_SETS = {1: ([1500], [129]), 3: ([1, 64, 300], [63, 1499, 128]), 5: ([65, 127, 1500, 1, 129], [128, 300, 63, 64, 1499])}


@pytest.fixture(scope="module", params=["BF16", "F16"], ids=["bf16", "fp16"])
def case(request, tmp_path_factory, oracle_mod):
    return ModelCase(tmp_path_factory.mktemp("encspan_" + request.param), "micro", 13, dtype=request.param)


@pytest.fixture(scope="module", params=[64, 128], ids=["rows64", "rows128"])
def handle(request, built_lib, case):
    os.environ["AX_WHISPER_ENC_SPAN_ROWS"] = str(request.param)
    try:
        e = built_lib.Whisper("micro", case.root, "zh", device=0, max_batch=5, cross_span="encoder")
    finally:
        del os.environ["AX_WHISPER_ENC_SPAN_ROWS"]
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 3, 5])
def test_kernel_against_float64(handle, case, n):
    e, dt = handle, "f16" if case.dtype == "F16" else "bf16"
    d, T = e.n_text_state, 1500
    assert e.get_config_int("cross_span") == 2
    rng = np.random.default_rng(77 + n)
    worst = 0.0
    for spans in SPAN_SETS[n]:
        q, k, v = (R.round16(rng.standard_normal((n, T, d)) * s, dt) for s in (2.0, 1.0, 1.0))
        for b, s in enumerate(spans):
            q[b, s:], k[b, s:], v[b, s:] = np.nan, np.nan, np.nan
        out = e.encoder_span_attention(q, k, v, spans)
        for b, s in enumerate(spans):
            assert not out[b, s:].any(), (spans, b, "rows at or beyond the span are not zero")
            for h in range(d // 64):
                c = slice(64 * h, 64 * h + 64)
                ref, bound = R.attention_expect(*(a[b, :s, c].astype(np.float64) for a in (q, k, v)), dt, -(-s // 64) * 64)
                worst = max(worst, R.check_values(f"spans {spans} clip {b} head {h}", out[b, :s, c], ref, bound))
    print(f"encoder span kernel, {n} clips: worst error / bound {worst:.3f}")


def clips_of(lengths):
    pcm = load_demo_pcm()
    return [np.ascontiguousarray(pcm[:n]) for n in lengths]


def test_routing(built_lib, micro_case, oracle_mod, monkeypatch):
    clips = clips_of((48000, 16000, 40000, 30000, 8000))
    plain = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5)
    short = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5, cross_span="encoder")
    monkeypatch.setenv("AX_WHISPER_CROSS_SPAN_MARGIN", "1500")
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5, cross_span="encoder")
    try:
        # full spans: a truncated pass of all rows, the oracle's ids
        got = e.run_tokens_batch(clips, max_new=8)
        assert e.get_config_int("encoder_span_passes") == 1 and e.get_config_int("encoder_span_frames") == 1500
        mels = [oracle_mod.log_mel(c, 80)[0] for c in clips]
        for b, mel in enumerate(mels):
            ck, cv = micro_case.oracle_bf16.encoder(mel)
            ids, lg = micro_case.oracle_bf16.greedy(ck, cv, "zh", max_new=8, want_logits=True)
            assert_ids_equal_or_tie(e, mel, got[b], ids, lg, f"clip {b}", batch_mels=np.stack(mels), slot=b)
        # default margin: spans 250, 150, 225, 194, 125 -> 256 rows per clip
        n0 = short.get_config_int("encoder_span_passes")
        assert all(len(g) == 8 for g in short.run_tokens_batch(clips, max_new=8))
        assert short.get_config_int("encoder_span_passes") == n0 + 1 and short.get_config_int("encoder_span_frames") == 256
        assert list(short.cross_spans()) == [250, 150, 225, 194, 125]
        k, v = short.get_cross_kv(1)
        assert np.isfinite(k).all() and np.isfinite(v).all() and np.abs(k[:, :150]).max() > 0 and not k[:, 150:].any() and not v[:, 150:].any()
        with pytest.raises(RuntimeError):
            short.detect_language_stage(5)
        with pytest.raises(RuntimeError):
            short.decode_forced(2, np.zeros((2, 3), dtype=np.int32))
        with pytest.raises(RuntimeError):
            short.decode_beam(2, 2, max_new=4)
        # prompts on the full-span handle: the prefill reads every frame, so the pass is full; the default handle's ids
        prompts = [[1000, 2000, 3000], [], [400], [500, 600], []]
        for a, b in zip(e.run_timestamp_prompted_batch(clips, prompts, max_new=6), plain.run_timestamp_prompted_batch(clips, prompts, max_new=6)):
            assert a["ids"] == b["ids"]
        for a, b in zip(e.run_tokens_batch(clips[:2], max_new=8), plain.run_tokens_batch(clips[:2], max_new=8)):
            assert list(a) == list(b)
        assert e.get_config_int("encoder_span_passes") == 1
        # two clips: the full pass, the default handle's ids
        n1 = short.get_config_int("encoder_span_passes")
        for a, b in zip(short.run_tokens_batch(clips[:2], max_new=8), plain.run_tokens_batch(clips[:2], max_new=8)):
            assert list(a) == list(b)
        assert short.get_config_int("encoder_span_passes") == n1
    finally:
        for x in (e, short, plain):
            x.close()


def encoder64(w, cfg, mel, n):
    """The encoder over the first n frames in float64 (positional rows [0, n), attention among those frames): cross K, V [L][n][d]."""
    W = lambda name: w[name].astype(np.float64)
    H, nm = cfg["n_audio_head"], mel.shape[0]
    ln = lambda x, p: (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * W(p + ".weight") + W(p + ".bias")
    conv_w = lambda name: W(name).transpose(0, 2, 1).reshape(W(name).shape[0], -1)  # [out][tap][in]
    mp = np.zeros((nm, 3002))
    mp[:, 1:3001] = mel  # column j = frame j - 1
    a1 = np.concatenate([mp[:, k:k + 2 * n].T for k in range(3)], axis=1)
    x1 = np.concatenate([np.zeros((1, W("encoder.conv1.bias").size)), R.gelu64(R.mm64(a1, conv_w("encoder.conv1.weight")) + W("encoder.conv1.bias"))])
    a2 = np.concatenate([x1[k:k + 2 * n:2][:n] for k in range(3)], axis=1)
    x = R.gelu64(R.mm64(a2, conv_w("encoder.conv2.weight")) + W("encoder.conv2.bias")) + W("encoder.positional_embedding")[:n]
    for i in range(cfg["n_audio_layer"]):
        p = f"encoder.blocks.{i}"
        h = ln(x, p + ".attn_ln")
        q, k, v = R.mm64(h, W(p + ".attn.query.weight")) + W(p + ".attn.query.bias"), R.mm64(h, W(p + ".attn.key.weight")), R.mm64(h, W(p + ".attn.value.weight")) + W(p + ".attn.value.bias")
        o = np.empty_like(q)
        for c in (slice(64 * j, 64 * j + 64) for j in range(H)):
            sc = R.mm64(q[:, c], k[:, c]) * 0.125
            pr = np.exp(sc - sc.max(1, keepdims=True))
            o[:, c] = (pr / pr.sum(1, keepdims=True)) @ v[:, c]
        x = x + R.mm64(o, W(p + ".attn.out.weight")) + W(p + ".attn.out.bias")
        h = R.gelu64(R.mm64(ln(x, p + ".mlp_ln"), W(p + ".mlp.0.weight")) + W(p + ".mlp.0.bias"))
        x = x + R.mm64(h, W(p + ".mlp.2.weight")) + W(p + ".mlp.2.bias")
    x = ln(x, "encoder.ln_post")
    dec = [f"decoder.blocks.{i}.cross_attn." for i in range(cfg["n_text_layer"])]
    return np.stack([R.mm64(x, W(p + "key.weight")) for p in dec]), np.stack([R.mm64(x, W(p + "value.weight")) + W(p + "value.bias") for p in dec])


def test_truncated_pass_against_float64(built_lib, micro_case, oracle_mod):
    """get_cross_kv of a truncated pass against the float64 encoder over each clip's first `span` frames. The yardstick is the default
    handle's own full pass against the same float64 encoder over 1500 frames: error / bound with bound = u16 (|ref| + rms(ref)), the
    16-bit storage step at the element's and the tensor's scale. The truncated pass runs the same arithmetic with fewer keys per
    softmax and fewer rows, so its worst ratio is another draw of the same roundings over other elements: it may reach 1.5 x the full
    pass's worst ratio (measured on the GPU: full 2.206, truncated 2.095; DESIGN.md "Encoder spans")."""
    clips = clips_of((48000, 16000, 40000, 30000, 8000))
    mels = [oracle_mod.log_mel(c, 80)[0] for c in clips]
    w, cfg = micro_case.oracle_bf16.w, micro_case.oracle_bf16.cfg
    ratio = lambda got, ref: float((np.abs(got - ref) / (R.u16("bf16") * (np.abs(ref) + np.sqrt((ref * ref).mean())))).max())
    worst = {}
    for mode in (None, "encoder"):
        e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5, cross_span=mode)
        try:
            e.run_tokens_batch(clips, max_new=2)
            assert (e.get_config_int("encoder_span_passes") == 1) == (mode is not None)
            spans = e.cross_spans() if mode else [1500] * 5
            for slot in range(5):
                n = int(spans[slot])
                refs = encoder64(w, cfg, mels[slot], n)
                worst[mode] = max([worst.get(mode, 0.0)] + [ratio(g[:, :n], r) for g, r in zip(e.get_cross_kv(slot), refs)])
        finally:
            e.close()
    print(f"whole pass, worst error / bound: full {worst[None]:.3f}, truncated {worst['encoder']:.3f}")
    assert worst["encoder"] <= 1.5 * worst[None], worst


def test_fp8_codes_come_from_the_span_alone(built_lib, micro_case):
    """A loud full-length clip in every slot, then quiet short ones: codes and scales of each slot equal cross_fp8_reference.quantize of
    the first `span` rows of its h16 image, bit for bit; the louder rows the first pass left behind the span move no scale."""
    pcm = load_demo_pcm()
    loud = np.ascontiguousarray(np.tile(pcm, 1 + 480000 // len(pcm))[:480000])
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5, cross_span="encoder", cross_kv="fp8")
    try:
        e.run_tokens_batch([loud] * 5, max_new=2)
        e.run_tokens_batch([np.ascontiguousarray(np.float32(0.02) * c) for c in clips_of((16000, 8000, 30000, 40000, 48000))], max_new=2)
        assert e.get_config_int("encoder_span_passes") == 2 and list(e.cross_spans()) == [150, 125, 194, 225, 250]
        for slot, n in enumerate(e.cross_spans()):
            kc, vc, sc = e.get_cross_kv_fp8(slot)
            for name, x, codes, scales in zip("KV", e.get_cross_kv(slot), (kc, vc), (sc[:, :, 0, :], sc[:, :, 1, :])):
                want, ex = F8.quantize(x, n_keys=int(n))
                assert np.array_equal(scales.reshape(ex.shape).view(np.uint32), F8.scales_of(ex).view(np.uint32)), (slot, name)
                assert np.array_equal(codes, want), (slot, name, int((codes != want).sum()))
    finally:
        e.close()


@pytest.mark.parametrize("mode", [None, "audio"])
def test_other_handles_keep_ids_and_counters(built_lib, micro_case, oracle_mod, monkeypatch, mode):
    """full and audio handles: no truncated pass, the oracle's ids, and the launch counters of the same call before this mode existed
    (none on a full handle; on an audio handle those of an encoder handle, whose decoder routing is the audio handle's)."""
    monkeypatch.setenv("AX_WHISPER_CROSS_SPAN_MARGIN", "1500")
    clips = clips_of((48000, 16000, 40000, 30000, 8000))
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5, cross_span=mode)
    ref = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=5, cross_span="encoder")
    try:
        got = e.run_tokens_batch(clips, max_new=8)
        ref.run_tokens_batch(clips, max_new=8)
        assert e.get_config_int("cross_span") == (1 if mode else 0) and e.get_config_int("encoder_span_passes") == 0
        assert e.get_config_int("cross_kv_fp8_launches") == 0
        assert e.get_config_int("cross_span_launches") == (ref.get_config_int("cross_span_launches") if mode else 0)
        assert ref.get_config_int("cross_span_launches") > 0
        mels = [oracle_mod.log_mel(c, 80)[0] for c in clips]
        for b, mel in enumerate(mels):
            ck, cv = micro_case.oracle_bf16.encoder(mel)
            ids, lg = micro_case.oracle_bf16.greedy(ck, cv, "zh", max_new=8, want_logits=True)
            assert_ids_equal_or_tie(e, mel, got[b], ids, lg, f"clip {b}", batch_mels=np.stack(mels), slot=b)
        with pytest.raises(RuntimeError):
            e.encoder_span_attention(*[np.zeros((1, 1500, e.n_text_state))] * 3, [5])
    finally:
        e.close()
        ref.close()
