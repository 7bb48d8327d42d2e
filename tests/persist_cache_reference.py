"""Reference side of tests/test_gpu_persistent_clips.py: what the self-attention caches of the later clips of a multi-clip
persistent launch (decode_persistent2.hip) must hold, and the comparison both that test and its CPU twin
(tests/test_persist_cache_reference.py) use.

Row t of layer l of a clip's cache is W_k / W_v . LN(residual stream entering layer l at step t): everything the launch
computed for that clip below that point. The oracle restates it one decoder step at a time (Oracle.decoder_step), teacher
forced along the launch's own ids, from the cross K/V the test hands it.

Seeded benign weights barely listen to ordinary audio (greedy ids of different clips are equal, a wrong clip's cross K/V moves
the cache by 0.03 .. 0.09); the three mels of `mels` are the inputs found to separate the clips: pairwise different ids and a
cache that moves by >= 0.7 in every layer >= 1 under a neighbour's cross K/V (`separation`)."""
import os
import wave

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The tolerance of the cache comparison is ulp16(ref) + A[dtype] per element.
#   ulp16(ref): derived. Engine and oracle round slightly different fp32 values at the 16-bit store.
#   A: fp32 association error carried through the layers; not derivable. A0 is MEASURED on a path earlier work verified (the
#   launch-per-phase decoder, AX_WHISPER_DECODE=graph, one clip: decode_forced + get_self_kv against forced_cache, on the cases of
#   test_gpu_persistent_clips.py; profiles/scripts/persist_cache_a0.py, figures in profiles/persist_cache_a0.txt) as the largest
#   excess of |got - ref| over ulp16(ref); A = 4 x A0 rounded up to one significant digit (two correct summation orders may sit
#   on opposite sides of the oracle, and compiler versions move it). Never taken from the multi-clip launch.
#   Measured on an MI355X: BF16 1.465e-3 (small/43, the +5 mel, K; micro 9.5e-7, mini 3.8e-6, tiny 1.2e-4, w512 3.1e-5: it grows with
#   depth and width), F16 4.578e-5 (tiny/44).
A0 = {"BF16": 1.465e-3, "F16": 4.578e-5}
A = {"BF16": 6e-3, "F16": 2e-4}

MANTISSA = {"BF16": 7, "F16": 10}
# ulp16's floor: the spacing at 2^-14, the smallest normal IEEE half (a small normal bfloat16, too), so that a reference of
# exactly 0 (or a subnormal) does not ask for bit equality
FLOOR_EXP = -14


def mels(n_mels):
    """The three mels [n_mels][3000] that tell clips apart: demo.wav's log-mel, +5.0 everywhere, +5.0 / -5.0 in even / odd bins."""
    import oracle

    w = wave.open(os.path.join(GOLDEN, "demo.wav"))
    pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).astype(np.float32) / np.float32(32768.0)
    demo = np.ascontiguousarray(oracle.log_mel(pcm, n_mels)[0], dtype=np.float32)
    assert demo.shape == (n_mels, 3000)
    plus5 = np.full((n_mels, 3000), 5.0, dtype=np.float32)
    bins = np.where((np.arange(n_mels) % 2 == 0)[:, None], np.float32(5.0), np.float32(-5.0)) * np.ones((1, 3000), dtype=np.float32)
    return [demo, plus5, np.ascontiguousarray(bins, dtype=np.float32)]


def forced_cache(orc, ck, cv, ids):
    """sot_seq("zh") + ids through the oracle's decoder, one step each -> (sk, sv), rows [0, len(ids) + 4) of every layer:
    fp32 [n_text_layer][len(ids) + 4][d]."""
    ck, cv = np.ascontiguousarray(ck, dtype=np.float32), np.ascontiguousarray(cv, dtype=np.float32)
    sk, sv = orc.new_self_cache()
    toks = list(orc.sot_seq("zh")) + [int(i) for i in ids]
    assert len(toks) <= sk.shape[1]
    for off, tok in enumerate(toks):
        orc.decoder_step(tok, off, ck, cv, sk, sv, want_logits=False)
    return sk[:, : len(toks)].copy(), sv[:, : len(toks)].copy()


def ulp16(r, dtype):
    """Spacing of the 16-bit type `dtype` ("BF16": 7 mantissa bits, "F16": 10) at |r|, elementwise, floored at the spacing at
    2^FLOOR_EXP."""
    a = np.abs(np.asarray(r, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** FLOOR_EXP)))  # (exact at powers of two: log2 of a power of two is exact in float64)
    return np.exp2(e - MANTISSA[dtype])


def worst_ratio(got, ref, dtype, a):
    """THE comparison: max over elements of |got - ref| / (ulp16(ref) + a). A cache passes when this is <= 1."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (ulp16(ref, dtype) + a)).max())


def max_tolerance(ref, dtype, a):
    """The largest per-element tolerance worst_ratio uses against `ref`."""
    return float(ulp16(np.abs(np.asarray(ref)).max(), dtype) + a)


def excess(got, ref, dtype):
    """Largest |got - ref| - ulp16(ref) (what A0 is the maximum of); negative when every element is within one spacing."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) - ulp16(ref, dtype)).max())


def separation(orc, kvs, idss, own=None):
    """How far a wrong clip's cross K/V moves a clip's cache: the minimum, over clips i and layers >= 1 (layer 0 depends on the
    ids only), of max |forced_cache(cross K/V of clip i + 1, ids_i) - forced_cache(cross K/V of clip i, ids_i)| -> (for K, for V).
    kvs: [(ck, cv)] per clip, idss: the ids per clip; own (optional): the clips' own forced_cache results, if the caller has them."""
    n = len(kvs)
    sep_k = sep_v = float("inf")
    for i in range(n):
        k0, v0 = own[i] if own is not None else forced_cache(orc, *kvs[i], idss[i])
        k1, v1 = forced_cache(orc, *kvs[(i + 1) % n], idss[i])
        for l in range(1, k0.shape[0]):
            sep_k = min(sep_k, float(np.abs(k1[l] - k0[l]).max()))
            sep_v = min(sep_v, float(np.abs(v1[l] - v0[l]).max()))
    return sep_k, sep_v
