"""GPU: the batched decode path (3+ clips: bf16-pair activations on the matrix cores, one attention workgroup per
(clip, head), several at few clips) against the oracle and against the small-batch path, at batch sizes that exercise
1, 2 and 4 clip blocks of 16 and a ragged last block."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libax_whisper.so: one HIP runtime per process)

from conftest import assert_ids_equal_or_tie, load_demo_pcm

pytestmark = pytest.mark.gpu


def _mels(n):
    from make_model_goldens_inputs import demo_mel, synth_mel

    out = [demo_mel(80)]
    for i in range(1, n):
        out.append(synth_mel(100 + i, 80, 3000 if i % 3 else 1000 + 37 * i))
    return out


@pytest.fixture(scope="module")
def engine(built_lib, micro_case):
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=50)
    yield e
    e.close()


@pytest.mark.parametrize("B", [3, 4, 5, 16, 21, 24, 44, 50])  # 3-5 clips: cross-attention key blocks split over several workgroups; 24 / 44 / 50 clips: 2 / 3 / 2 graph branches
def test_batched_teacher_forced_logits_vs_oracle(engine, micro_case, B):
    mels = _mels(B)
    engine.encode_mel(np.stack(mels))
    n_forced = 10
    check = sorted(set([0, 1, B // 2, B - 1]))
    forced = np.zeros((B, n_forced), dtype=np.int32)
    refs = {}
    for b in check:
        ck, cv = micro_case.oracle_bf16.encoder(mels[b])
        ids = micro_case.oracle_bf16.greedy(ck, cv, "zh", max_new=n_forced)
        ids = (ids + [0] * n_forced)[:n_forced]
        _, lg = micro_case.oracle_bf16.greedy(ck, cv, "zh", max_new=n_forced, forced=ids, want_logits=True)
        forced[b] = ids
        refs[b] = lg
    for b in range(B):
        if b not in refs:
            forced[b] = forced[check[0]]
    logits, am = engine.decode_forced(B, forced)
    for b in check:
        err = np.abs(logits[b] - refs[b]).max(axis=1)
        print(f"B={B} clip {b}: logits err {err.max():.3e}")
        assert err.max() < 1e-3  # measured 1.1e-4 .. 2.3e-4 at every batch size
        srt = np.sort(refs[b], axis=1)
        margin = srt[:, -1] - srt[:, -2]
        for s in range(refs[b].shape[0]):
            assert am[b, s] == int(refs[b][s].argmax()) or margin[s] < 2 * err[s] + 1e-4


def test_batched_and_single_paths_agree(engine):
    """The same clip through the 1-clip GEMV path and inside a 7-clip MFMA batch: logits within 1e-3, same ids."""
    mels = _mels(7)
    engine.encode_mel(np.stack(mels))
    forced = np.tile(np.arange(10, 18, dtype=np.int32), (7, 1))
    lg_b, am_b = engine.decode_forced(7, forced)
    for b in (0, 3, 6):
        engine.encode_mel(mels[b])
        lg_1, am_1 = engine.decode_forced(1, forced[:1])
        err = np.abs(lg_b[b] - lg_1[0]).max()
        print("clip", b, "batched vs single logits diff", err)
        assert err < 1e-3
        srt = np.sort(lg_1[0], axis=1)
        for s in range(lg_1.shape[1]):
            assert am_b[b, s] == am_1[0, s] or srt[s, -1] - srt[s, -2] < 2e-3


def test_batched_greedy_end_to_end(engine, micro_case):
    import modelgen

    clips = [load_demo_pcm()] + [modelgen.synth_clip(i, 480000 if i % 2 else 160000 + 1000 * i) for i in range(1, 9)]
    got = engine.run_tokens_batch(clips, max_new=12)
    assert len(got) == 9 and all(len(g) == 12 for g in got)
    import oracle

    for b in (0, 4, 8):
        mel, _, _ = oracle.log_mel(clips[b], 80)
        ck, cv = micro_case.oracle_bf16.encoder(mel)
        ids, lg = micro_case.oracle_bf16.greedy(ck, cv, "zh", max_new=12, want_logits=True)
        assert_ids_equal_or_tie(engine, mel, got[b], ids, lg, f"clip {b}")


def test_more_than_64_clips_agree_with_single_path(built_lib, micro_case):
    """70 clips: the clip-block GEMMs span 5 clip blocks in one launch, the vocabulary projection runs as two launches
    (64 + 6 clips); clips on both sides of the boundary must match the 1-clip path."""
    B = 70
    mels = _mels(7)
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=B)
    try:
        e.encode_mel(np.stack([mels[b % 7] for b in range(B)]))
        forced = np.tile(np.arange(20, 28, dtype=np.int32), (B, 1))
        lg_b, am_b = e.decode_forced(B, forced)
        for b in (0, 15, 16, 63, 64, 69):
            e.encode_mel(mels[b % 7])
            lg_1, am_1 = e.decode_forced(1, forced[:1])
            err = np.abs(lg_b[b] - lg_1[0]).max()
            print("clip", b, "batched(70) vs single logits diff", err)
            assert err < 1e-3
            srt = np.sort(lg_1[0], axis=1)
            for s in range(lg_1.shape[1]):
                assert am_b[b, s] == am_1[0, s] or srt[s, -1] - srt[s, -2] < 2e-3
    finally:
        e.close()


@pytest.mark.parametrize("model_type,seed", [("w512", 21), ("w1024", 22), ("w1280", 23)])
def test_model_widths_batched_and_single_vs_oracle(built_lib, oracle_mod, tmp_path, model_type, seed):
    """The widths of Whisper base / medium / large at reduced depth: every width-dependent instantiation of the batched
    kernels (LayerNorm-prologue GEMM with 2, 4 and 5 k-steps per wave, register-resident vocabulary projection, the
    split-K sequence at 1280) and of the 1-clip path, teacher-forced logits against the oracle (bf16 policy)."""
    from conftest import ModelCase
    from make_model_goldens_inputs import demo_mel, synth_mel

    case = ModelCase(tmp_path, model_type, seed)
    nm = case.dims["n_mels"]
    B, n = 20, 6
    mels = [demo_mel(nm)] + [synth_mel(50 + i, nm, 3000 if i % 2 else 1200 + 11 * i) for i in range(1, B)]
    check = (0, 7, 19)
    forced = np.zeros((B, n), dtype=np.int32)
    refs = {}
    for b in check:
        ck, cv = case.oracle_bf16.encoder(mels[b])
        ids = case.oracle_bf16.greedy(ck, cv, "zh", max_new=n)
        ids = (ids + [0] * n)[:n]
        _, lg = case.oracle_bf16.greedy(ck, cv, "zh", max_new=n, forced=ids, want_logits=True)
        forced[b], refs[b] = ids, lg
    for b in range(B):
        if b not in refs:
            forced[b] = forced[0]
    e = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=B)
    try:
        for batch in (B, 6):  # two clip blocks (one ragged) / one
            e.encode_mel(np.stack(mels[:batch]))
            logits, am = e.decode_forced(batch, forced[:batch])
            for b in [c for c in check if c < batch]:
                err = np.abs(logits[b] - refs[b]).max(axis=1)
                print(f"{model_type} batch {batch} clip {b}: logits err {err.max():.3e}")
                assert err.max() < 4e-3  # measured: d = 512 6.3e-4, d = 1024 5.4e-4, d = 1280 1.0e-3
                srt = np.sort(refs[b], axis=1)
                for s in range(refs[b].shape[0]):
                    assert am[b, s] == int(refs[b][s].argmax()) or srt[s, -1] - srt[s, -2] < 2 * err[s] + 1e-4
        e.encode_mel(mels[7])
        lg1, _ = e.decode_forced(1, forced[7:8])
        err1 = np.abs(lg1[0] - refs[7]).max()
        print(f"{model_type} single clip: logits err {err1:.3e}")
        assert err1 < 3e-3  # measured 4.0e-4 .. 6.7e-4
    finally:
        e.close()


@pytest.mark.parametrize("B,n_forced", [(3, 8), (4, 8), (4, 70)], ids=["3", "4", "4-past-key-block-64"])
def test_cross_attention_splits_and_decode_families_agree(built_lib, micro_case, monkeypatch, B, n_forced):
    """At few clips the key blocks of a (clip, head) are divided among several workgroups that meet through a ticket
    (decoder.hip); the result must not depend on the split count (fold in split order), and the GEMV family (still the
    path of one and two clips without the persistent launch) must agree with the clip-block GEMMs on the same clips.

    70 forced ids (decode offsets 0..72): every family appends K / V rows on both sides of the self cache's first 64-key block
    boundary — the four-clip GEMV kernel, the clip-block GEMM and, in that case only, the split-K sequence
    (AX_WHISPER_BATCHED_LN=0: decode_gemm_kernel + act_prep) — and attends over two blocks. The bounds are those of the 8-id cases:
    the families differ in fp32 summation order and in which side of a rounding boundary a cached 16-bit K / V value falls, per row;
    neither grows with the number of cached rows (softmax weights sum to 1), while a row appended at a wrong index is an error of
    the size of the logits themselves."""
    mels = np.stack(_mels(B))
    forced = np.tile(np.array([[50258 + (i * 7) % 100 for i in range(n_forced)]], dtype=np.int32), (B, 1))
    out = {}
    cases = [("default", {}), ("one workgroup", {"AX_WHISPER_CROSS_SPLIT": "1"}), ("three", {"AX_WHISPER_CROSS_SPLIT": "3"}),
             ("gemv family", {"AX_WHISPER_GEMV_MAX": "4"})]
    if n_forced > 64:
        cases.append(("split-K sequence", {"AX_WHISPER_BATCHED_LN": "0"}))
    for name, env in cases:
        for k in ("AX_WHISPER_CROSS_SPLIT", "AX_WHISPER_GEMV_MAX", "AX_WHISPER_BATCHED_LN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=B)
        try:
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"batched_ln") == (0 if name == "split-K sequence" else 1)
            e.encode_mel(mels)
            out[name] = e.decode_forced(B, forced)[0]
        finally:
            e.close()
    for name in ("one workgroup", "three"):
        d = float(np.abs(out[name] - out["default"]).max())
        print(f"B={B} cross-attention splits, {name} vs default: {d:.3e}")
        assert d < 2e-4  # fp32 partial sums in a different association
    d = float(np.abs(out["gemv family"] - out["default"]).max())
    print(f"B={B} GEMV family vs clip-block GEMMs: {d:.3e}")
    assert d < 5e-3
    if "split-K sequence" in out:
        d = float(np.abs(out["split-K sequence"] - out["default"]).max())
        print(f"B={B} split-K sequence vs clip-block GEMMs: {d:.3e}")
        assert d < 2e-3  # the bound of test_gpu_fullsize.test_small_batched_decode_sequences_agree (both sides carry (hi, lo) pairs)


@pytest.mark.parametrize("B", [3, 6])
def test_ragged_small_batch_with_split_cross_attention(built_lib, micro_case, B):
    """Clips that leave early (per-clip id budgets) beside clips that run on, at clip counts where the cross-attention of a
    (clip, head) is split over several workgroups: a finished clip's workgroups return before they touch the tickets of
    their (clip, head), the others' ids stay those of the uniform run."""
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=B)
    try:
        e.encode_mel(np.stack(_mels(B)))
        uniform = e.decode_greedy(B, max_new=24)
        budget = [2 + 7 * (b % 3) for b in range(B)]
        ragged = e.decode_greedy(B, max_new=24, max_new_clip=budget)
        for b in range(B):
            assert ragged[b] == uniform[b][: budget[b]], b
        again = e.decode_greedy(B, max_new=24)  # tickets were left at zero: the next call is unaffected
        assert again == uniform
    finally:
        e.close()


@pytest.mark.parametrize("model_type,kind,B,seed", [("micro", "benign", 4, 11), ("mini", "realistic", 7, 42), ("micro", "benign", 40, 11),
                                                    ("w512", "realistic", 20, 43)])
def test_clip_block_query_fold_equals_the_fused_projection(built_lib, oracle_mod, tmp_path, monkeypatch, model_type, kind, B, seed):
    """Round 6 (decode_gemm.hip "QUERY FOLD"): the clip-block step folds the cross-attention query through the self-attention
    output projection — A0 from the QKV launch, T = A0 + M a + d and the block statistics from the o launch, the cross-attention
    workgroups start with r (T - mu s) + c. Against the fused projection of the same build (AX_WHISPER_CBLOCK_QFOLD=0), the same
    arithmetic in another association: teacher-forced logits within 2e-5 (benign) / 4e-4 (trained-model statistics) of the logit
    scale; and against the policy oracle as every other batched test. One branch with key splits (4, 7, 20 clips) and two
    branches (40 clips)."""
    from conftest import ModelCase
    import modelgen

    case = ModelCase(tmp_path, model_type, seed, kind=kind)
    n_mels = case.dims["n_mels"]
    clips = [load_demo_pcm(), modelgen.synth_clip(seed, 200000), modelgen.synth_clip(seed + 1, 90000)]
    n = 12
    out = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("AX_WHISPER_CBLOCK_QFOLD", "2" if fold == "1" else "0")  # "2": the fold in multi-branch steps too (production: one-branch steps)
        e = built_lib.Whisper(model_type, case.root, "zh", device=0, max_batch=B)
        try:
            assert e.L.AX_WHISPER_GetConfigInt(e.h, b"cblock_qfold") == (2 if fold == "1" else 0)
            mels = np.stack([e.compute_mel(clips[b % 3]) for b in range(B)])
            e.encode_mel(mels)
            if fold == "1":
                ids = e.decode_greedy(B, max_new=n)
                forced = np.array([(ids[b] + [50257] * n)[:n] for b in range(B)], dtype=np.int32)
            lg, am = e.decode_forced(B, forced)
            out[fold] = (lg, am, e.decode_greedy(B, max_new=n))
        finally:
            e.close()
    (l1, a1, g1), (l0, a0, g0) = out["1"], out["0"]
    scale = float(np.abs(l0).max())
    err = float(np.abs(l1 - l0).max())
    print(f"{model_type} ({kind}) B={B}: folded vs fused-projection logits differ by {err:.3e} at |logit| <= {scale:.1f}")
    # M enters as an (hi, lo) h16 pair (2^-17 relative) where the fused projection multiplies the exact W_cq rows, and a last-bit fp32
    # difference in a query flips the 16-bit rounding of a stored self-attention K/V entry here and there: measured 6.6e-5 at
    # |logit| <= 1.1 (micro, 4 clips) — the size of the difference between any two batched paths (1.5e-4 vs the oracle above)
    rel = 1.5e-4 if kind == "benign" else 4e-4
    assert err < rel * max(scale, 1.0) + 2e-5, (err, scale)
    for b in range(B):  # greedy ids: equal, or a tie at the first difference measured on the forced logits of that clip
        if g1[b] != g0[b]:
            i = next(i for i in range(min(len(g1[b]), len(g0[b]))) if g1[b][i] != g0[b][i])
            srt = np.sort(l0[b, i])
            assert srt[-1] - srt[-2] < 2 * float(np.abs(l1[b, i] - l0[b, i]).max()) + 1e-4, (b, i)
    # the policy oracle on clip 0 and 1 (teacher-forced along the same ids)
    for b in (0, 1):
        mel = oracle_mod.log_mel(clips[b % 3], n_mels)[0]
        ck, cv = case.oracle_bf16.encoder(mel)
        _, lg = case.oracle_bf16.greedy(ck, cv, "zh", max_new=n, forced=[int(t) for t in forced[b]], want_logits=True)
        eo = float(np.abs(l1[b, : len(lg)] - lg).max())
        print(f"  clip {b}: folded vs policy oracle {eo:.3e}")
        assert eo < (5e-3 if kind == "benign" else 0.2), eo
