"""GPU, end to end: the persistent launches' attention block where the self-attention cache crosses a 64-key block. On `micro`,
both dtype builds: teacher-forced logits of the one-clip launch at steps t = 63, 64, 65, 127, 128, 129 (step t attends keys 0..t;
the prompt is steps 0..3, so logits row i is step i + 3) against the oracle with the tolerance of
test_gpu_persistent.py::test_persistent_equals_graph_path_and_oracle; the ids of a 130-id greedy run against the launch-per-phase
path; and the ids of a pair in one two-clip launch (clip 1's blocks are register-held) against its clips decoded alone."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (imported before libax_whisper.so so both share torch's HIP runtime in this process)

from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu
STEPS = (63, 64, 65, 127, 128, 129)
N_IDS = 130


def _engine(wa, case, mode, max_batch=1):
    old = os.environ.get("AX_WHISPER_DECODE")
    if mode:
        os.environ["AX_WHISPER_DECODE"] = mode
    else:
        os.environ.pop("AX_WHISPER_DECODE", None)
    try:
        return wa.Whisper(case.model_type, case.root, "zh", device=0, max_batch=max_batch)
    finally:
        if old is None:
            os.environ.pop("AX_WHISPER_DECODE", None)
        else:
            os.environ["AX_WHISPER_DECODE"] = old


@pytest.mark.parametrize("dtype,seed", [("BF16", 61), ("F16", 62)])
def test_block_edges_on_micro(built_lib, oracle_mod, tmp_path, dtype, seed):
    import modelgen

    case = ModelCase(tmp_path, "micro", seed, dtype=dtype)
    clips = [modelgen.synth_clip(seed, 160000), load_demo_pcm()]
    ep, eg = _engine(built_lib, case, None, max_batch=2), _engine(built_lib, case, "graph")
    try:
        assert ep.L.AX_WHISPER_GetConfigInt(ep.h, b"persistent_decode") == 1 and eg.L.AX_WHISPER_GetConfigInt(eg.h, b"persistent_decode") == 0
        assert ep.L.AX_WHISPER_GetConfigInt(ep.h, b"fp16") == (1 if dtype == "F16" else 0)
        # teacher-forced logits at the block edges against the oracle
        mel, _, _ = oracle_mod.log_mel(clips[0], 80)
        ck, cv = case.oracle_bf16.encoder(mel)
        ref_ids, ref_lg = case.oracle_bf16.greedy(ck, cv, "zh", max_new=N_IDS, want_logits=True, eot=-1)
        assert len(ref_ids) == N_IDS
        ep.encode_mel(mel[None])
        lp, _ = ep.decode_forced(1, np.array([ref_ids]))
        for t in STEPS:
            err = float(np.abs(lp[0, t - 3] - ref_lg[t - 3]).max())
            print(f"{dtype} step {t}: logits against the oracle {err:.3e}")
            assert err < 4e-3, (t, err)
        assert float(np.abs(lp[0, :N_IDS + 1] - ref_lg).max()) < 4e-3
        # greedy ids across both edges: the persistent launch and the launch-per-phase path
        ids_p, ids_g = ep.run_tokens(clips[0], max_new=N_IDS), eg.run_tokens(clips[0], max_new=N_IDS)
        assert ids_p == ids_g
        assert len(ids_p) == N_IDS, len(ids_p)  # (an early end of text would keep the run off the edges)
        # a pair in ONE two-clip launch (clip 1's blocks are register-held) against its clips decoded alone
        assert ep.L.AX_WHISPER_GetConfigInt(ep.h, b"persistent_two_clips") == 1 and ep.L.AX_WHISPER_GetConfigInt(ep.h, b"persistent_max_clips") >= 2
        mels = np.stack([ep.compute_mel(c) for c in clips])
        single = []
        for m in mels:
            ep.encode_mel(m)
            single.append(ep.decode_greedy(1, max_new=N_IDS)[0])
        for pair in ((0, 1), (1, 0)):
            ep.encode_mel(np.stack([mels[i] for i in pair]))
            assert ep.decode_greedy(2, max_new=N_IDS) == [single[i] for i in pair], pair
        assert ep.L.AX_WHISPER_GetConfigInt(ep.h, b"persistent_giveups") == 0
    finally:
        ep.close()
        eg.close()
