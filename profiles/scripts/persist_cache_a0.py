"""A0 of tests/persist_cache_reference.py: how far a VERIFIED decode path's self-attention cache sits from the oracle's beyond one
16-bit spacing. The path is the launch-per-phase decoder (AX_WHISPER_DECODE=graph), one clip, teacher forced along its own greedy
ids (decode_forced + get_self_kv), on the cases and mels of tests/test_gpu_persistent_clips.py; the oracle is fed the engine's own
cross K/V (get_cross_kv). Per case and mel: max |got - ref| - ulp16(ref) for K and V; per dtype: the maximum = A0.
usage: persist_cache_a0.py [out.txt]   (needs an MI355X; the multi-clip launch is never run here)"""
import os
import sys
import tempfile

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (R, os.path.join(R, "whisper.axera_amd", "tools"), os.path.join(R, "oracle"), os.path.join(R, "tests"), os.path.join(R, "tests", "golden")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401  (before libax_whisper.so: one HIP runtime in the process)

import oracle  # noqa: E402
import persist_cache_reference as prc  # noqa: E402
import whisper_axera_amd as wa  # noqa: E402
from conftest import ModelCase  # noqa: E402
from test_gpu_persistent_clips import CASES  # noqa: E402

oracle.build(ref=False)
os.environ["AX_WHISPER_DECODE"] = "graph"
lines = []
a0 = {"BF16": -1.0, "F16": -1.0}
for model, seed, dtype, _launches, max_new in CASES:
    case = ModelCase(tempfile.mkdtemp(), model, seed, dtype=dtype)
    e = wa.Whisper(model, case.root, "zh", device=0, max_batch=1)
    try:
        assert e.L.AX_WHISPER_GetConfigInt(e.h, b"persistent_decode") == 0
        for name, mel in zip(("demo", "+5", "bins"), prc.mels(80)):
            e.encode_mel(mel)
            ids = e.decode_greedy(1, max_new=max_new)[0]
            e.encode_mel(mel)
            ck, cv = e.get_cross_kv(0)
            e.decode_forced(1, np.array([ids], dtype=np.int32), want_logits=False)
            k, v = e.get_self_kv(0, len(ids) + 4)
            rk, rv = prc.forced_cache(case.oracle_bf16, ck, cv, ids)
            xk, xv = prc.excess(k, rk, dtype), prc.excess(v, rv, dtype)
            a0[dtype] = max(a0[dtype], xk, xv)
            lines.append("%-5s seed %d %s mel %-4s %3d ids: max|K| %.3f max|V| %.3f  max|dK| %.3e max|dV| %.3e  excess over ulp16(ref): K %.3e V %.3e"
                         % (model, seed, dtype, name, len(ids), np.abs(rk).max(), np.abs(rv).max(), np.abs(k - rk).max(), np.abs(v - rv).max(), xk, xv))
            print(lines[-1], flush=True)
    finally:
        e.close()
for dtype, x in a0.items():
    lines.append("A0[%s] = %.3e" % (dtype, x))
    print(lines[-1])
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
