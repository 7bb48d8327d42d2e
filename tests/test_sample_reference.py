"""CPU: the temperature-fallback contract off the GPU — Philox's known answers, the reference sampler against the distribution
it claims to draw from, AX_WHISPER_CompressionRatio and AX_WHISPER_WindowNeedsFallback against Python, the attempt bookkeeping
of the loop reference, the sampled kernel's resources in both builds and the new exports."""
import ctypes as C
import math
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import longform_reference as lfr
import sample_reference as smp
import score_reference as sr
import ts_reference as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["AX_WHISPER_SampleTimestampRules", "AX_WHISPER_DecodeForcedTimestampSampled", "AX_WHISPER_RunPCMBatchTimestampSampled",
               "AX_WHISPER_CompressionRatio", "AX_WHISPER_WindowNeedsFallback", "AX_WHISPER_RunPCMLongWindowsFallback",
               "AX_WHISPER_RunPCMLongFallback", "AX_WHISPER_RunFileLongFallback"]
E, T, NV = 50257, 50364, 51865

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = tuple(int(w) for w in smp.philox4x32_10(*ctr, *key))
        assert got == want, ([hex(g) for g in got], [hex(w) for w in want])
    # vectorised over counters: the same words as one call per counter
    c0 = np.arange(5, dtype=np.uint64)
    many = np.stack(smp.philox4x32_10(c0, np.full(5, 3), np.full(5, 7), np.full(5, 9), 11, 13), axis=1)
    for i in range(5):
        assert tuple(int(w) for w in many[i]) == tuple(int(w) for w in smp.philox4x32_10(i, 3, 7, 9, 11, 13))


def test_uniforms_and_gumbel_row():
    u = smp.uniforms(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint64))
    assert u[0] == u[1] == 2.0 ** -24 and u[2] == 1.5 * 2.0 ** -23 and u[3] == 1.0 - 2.0 ** -24
    g = smp.gumbel_row(NV, 5, (3 << 32) | 17, 0x1234567890)
    assert g.shape == (NV,) and np.isfinite(g).all() and g.min() > -2.9 and g.max() < 16.7
    # id i takes word i & 3 of counter (i >> 2, n, stream low, stream high)
    w = smp.philox4x32_10(NV // 4, 5, 17, 3, 0x34567890, 0x12)
    last = smp.uniforms(np.array([int(w[0])], dtype=np.uint64))
    assert g[NV - 1] == -np.log(-np.log(last[0]))  # 51864 = 4 * 12966 + 0: the vocabulary's last, partial chunk
    assert not np.array_equal(g, smp.gumbel_row(NV, 6, (3 << 32) | 17, 0x1234567890))
    assert not np.array_equal(g, smp.gumbel_row(NV, 5, (3 << 32) | 18, 0x1234567890))
    assert not np.array_equal(g, smp.gumbel_row(NV, 5, (3 << 32) | 17, 0x1234567891))


# 0.999 quantiles of chi-square with 1 .. 7 degrees of freedom
CHI2_999 = {1: 10.828, 2: 13.816, 3: 16.266, 4: 18.467, 5: 20.515, 6: 22.458, 7: 24.322}


@pytest.mark.parametrize("t", [0.2, 0.6, 1.0])
def test_the_reference_sampler_is_a_sampler(t):
    """4096 draws over varying (stream, n) against softmax(x / t); cells with expectation >= 5. The seeds are fixed, so the outcome is."""
    vals = [0.0, 1.0, 2.0, -1.0, 0.5, 1.5, -2.0, 3.0]
    ids = [5, 100, 2000, T + 10, 30000, E, T + 1400, 7777]  # text ids, eot and timestamps, all allowed after [T, 5, T + 3, T + 3, 9]
    hist = [T, 5, T + 3, T + 3, 9]
    x = np.full(NV, -np.inf, dtype=np.float32)
    x[ids] = vals
    assert not tsr.decide(x, hist, T, E)[1]["rule5"]  # (the eight candidates are the final allowed set's finite part)
    N = 4096
    counts = dict.fromkeys(ids, 0)
    seqs = [[T, 5] * r + hist for r in range(3)]  # the history length is the counter's second word: three lengths, one rule state
    allowed = [(tsr.decide(x, q, T, E)[1], sr.final_allowed(x, q, T, E)) for q in seqs]
    for k in range(N):
        c, lp, info = smp.sample(x, seqs[k % 3], T, E, t, stream=(k // 7) | ((k % 5) << 32), seed=20240, allowed=allowed[k % 3])
        counts[c] += 1
        assert abs(float(lp) - (float(x[c]) - tsr._lse(np.array(vals)))) < 1e-6  # untempered
    p = np.exp(np.array(vals) / t)
    p /= p.sum()
    cells = [(counts[i], N * pi) for i, pi in zip(ids, p) if N * pi >= 5.0]
    chi2 = sum((o - e) ** 2 / e for o, e in cells)
    dof = len(cells) - 1
    print("t = %.1f: chi-square %.2f over %d cells (0.999 quantile %.2f)" % (t, chi2, len(cells), CHI2_999[dof]))
    assert dof == {0.2: 1, 0.6: 5, 1.0: 7}[t]
    assert chi2 < CHI2_999[dof], (t, chi2, counts)


def test_reference_sampler_edges():
    x = np.full(NV, -10.0, dtype=np.float32)
    hist = [T, 5]
    # temperature 0: the scored reference
    assert smp.sample(x, hist, T, E, 0.0, 1, 2)[:2] == sr.token_logprob(x, hist, T, E)[:2]
    # a +inf logit has key +inf; two of them: the lowest id, never a near tie
    y = x.copy(); y[900] = np.inf; y[40] = np.inf
    c, lp, info = smp.sample(y, hist, T, E, 0.6, 1, 2)
    assert c == 40 and lp == 0.0 and not info["near_tie"]
    # NaN logits are masked; nothing finite left: eot with -inf
    z = np.full(NV, np.nan, dtype=np.float32); z[77] = 1.0
    assert smp.sample(z, hist, T, E, 1.0, 1, 2)[0] == 77
    c, lp, _ = smp.sample(np.full(NV, -np.inf, dtype=np.float32), hist, T, E, 1.0, 1, 2)
    assert c == E and lp == -np.inf
    # rules 1-5 are decided on the untempered logits: after an open pair text stays masked whatever the noise
    y = x.copy(); y[5] = 50.0
    for s in range(20):
        c, _, _ = smp.sample(y, [T, 5, T + 10], T, E, 1.0, s, 2)
        assert c == E or c >= T + 10
    # rule 5 fired: a timestamp, even where a text id has the larger key
    y = x.copy(); y[T + 1:T + 101] = 0.0; y[7] = 2.0
    assert tsr.decide(y, hist, T, E)[1]["rule5"]
    assert all(smp.sample(y, hist, T, E, 1.0, s, 2)[0] > T for s in range(20))


def test_compression_ratio(built_lib):
    cases = [b"", b"a", b"hello world", b"ab" * 400, "你好，世界。".encode("utf-8"), ("重复" * 120).encode("utf-8"), bytes(range(256)) * 3,
             b" the the the the the the the the the the the the the the the the"]
    for b in cases:
        want = len(b) / len(zlib.compress(b))
        assert built_lib.compression_ratio(b) == np.float32(want), (b[:20], built_lib.compression_ratio(b), want)
        assert smp.compression_ratio(b) == np.float32(want)
    assert built_lib.compression_ratio(b"") == 0.0
    assert built_lib.compression_ratio("你好") == built_lib.compression_ratio("你好".encode("utf-8"))
    assert built_lib.compression_ratio(b"ab" * 400) > 2.4 > built_lib.compression_ratio(b"hello world")
    # the text rule: ids below eot, ASCII whitespace stripped at both ends only
    table = {1: b" hello", 2: b" world \n", 3: b"\xe4\xbd\xa0", E: b"<|endoftext|>", T: b"<|0.00|>"}
    detok = lambda ids: b"".join(table[i] for i in ids)
    assert smp.window_text([T, 1, 2, T + 0, E], E, detok) == b"hello world"
    assert smp.window_text([T, 3, 1], E, detok) == b"\xe4\xbd\xa0 hello"
    assert smp.window_text([T], E, detok) == b""


def test_window_needs_fallback_grid(built_lib):
    nan, inf = math.nan, math.inf
    lp = math.log
    table = [
        # cr, avg, nsp, cr_thr, lp_thr, ns_thr, want
        (3.0, -0.5, lp(0.1), 2.4, -1.0, 0.6, True),      # repetition
        (2.0, -0.5, lp(0.1), 2.4, -1.0, 0.6, False),
        (2.0, -1.5, lp(0.1), 2.4, -1.0, 0.6, True),      # low confidence
        (2.0, -1.5, lp(0.9), 2.4, -1.0, 0.6, False),     # silence overrides
        (3.0, -1.5, lp(0.9), 2.4, -1.0, 0.6, False),     # ... the ratio too
        (3.0, -0.5, lp(0.9), 2.4, -1.0, 0.6, True),      # confident text over a high no-speech value: the ratio still counts
        (2.4, -1.0, lp(0.1), 2.4, -1.0, 0.6, False),     # on both thresholds: strict comparisons
        (float(np.nextafter(np.float32(2.4), np.float32(3))), -1.0, lp(0.1), 2.4, -1.0, 0.6, True),
        (2.4, float(np.nextafter(np.float32(-1.0), np.float32(-2))), lp(0.1), 2.4, -1.0, 0.6, True),
        (9.0, -0.5, lp(0.1), nan, -1.0, 0.6, False),     # NaN thresholds switch their part off
        (9.0, -5.0, lp(0.1), 2.4, nan, 0.6, True),
        (1.0, -5.0, lp(0.1), 2.4, nan, 0.6, False),
        (1.0, -5.0, lp(0.9), 2.4, -1.0, nan, True),
        (9.0, -5.0, lp(0.9), nan, nan, nan, False),
        (0.0, -5.0, lp(0.1), 0.0, nan, nan, False),      # 0 > 0 is false: an empty text never trips the ratio at threshold 0
        (0.5, -0.1, lp(0.1), 0.0, nan, nan, True),
        (nan, -0.5, lp(0.1), 2.4, -1.0, 0.6, False),
        (2.0, -inf, -inf, 2.4, -1.0, 0.6, True),
    ]
    for cr, avg, nsp, a, b, c, want in table:
        assert smp.needs_fallback(cr, avg, nsp, a, b, c) == want, (cr, avg, nsp, a, b, c)
        assert built_lib.window_needs_fallback(cr, avg, nsp, a, b, c) == want, (cr, avg, nsp, a, b, c)
    assert built_lib.window_needs_fallback(9.0, -5.0, 0.0) is False  # None: every part off
    rng = np.random.default_rng(9)
    for _ in range(3000):
        cr, avg, nsp = float(rng.uniform(0.0, 4.0)), -float(rng.exponential(1.2)), -float(rng.exponential(1.0))
        a, b, c = (float(rng.choice(v)) for v in ([2.4, 0.0, nan], [-1.0, -0.3, nan, inf], [0.6, 0.2, nan]))
        assert bool(built_lib.load_library().AX_WHISPER_WindowNeedsFallback(cr, avg, nsp, a, b, c)) == smp.needs_fallback(cr, avg, nsp, a, b, c)


def test_loop_reference_attempt_bookkeeping():
    n_samples = lfr.LENGTHS[4]  # 75 s
    temps = [0.0, 0.2, 0.4, 0.6]
    good, loop_text = b"some ordinary words that do not repeat", b"ha " * 200
    ids_of = lambda seek: [T, 5, 6, T + 200, T + 200, 7, T + 1000, T + 1000, 8]  # advance 2000 frames unless the window is short
    calls = []

    def scripted(script):
        def decode(seek, wf, a, t):
            calls.append((seek, a))
            text, avg, nsp = script(seek, a)
            return ids_of(seek), nsp, avg, text
        return decode

    quiet, loud = math.log(0.01), math.log(0.95)
    run = lambda script: smp.loop_fallback(n_samples, scripted(script), T, E, temps, 2.4, -1.0, 0.6)
    # pass at attempt 0 everywhere: the plain loop, one entry per window
    got = run(lambda s, a: (good, -0.4, quiet))
    plain = lfr.loop(n_samples, lambda s, w: ids_of(s), T, E)
    assert [(w[0], w[1], w[2], w[3]) for w in got] == plain and all(w[4] == 0 and w[7] and not w[8] for w in got)
    # the window at 2000 repeats until attempt 2, the one at 4000 is unsure at attempt 0 only
    script = lambda s, a: (loop_text, -0.4, quiet) if (s == 2000 and a < 2) else ((good, -1.6, quiet) if (s == 4000 and a == 0) else (good, -0.4, quiet))
    got = run(script)
    assert [(w[0], w[4], w[7], w[2]) for w in got] == [(0, 0, True, 2000), (2000, 0, False, 0), (2000, 1, False, 0), (2000, 2, True, 2000),
                                                       (4000, 0, False, 0), (4000, 1, True, 2000), (6000, 0, True, 1500)]
    assert [w[5] for w in got if w[0] == 2000] == [0.0, float(np.float32(0.2)), float(np.float32(0.4))]
    assert got[1][6] > 2.4 > got[3][6]
    # never passes: every temperature is tried, the last is kept and advances by the window rule
    got = run(lambda s, a: (loop_text, -0.4, quiet))
    assert [w[4] for w in got if w[0] == 0] == [0, 1, 2, 3] and [w[7] for w in got if w[0] == 0] == [False, False, False, True]
    assert len(got) == 4 * len(plain) and [w[0] for w in got if w[7]] == [w[0] for w in plain]
    # silence override: low confidence under a high no-speech value is not retried, the silent-window rule skips it
    got = run(lambda s, a: (good, -3.0, loud))
    assert all(w[4] == 0 and w[7] and w[8] and w[2] == w[1] for w in got) and [w[0] for w in got] == [0, 3000, 6000]
    # one temperature: no retry at all
    got = smp.loop_fallback(n_samples, scripted(lambda s, a: (loop_text, -3.0, quiet)), T, E, [0.0], 2.4, -1.0, 0.6)
    assert all(w[7] and w[4] == 0 for w in got) and len(got) == len(plain)


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
def test_sampled_kernel_resources(f16, tmp_path):
    out = tmp_path / "ts.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-o", str(out),
                        os.path.join(ROOT, "whisper.axera_amd", "csrc", "decode_timestamps.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    assert sum("timestamp_rules_sampled_kernel" in n for n in names) == 1, names
    k = next(i for i, n in enumerate(names) if "timestamp_rules_sampled_kernel" in n)
    field = lambda f: [int(x) for x in re.findall(r"^\s+\.%s:\s+(\d+)" % f, text, re.M)]
    assert field("private_segment_fixed_size")[k] == 0
    assert field("vgpr_spill_count")[k] == 0 and field("sgpr_spill_count")[k] == 0
    # 256-thread workgroups, eight of them per CU wanted (64 VGPRs each); the Philox rounds and two more argmax pairs fit in 48
    assert field("vgpr_count")[k] <= 48, field("vgpr_count")[k]


def test_new_symbols_are_exported_and_bound(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    assert set(NEW_SYMBOLS) <= set(built_lib.SYMBOLS)
    for m in ("sample_timestamp_rules", "decode_forced_timestamp_sampled", "run_timestamp_sampled_batch", "run_long_windows", "run_long_scored",
              "run_long_text"):
        assert callable(getattr(built_lib.Whisper, m))
    assert callable(built_lib.compression_ratio) and callable(built_lib.window_needs_fallback)


def test_sampled_calls_reject_null_arguments(built_lib):
    L = built_lib.load_library()
    n = C.c_int()
    out = C.c_void_p()
    t = (C.c_float * 1)(0.0)
    assert L.AX_WHISPER_SampleTimestampRules(None, None, None, None, 1, None, None, 0, None, None) == -1
    assert L.AX_WHISPER_DecodeForcedTimestampSampled(None, 1, None, 0, None, None, 0, None, None, None, None, None) == -1
    assert L.AX_WHISPER_RunPCMBatchTimestampSampled(None, None, None, 1, 0, None, None, None, 0, None, None, None, None, None, None) == -1
    assert L.AX_WHISPER_CompressionRatio(None, 3, None) == -1
    assert L.AX_WHISPER_RunPCMLongWindowsFallback(None, None, None, 1, 0, 0, 0.6, -1.0, 2.4, t, 1, 0, None, 0, None, None, None, C.byref(n)) == -1
    assert L.AX_WHISPER_RunPCMLongWindowsFallback(None, None, None, 1, 0, 0, 0.6, -1.0, 2.4, None, 0, 0, None, 0, None, None, None, C.byref(n)) == -1
    assert L.AX_WHISPER_RunPCMLongFallback(None, None, 0, 0.6, -1.0, 2.4, t, 1, 0, C.byref(out)) == -1
    assert L.AX_WHISPER_RunFileLongFallback(None, b"x.wav", 0.6, -1.0, 2.4, t, 1, 0, C.byref(out)) == -1
