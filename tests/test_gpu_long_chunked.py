"""GPU: chunked long-form (DESIGN.md "Chunked long-form") — the levels kernel against float64 within the bound derived from its sums,
the plan kernel against the host rule (exactly), the cut window against the existing window call (bit for bit), the passes against
the oracle at the cross K/V and through the tie rule, segments in file time, the scored variant, isolation from the existing entry
points, every refusal, and the CLI's --long --chunked lines.

Inputs: the files of tests/longform_reference.py (12 s, 45 s, 75 s) and a 0.1 s file. End to end: W_max = 1000, W_min = 600 on the
45 s and the 75 s file together with 8 slots (6 + 10 windows: two full passes), and once more with the 12 s file's two windows behind
them as a pass that does not fill the slots."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import long_cuts_reference as lcr
import longform_reference as lfr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

BUDGET = 12      # ids per window: enough for timestamps, text and a cut; the oracle decodes every window once
KV_AGREE = 2e-2  # the cross-K/V bar of test_gpu_parity.py and test_gpu_longform.py
W_MIN, W_MAX = 600, 1000


class Model:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=8)
        self.T, self.E, self.nm = self.e.timestamp_begin, self.e.eot, self.case.dims["n_mels"]
        demo = load_demo_pcm()
        self.files = {k: lfr.make_file(demo, k) for k in (1, 3, 4)}
        self.files[0] = np.ascontiguousarray(self.files[1][5000:6600])  # 0.1 s: 11 frames, every box clamped at both ends
        self._norm, self._x, self._enc, self._dec = {}, {}, {}, {}
        self.prefix = self.case.oracle_bf16.sot_seq("zh")[:3]
        self.excused = 0

    def norm(self, k):
        if k not in self._norm:
            self._norm[k] = lfr.file_log_mel(self.files[k], self.nm)[0]
        return self._norm[k]

    def x(self, k):
        """what the encoder will see of every frame of file k, as the GPU's own window call returns it: float32 [n_frames][n_mels]"""
        if k not in self._x:
            n_frames = 1 + len(self.files[k]) // 160
            rows = [self.e.compute_mel_window(self.files[k], seek).T for seek in range(0, n_frames, 3000)]
            self._x[k] = np.concatenate(rows)[:n_frames].copy()
        return self._x[k]

    def window(self, k, seek, ln):
        return lcr.cut_window(self.norm(k), seek, ln)

    def oracle_kv(self, k, seek, ln):
        if (k, seek, ln) not in self._enc:
            self._enc[(k, seek, ln)] = self.case.oracle_bf16.encoder(self.window(k, seek, ln))
        return self._enc[(k, seek, ln)]

    def oracle_ids(self, k, seek, ln):
        if (k, seek, ln) not in self._dec:
            ck, cv = self.oracle_kv(k, seek, ln)
            self._dec[(k, seek, ln)] = tsr.greedy_ts(self.case.oracle_bf16, ck, cv, self.prefix, max_new=BUDGET, want_logits=True)
        return self._dec[(k, seek, ln)]

    def ids_equal_or_tie(self, k, seek, ln, got, what):
        """The tie rule of test_gpu_longform.py: True: the window's ids equal the oracle's. False: they diverge at a measured tie
        (the oracle's decision margin below 2 x the logit error at that step + 1e-4). Anything else fails."""
        ids, infos, rows = self.oracle_ids(k, seek, ln)
        if list(got) == list(ids):
            return True
        n = min(len(got), len(ids))
        i = next((i for i in range(n) if got[i] != ids[i]), n)
        self.e.encode_mel(self.window(k, seek, ln))
        lg, _ = self.e.decode_forced_timestamps(1, np.array([ids[:i]], dtype=np.int32).reshape(1, i))
        err = float(np.abs(lg[0, i] - rows[i]).max())
        assert infos[i]["margin"] < 2 * err + 1e-4, (what, "file", k, "seek", seek, "len", ln, "step", i, infos[i], "logit err", err, ids, got)
        self.excused += 1
        return False


# The weight seeds. Check 4 needs the windows of one pass to be further apart at the oracle's cross K/V than twice the agree bar, which
# is a property of the oracle and the inputs alone (computed on the CPU, no engine involved). The second pass holds eight windows of
# the 75 s file, which is built from repeats of one 4.2 s clip, and under most seeds two of them come closer than that: seeds 11 / 21 of
# test_gpu_longform.py give 0.031 / 0.035 there, against the 0.04 needed. Of seeds 11 .. 39 (micro) and 21 .. 43 (miniturbo) these are
# the first with both passes above 0.04: 0.061 and 0.045 (micro, 15), 0.050 and 0.045 (miniturbo, 26).
@pytest.fixture(scope="module", params=[("micro", 15, "BF16"), ("miniturbo", 26, "F16")], ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("chunk_" + request.param[0]), *request.param)
    yield m
    m.e.close()


def test_levels_against_float64(model):
    """Check 1: e and s of files 1 and 4 and of the 0.1 s file, three ragged files in ONE launch, against float64 on the GPU's own
    float32 x, within the bound derived from the kernel's sums (long_cuts_reference.levels_bounds)."""
    ks = (1, 4, 0)
    for R in (0, 25, 64):
        got = model.e.long_frame_levels([model.files[k] for k in ks], R)
        for k, (e, s) in zip(ks, got):
            x = model.x(k)
            assert e.shape == s.shape == (1 + len(model.files[k]) // 160,) and (k != 0 or len(e) == 11)
            e_ref, s_ref = lcr.frame_levels(x, R)
            be, bs = lcr.levels_bounds(x, e, R)
            de, ds = np.abs(e - e_ref), np.abs(s - s_ref)
            print("file %d R %d: worst e error %.3g (bound there %.3g), worst s error %.3g (bound there %.3g); worst ratios %.3f %.3f" % (
                k, R, de.max(), be[de.argmax()], ds.max(), bs[ds.argmax()], (de / be).max(), (ds / bs).max()))
            assert (de <= be).all() and (ds <= bs).all(), (k, R)
            assert k == 0 or e.std() > 1e-3  # the levels do follow the audio
            if R == 0:
                assert np.array_equal(e, s)
    # a file gives the same levels alone and beside others
    alone = model.e.long_frame_levels([model.files[4]], 25)[0]
    beside = model.e.long_frame_levels([model.files[k] for k in ks], 25)[1]
    assert np.array_equal(alone[0], beside[0]) and np.array_equal(alone[1], beside[1])


def test_plan_kernel_equals_the_host_rule(model, built_lib):
    """Check 2: exact equality, no tolerance: the plan kernel on the crafted and random levels of the CPU test, and the whole plan call
    on three ragged files against the host rule applied to the levels the same call read back."""
    for name, (s, w_min, w_max) in sorted(lcr.crafted_levels().items()):
        assert model.e.long_cut_plan_from_levels(s, w_min, w_max) == built_lib.long_cut_plan_host(s, w_min, w_max) == lcr.cut_plan(s, w_min, w_max), name
    for k in range(50):
        s = lcr.random_levels(k)
        assert model.e.long_cut_plan_from_levels(s, 200, 300) == built_lib.long_cut_plan_host(s, 200, 300), k
    ks = (3, 0, 4)
    for w_min, w_max, R in ((W_MIN, W_MAX, 25), (2000, 3000, 25), (2, 4, 0), (100, 3000, 64)):
        plans, levels = model.e.long_cut_plan([model.files[k] for k in ks], w_min, w_max, R, levels=True)
        for k, plan, s in zip(ks, plans, levels):
            content = len(model.files[k]) // 160
            assert plan == built_lib.long_cut_plan_host(s, w_min, w_max, content=content) == lcr.cut_plan(s, w_min, w_max, content=content), (k, w_min)
            lcr.check_plan(plan, content, w_min, w_max)
        if R == 25:  # the levels of the plan call are those of the levels call
            for k, s in zip(ks, levels):
                assert np.array_equal(s, model.e.long_frame_levels([model.files[k]], 25)[0][1])
    assert len(plans[2]) >= 3


def test_cut_window_is_the_window_up_to_its_length(model):
    """Check 3: bit-equal to compute_mel_window below len, zero from len on; len = 3000 is the existing call as a whole."""
    pcm = model.files[3]  # 45 s: 4501 frames
    for seek in (37, 1501, 2000):  # (2000: the window runs past the file's end)
        full = model.e.compute_mel_window(pcm, seek)
        valid = min(3000, 4501 - seek)
        assert (full[:, valid:] == 0).all() and np.abs(full[:, :valid]).max() > 0
        for ln in (1, 63, 64, 65, 2999, 3000):
            got = model.e.compute_mel_window_cut(pcm, seek, ln)
            assert np.array_equal(got[:, :ln], full[:, :ln]), (seek, ln)
            assert (got[:, ln:] == 0).all(), (seek, ln)
            if ln == 3000:
                assert np.array_equal(got, full)
    assert (model.e.compute_mel_window_cut(pcm, 0, 0) == 0).all()
    with pytest.raises(RuntimeError, match="len must be"):
        model.e.compute_mel_window_cut(pcm, 0, 3001)


def _flat(logs, ks):
    """the windows of a call in execution order: (file key, window) sorted by (pass, slot)"""
    return sorted(((k, w) for k, log in zip(ks, logs) for w in log), key=lambda kw: (kw[1][4], kw[1][5]))


def _passes_against_the_oracle(model, ks, want_order):
    """The windows of files `ks` (planned: want_order) through the max_passes loop: after a run stopped at pass p every slot holds
    the cross K/V of ITS window and of no other window of the pass; order, compaction, prefixes; ids through the tie rule.
    Returns (windows in execution order, those equal to the oracle id for id)."""
    files = [model.files[k] for k in ks]
    total = len(want_order)
    n_pass = -(-total // 8)
    sizes = [min(8, total - 8 * p) for p in range(n_pass)]
    full = model.e.run_long_chunked_windows(files, max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX)
    flat = _flat(full, ks)
    assert [(k, w[0], w[1]) for k, w in flat] == want_order           # file-then-seek, every window once
    assert all(w[1] == w[2] for _, w in flat)                         # window_frames = advance = len
    assert [(w[4], w[5]) for _, w in flat] == [(i // 8, i % 8) for i in range(total)]  # passes of min(slots, remaining), slots compacted
    kv_checked = 0
    for p in range(1, n_pass + 1):
        logs = model.e.run_long_chunked_windows(files, max_new=BUDGET, max_passes=p, min_frames=W_MIN, max_frames=W_MAX)
        part = _flat(logs, ks)
        assert part == flat[: len(part)] and len(part) == sum(sizes[:p])  # the logs of shorter runs are prefixes
        last = [(k, w) for k, w in part if w[4] == p - 1]
        assert len(last) == sizes[p - 1]
        oracle = [model.oracle_kv(k, w[0], w[1]) for k, w in last]
        # the apart bar: a third of the smallest oracle-to-oracle distance between the windows of this pass (CPU only)
        dist = min(max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max())) for i, a in enumerate(oracle) for b in oracle[i + 1:])
        assert dist > 2 * KV_AGREE, (p, dist)
        apart_bar = dist / 3
        for i, (k, w) in enumerate(last):
            gk, gv = model.e.get_cross_kv(w[5])
            dk, dv = float(np.abs(gk - oracle[i][0]).max()), float(np.abs(gv - oracle[i][1]).max())
            assert dk < KV_AGREE and dv < KV_AGREE, (p, k, w[:2], dk, dv)
            for j, (ok2, ov2) in enumerate(oracle):
                if j != i:
                    apart = max(float(np.abs(gk - ok2).max()), float(np.abs(gv - ov2).max()))
                    assert apart > apart_bar, (p, "slot", w[5], "file", k, "seek", w[0], "looks like window", last[j][1][:2], apart, apart_bar)
            kv_checked += 1
        print("files %s pass %d: %d slots agree with their window (smallest distance between two windows %.3f)" % (ks, p - 1, len(last), dist))
    assert kv_checked == total
    equal = sum(model.ids_equal_or_tie(k, w[0], w[1], w[3], "check 4") for k, w in flat)
    print("files %s: %d of %d windows match the oracle id for id, %d excused by the tie rule" % (ks, equal, total, total - equal))
    assert 5 * equal >= 4 * total, (equal, total)  # the tie cap: excused ties must not hide a failure
    return flat, equal


def test_passes_against_the_oracle(model):
    """Check 4: the 45 s and the 75 s file together, W = 600 / 1000, 8 slots (_passes_against_the_oracle says what is checked); a
    file's plan alone and beside other files. These two files give 6 + 10 windows, two FULL passes, so the same checks run once more
    with the 12 s file behind them: its two windows are a last pass that does not fill the slots."""
    ks = (3, 4, 1)
    plans = model.e.long_cut_plan([model.files[k] for k in ks], W_MIN, W_MAX)
    for k, plan in zip(ks, plans):  # a file's plan is identical alone and beside other files
        assert model.e.long_cut_plan([model.files[k]], W_MIN, W_MAX)[0] == plan
    assert model.e.long_cut_plan([model.files[3], model.files[4]], W_MIN, W_MAX) == plans[:2]
    order = [(k, seek, ln) for k, plan in zip(ks, plans) for seek, ln in plan]  # file-then-seek
    two = len(plans[0]) + len(plans[1])
    print("windows per file", [len(p) for p in plans])
    assert two >= 9 and len(order) % 8 != 0  # several passes; the last one of the three-file call is not full
    flat2, _ = _passes_against_the_oracle(model, (3, 4), order[:two])
    flat3, _ = _passes_against_the_oracle(model, ks, order)
    assert flat3[:two] == flat2  # the same windows in the same slots: the same log


def test_segments_in_file_time(model):
    """Check 5: run_long_chunked's segments are ChunkedSegments in Python on the engine's own ids; starts never go backwards."""
    pcm = model.files[4]
    wins = model.e.run_long_chunked_windows([pcm], max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX)[0]
    want = []
    for seek, wf, _adv, ids, _p, _s in wins:
        for s, e, tb, te in lcr.chunked_segments(ids, model.T, model.E, seek, wf):
            assert seek * 0.01 - 1e-9 <= s <= e <= (seek + wf) * 0.01 + 1e-9
            want.append((s, e, model.e.transcript(ids[tb:te])))
    got = model.e.run_long_chunked(pcm, max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX)
    assert len(got) == len(want) >= len(wins) >= 3
    for (s, e, t), (ws, we, wt) in zip(got, want):
        assert abs(s - ws) < 1e-9 and abs(e - we) < 1e-9 and t == wt
    assert all(b[0] >= a[0] - 1e-9 for a, b in zip(got, got[1:]))
    assert got[-1][1] > 60.0  # times from the file's start


def test_scored_variant(model):
    """Check 6: every window carries its two numbers, skipped is long_window_is_silent on them, a skipped window emits nothing."""
    pcm = model.files[3]
    plain = model.e.run_long_chunked_windows([pcm], max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX)[0]
    for nst, lpt in ((None, None), (0.0, None), (0.5, -1.0), (1e-30, 100.0)):
        wins = model.e.run_long_chunked_windows([pcm], max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX, no_speech_threshold=nst,
                                                logprob_threshold=lpt, scores=True)[0]
        assert [w[:6] for w in wins] == [w[:6] for w in plain]  # the scored mode decodes what the timestamp mode decodes
        a, b = (float("nan") if nst is None else nst), (float("inf") if lpt is None else lpt)
        for w in wins:
            assert np.isfinite(w[6]) and w[6] <= 0 and np.isfinite(w[7])
            assert w[8] == model.lib.long_window_is_silent(w[6], w[7], a, b), (nst, lpt, w[6:])
        if nst is not None:
            segs = model.e.run_long_chunked(pcm, max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX, no_speech_threshold=nst, logprob_threshold=lpt)
            kept = [w for w in wins if not w[8]]
            assert len(segs) == sum(len(lcr.chunked_segments(w[3], model.T, model.E, w[0], w[1])) for w in kept)
            if nst == 0.0:
                assert all(w[8] for w in wins) and segs == []  # every no-speech probability is above 0
    # a language and a task per file: the handle's own language gives the same windows
    both = model.e.run_long_chunked_windows([pcm, model.files[1]], max_new=BUDGET, min_frames=W_MIN, max_frames=W_MAX, languages=["zh", None],
                                            tasks=["transcribe", "transcribe"])
    assert [w[:4] for w in both[0]] == [w[:4] for w in plain]


def test_existing_calls_are_unchanged_by_chunked_calls(built_lib, model):
    """Check 7, on a fresh handle: the seek loop, the timestamp entry point and run before and after chunked calls."""
    e = built_lib.Whisper(model.case.model_type, model.case.root, "zh", device=0, max_batch=4)
    try:
        pcm = model.files[3]
        clips = [model.files[1], pcm[:100000]]
        before = (e.run_long_windows([pcm, model.files[1]], max_new=6), e.run_timestamp_tokens_batch(clips, max_new=24), e.run(model.files[1]),
                  e.compute_mel_window(pcm, 1234))
        e.run_long_chunked_windows([pcm, model.files[1]], max_new=6, min_frames=W_MIN, max_frames=W_MAX)
        e.long_frame_levels([pcm], 25)
        e.long_cut_plan([pcm])
        e.compute_mel_window_cut(pcm, 77, 100)
        e.long_cut_plan_from_levels(lcr.random_levels(0), 200, 300)
        after = (e.run_long_windows([pcm, model.files[1]], max_new=6), e.run_timestamp_tokens_batch(clips, max_new=24), e.run(model.files[1]),
                 e.compute_mel_window(pcm, 1234))
        assert before[:3] == after[:3] and np.array_equal(before[3], after[3])
    finally:
        e.close()


def test_refusals(model, built_lib, monkeypatch):
    """Check 8: everything the mode does not cover is refused with its text, and the handle works afterwards."""
    pcm = model.files[1]
    run = lambda **kw: model.e.run_long_chunked_windows([pcm], max_new=2, **kw)
    for kw, text in (({"languages": ["auto"]}, "language detection"),
                     ({"temperatures": [0.0, 0.4]}, "temperatures"),
                     ({"compression_ratio_threshold": 2.4}, "temperature"),
                     ({"initial_prompt_ids": [[5, 6, 7]]}, "prompts"),
                     ({"condition_on_previous_text": True}, "condition_on_previous_text"),
                     ({"word_timestamps": True}, "word timestamps"),
                     ({"beam_size": 5}, "beam search"),
                     ({"min_frames": 601}, "must be even"),
                     ({"max_frames": 999, "min_frames": 600}, "must be even"),
                     ({"min_frames": 1000, "max_frames": 600}, "chunk_min_frames <= chunk_max_frames"),
                     ({"max_frames": 3002}, "<= 3000"),
                     ({"min_frames": 0}, "2 <= chunk_min_frames"),
                     ({"smooth_frames": 65}, "smooth_frames must be 0 .. 64"),
                     ({"smooth_frames": -1}, "smooth_frames must be 0 .. 64")):
        with pytest.raises(RuntimeError, match=re.escape(text)):
            run(**kw)
        assert len(run()[0]) == 1  # the handle still works: 12 s is one window
    with pytest.raises(RuntimeError, match="smooth_frames"):
        model.e.long_frame_levels([pcm], 65)
    with pytest.raises(RuntimeError, match="must be even"):
        model.e.long_cut_plan([pcm], 601, 1000)
    with pytest.raises(RuntimeError, match="must be even"):
        model.e.long_cut_plan_from_levels(lcr.random_levels(0), 200, 301)
    bad = lcr.random_levels(0)
    bad[5] = np.inf
    with pytest.raises(RuntimeError, match="not finite"):
        model.e.long_cut_plan_from_levels(bad, 200, 300)
    monkeypatch.setenv("AX_WHISPER_LONG_MAX_BYTES", "1000000")
    with pytest.raises(RuntimeError, match="AX_WHISPER_LONG_MAX_BYTES"):  # the levels count towards the cap
        model.e.run_long_chunked_windows([model.files[4]], max_new=2)
    monkeypatch.delenv("AX_WHISPER_LONG_MAX_BYTES")
    assert model.e.bench("long_cut_plan", 2, 45, 2) > 0  # the bench target runs
    assert len(run()[0]) == 1
    monkeypatch.setenv("AX_WHISPER_FEATURE_MODE", "openai")
    o = built_lib.Whisper(model.case.model_type, model.case.root, "zh", device=0, max_batch=1)
    try:
        with pytest.raises(RuntimeError, match="openai"):
            o.run_long_chunked_windows([pcm], max_new=2)
        with pytest.raises(RuntimeError, match="openai"):
            o.long_cut_plan([pcm])
    finally:
        o.close()


def test_cli_chunked_lines(model, built_lib, tmp_path):
    """Check 9: whisper_cli --long --chunked on a 75 s WAV against the Python call (same parameters, same number of slots)."""
    cli = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_cli")
    wav = str(tmp_path / "long75.wav")
    pcm16 = np.clip(np.round(model.files[4] * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm16.tobytes())
    pcm = pcm16.astype(np.float32) / np.float32(32768.0)
    args = [cli, "-w", wav, "-t", model.case.model_type, "-p", model.case.root, "--language", "zh", "--long", "--chunked", "--chunk_max_s", "10",
            "--chunk_min_s", "6", "--chunk_smooth_ms", "510"]
    r = subprocess.run(args, capture_output=True, timeout=600, env=dict(os.environ, AX_WHISPER_MAX_BATCH="8"))
    assert r.returncode == 0, r.stderr
    out = r.stdout.decode("utf-8", "replace")
    rest = out.split("\nResult: ", 1)[1]
    want = model.e.run_long_chunked(pcm, min_frames=W_MIN, max_frames=W_MAX, smooth_frames=25)
    text = "".join(t for _, _, t in want)
    assert rest.startswith(text + "\n")
    block = rest[len(text) + 1: rest.rindex("RTF: ")]
    hdr = re.compile(r"(?m)^\[(\d\d+):(\d\d)\.(\d\d\d) --> (\d\d+):(\d\d)\.(\d\d\d)\] ")
    heads = list(hdr.finditer(block))
    assert heads and heads[0].start() == 0, block[:200]
    parsed = []
    for j, m in enumerate(heads):
        g = m.groups()
        t = block[m.end(): heads[j + 1].start() if j + 1 < len(heads) else len(block)]
        assert t.endswith("\n")
        parsed.append((int(g[0]) * 60 + int(g[1]) + int(g[2]) / 1000, int(g[3]) * 60 + int(g[4]) + int(g[5]) / 1000, t[:-1]))
    assert len(parsed) == len(want)
    for (s, e, t), (ws, we, wt) in zip(parsed, want):
        assert abs(s - ws) < 6e-4 and abs(e - we) < 6e-4 and t == wt
    assert parsed[-1][1] > 60.0
    # without --long the flag is refused before anything is loaded
    bad = subprocess.run([cli, "-w", wav, "-t", model.case.model_type, "-p", model.case.root, "--chunked"], capture_output=True, timeout=60)
    assert bad.returncode == 1 and b"--chunked needs --long" in bad.stderr
