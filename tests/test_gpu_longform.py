"""GPU: long-form transcription (DESIGN.md "Long-form") — the whole-file front-end and the window kernel against the numpy
reference, the seek loop's windows against the oracle pass by pass (content pinned at the cross K/V: on synthetic weights
neither ids nor logits depend on the audio), files in a batch against files alone, groups and two engines, the text entry
points, isolation from the existing entry points, and the CLI's --long lines.

Inputs: five files of 12 s, exactly 30 s, 45 s, 75 s and 100 s built from demo.wav (longform_reference.make_file). Per-window
budgets 48 and 6 on all five, 4 and 2 on the 45 s file alone."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import longform_reference as lfr
import ts_reference as tsr
from conftest import ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

ORC_BUDGET = 48   # the oracle decodes every window once at the largest budget; smaller budgets are prefixes
KV_AGREE = 2e-2   # the cross-K/V bar of test_gpu_parity.py
KV_APART = 4e-2   # twice that, a third of the smallest distance between two windows of these files (0.132 / 0.158)
MEL_BAR = 2e-4    # the front-end bar of test_gpu_parity.py


class Model:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        self.lib = built_lib
        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=8)
        self.T, self.E, self.nm = self.e.timestamp_begin, self.e.eot, self.case.dims["n_mels"]
        demo = load_demo_pcm()
        self.files = {k: lfr.make_file(demo, k) for k in range(1, 6)}
        self.norm = {k: lfr.file_log_mel(self.files[k], self.nm)[0] for k in range(1, 6)}
        self.prefix = self.case.oracle_bf16.sot_seq("zh")[:3]
        self._enc, self._dec, self._alone = {}, {}, {}
        self.excused = 0
        self.branches = set()

    def window(self, k, seek):
        return lfr.window_of(self.norm[k], seek)

    def oracle_kv(self, k, seek):
        if (k, seek) not in self._enc:
            self._enc[(k, seek)] = self.case.oracle_bf16.encoder(self.window(k, seek))
        return self._enc[(k, seek)]

    def oracle_ids(self, k, seek, budget):
        """(ids, infos, logits rows) of the oracle's timestamp-mode loop on the window of file k at seek"""
        if (k, seek) not in self._dec:
            ck, cv = self.oracle_kv(k, seek)
            self._dec[(k, seek)] = tsr.greedy_ts(self.case.oracle_bf16, ck, cv, self.prefix, max_new=ORC_BUDGET, want_logits=True)
        ids, infos, rows = self._dec[(k, seek)]
        assert 0 < budget <= ORC_BUDGET
        return ids[:budget], infos, rows

    def ids_equal_or_tie(self, k, seek, budget, got, what):
        """True: the window's ids equal the oracle's. False: they diverge at a measured tie (test_gpu_timestamps.py:91-95: the
        oracle's decision margin below 2 x the logit error at that step + 1e-4). Anything else fails."""
        ids, infos, rows = self.oracle_ids(k, seek, budget)
        if list(got) == list(ids):
            return True
        n = min(len(got), len(ids))
        i = next((i for i in range(n) if got[i] != ids[i]), n)
        self.e.encode_mel(self.window(k, seek))
        lg, _ = self.e.decode_forced_timestamps(1, np.array([ids[:i]], dtype=np.int32).reshape(1, i))
        err = float(np.abs(lg[0, i] - rows[i]).max())
        assert infos[i]["margin"] < 2 * err + 1e-4, (what, "file", k, "seek", seek, "step", i, infos[i], "logit err", err, ids, got)
        self.excused += 1
        return False

    def alone(self, k, budget):
        if (k, budget) not in self._alone:
            self._alone[(k, budget)] = self.e.run_long_windows([self.files[k]], max_new=budget)[0]
        return self._alone[(k, budget)]

    def same_as_alone(self, k, budget, log, what):
        """A file's log equals the log of the same file run alone, except from a window excused by the tie rule on"""
        ref = self.alone(k, budget)
        for w, r in zip(log, ref):
            if w[:4] == r[:4]:
                continue
            assert w[0] == r[0] and w[1] == r[1], (what, k, w[:3], r[:3])  # same window, different ids
            ok_w = self.ids_equal_or_tie(k, w[0], budget, w[3], what)
            ok_r = self.ids_equal_or_tie(k, r[0], budget, r[3], what + " (alone)")
            assert not (ok_w and ok_r)
            return
        assert len(log) == len(ref), (what, k, len(log), len(ref))


@pytest.fixture(scope="module", params=[("micro", 11, "BF16"), ("miniturbo", 21, "F16")], ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("long_" + request.param[0]), *request.param)
    yield m
    m.e.close()


def test_front_end_windows(model):
    """Check 1: seek 0 is bit-equal to compute_mel; other seeks agree with the numpy reference; zero past the file's end."""
    for k in (1, 4):
        pcm = model.files[k]
        assert np.array_equal(model.e.compute_mel_window(pcm, 0), model.e.compute_mel(pcm)), k
        n_frames = 1 + len(pcm) // 160
        last30, last1 = max(n_frames - 2000, 3), n_frames - 50
        for seek in (1, 2, 1499, 3000, last30, last1):
            got = model.e.compute_mel_window(pcm, seek)
            want = model.window(k, seek)
            err = float(np.abs(got - want).max())
            print("file %d seek %d: max |d| = %.3g" % (k, seek, err))
            assert err < MEL_BAR, (k, seek, err)
            valid = max(0, min(3000, n_frames - seek))
            assert (got[:, valid:] == 0).all(), (k, seek)
            if valid:
                assert np.abs(got[:, :valid]).max() > 0


def test_first_window_is_the_timestamp_entry_point(model):
    """Check 2: window 0 has seek 0 and exactly the ids of run_timestamp_tokens_batch on the same input and budget."""
    for budget, ks in ((48, (1, 2, 3, 4, 5)), (6, (1, 2, 3, 4, 5)), (4, (3,)), (2, (3,))):
        for k in ks:
            log = model.alone(k, budget)
            want = model.e.run_timestamp_tokens_batch([model.files[k]], max_new=budget)[0]
            assert log[0][0] == 0 and log[0][3] == want, (budget, k, log[0], want)
            assert log[0][4] == 0 and log[0][5] == 0
    assert len(model.alone(1, 48)) == 1 and len(model.alone(1, 6)) == 1  # 12 s: one window


def _check_log_against_python(model, k, budget, log):
    """seek chain, window_frames and advance against the Python rule on the engine's own ids; ids against the oracle"""
    content = len(model.files[k]) // 160
    seek = 0
    for i, (s, wf, adv, ids, _p, _sl) in enumerate(log):
        assert s == seek, (k, budget, i, s, seek)             # previous seek + the rule's advance on the engine's previous ids
        assert wf == min(3000, content - s)
        _, padv, branch = lfr.split_window(ids, model.T, model.E, wf)
        assert adv == padv and adv >= 1
        model.branches.add(branch)
        model.ids_equal_or_tie(k, s, budget, ids, "budget %d" % budget)
        seek = s + adv
    return seek


@pytest.mark.parametrize("budget,ks", [(48, (1, 2, 3, 4, 5)), (6, (3, 5))], ids=["budget48_five_files", "budget6_two_files"])
def test_every_pass_against_the_oracle(model, budget, ks):
    """Check 3: after a run stopped at pass p, every slot holds the cross K/V of ITS window (agrees with the oracle's encoder on
    the numpy window of that file at that seek) and of no other window of the pass nor the file's previous window."""
    files = [model.files[k] for k in ks]
    prev_logs, asked, kv_checked = None, 0, 0
    while True:
        asked += 1
        logs = model.e.run_long_windows(files, max_new=budget, max_passes=asked)
        n_pass = 1 + max(w[4] for log in logs for w in log)
        if prev_logs is not None:  # the logs of the runs are prefixes of one another
            for a, b in zip(prev_logs, logs):
                assert b[: len(a)] == a
        if n_pass < asked:
            break
        assert n_pass == asked
        last = [(ks[f], w) for f, log in enumerate(logs) for w in log if w[4] == asked - 1]
        assert sorted(w[5] for _, w in last) == list(range(len(last)))  # compacted into slots 0..A-1
        others = {(k, w[0]) for k, w in last}
        for f, log in enumerate(logs):
            if len(log) >= 2 and log[-1][4] == asked - 1:
                others.add((ks[f], log[-2][0]))  # the same file's previous window
        for k, w in last:
            gk, gv = model.e.get_cross_kv(w[5])
            ok, ov = model.oracle_kv(k, w[0])
            dk, dv = float(np.abs(gk - ok).max()), float(np.abs(gv - ov).max())
            assert dk < KV_AGREE and dv < KV_AGREE, (asked, k, w[0], dk, dv)
            for (k2, s2) in others:
                if (k2, s2) == (k, w[0]):
                    continue
                ok2, ov2 = model.oracle_kv(k2, s2)
                apart = max(float(np.abs(gk - ok2).max()), float(np.abs(gv - ov2).max()))
                assert apart > KV_APART, (asked, "slot", w[5], "file", k, "seek", w[0], "looks like file", k2, "seek", s2, apart)
            kv_checked += 1
        prev_logs = logs
    sizes = [sum(1 for log in prev_logs for w in log if w[4] == p) for p in range(asked - 1)]
    print("budget %d: passes of %s windows, %d slots checked at the cross K/V" % (budget, sizes, kv_checked))
    for f, k in enumerate(ks):
        end = _check_log_against_python(model, k, budget, prev_logs[f])
        assert end == len(model.files[k]) // 160  # every file's last window ends at content_frames
        seeks = [w[0] for w in prev_logs[f]]
        assert all(b > a for a, b in zip(seeks, seeks[1:]))
    if budget == 48:
        assert len(set(sizes)) >= 3, sizes  # check 4: passes of at least three different sizes
        for f, k in enumerate(ks):            # check 4: every file's log equals the same file run alone
            model.same_as_alone(k, budget, prev_logs[f], "five files")
    print("windows excused by the tie rule so far:", model.excused)


def test_small_budgets_on_the_45s_file(model):
    """Budgets 4 and 2 on the 45 s input alone (budget 4: the micro model advances 2 s per window)."""
    for budget in (4, 2):
        log = model.alone(3, budget)
        assert _check_log_against_python(model, 3, budget, log) == 4500
        print("budget %d: %d windows" % (budget, len(log)))
    for budget in (48, 6):
        _check_log_against_python(model, 3, budget, model.alone(3, budget))
    print("windows excused by the tie rule so far:", model.excused, "branches", sorted(model.branches))
    assert model.branches == {"none", "cuts", "single_end"}


def test_groups_and_two_engines(model, built_lib, monkeypatch):
    """Check 5: more files than capacity, and two engines on one device, give the single-file logs."""
    ks = (1, 2, 3, 4, 5)
    files = [model.files[k] for k in ks]
    small = built_lib.Whisper(model.case.model_type, model.case.root, "zh", device=0, max_batch=2)
    try:
        logs = small.run_long_windows(files, max_new=48)
        assert max(w[5] for log in logs for w in log) == 1  # never more than two windows side by side
        for f, k in enumerate(ks):
            model.same_as_alone(k, 48, logs[f], "max_batch 2")
    finally:
        small.close()
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    two = built_lib.Whisper(model.case.model_type, model.case.root, "zh", devices=[0, 0], max_batch=4)
    try:
        logs = two.run_long_windows(files, max_new=48)
        for f, k in enumerate(ks):
            model.same_as_alone(k, 48, logs[f], "two engines")
    finally:
        two.close()


def test_text_entry_points(model):
    """Check 6: run_long / RunPCMLong = the transcripts of the Python rule's segments of the logged windows."""
    pcm = model.files[4]
    log = model.e.run_long_windows([pcm])[0]
    want = []
    for seek, wf, adv, ids, _p, _s in log:
        for s, e, tb, te in lfr.split_window(ids, model.T, model.E, wf)[0]:
            want.append((seek * 0.01 + s, seek * 0.01 + e, model.e.transcript(ids[tb:te])))
    got = model.e.run_long(pcm)
    assert len(got) == len(want) >= 1
    for (s, e, t), (ws, we, wt) in zip(got, want):
        assert abs(s - ws) < 1e-5 and abs(e - we) < 1e-5 and t == wt
    assert all(b[0] >= a[0] and a[1] >= a[0] for a, b in zip(got, got[1:]))  # absolute, non-decreasing
    assert model.e.run_long_text(pcm) == "".join(t for _, _, t in want)
    # the progress guard, GPU-free
    assert model.lib.split_window([model.T, model.T, 5], model.T, model.E, 640)[1] == 640


def test_existing_entry_points_are_unchanged_by_long_form_calls(built_lib, model):
    """Check 7, on a fresh handle: plain and timestamp entry points before and after long-form calls."""
    e = built_lib.Whisper(model.case.model_type, model.case.root, "zh", device=0, max_batch=4)
    try:
        pcm = model.files[4]
        clips = [model.files[1], model.files[2][:100000], pcm]
        before = (e.run_tokens(pcm, max_new=24), e.run_tokens_batch(clips, max_new=24), e.run_timestamp_tokens_batch(clips, max_new=24),
                  e.compute_mel(pcm))
        e.run_long_windows([pcm, model.files[3]], max_new=6)
        e.compute_mel_window(pcm, 1234)
        after = (e.run_tokens(pcm, max_new=24), e.run_tokens_batch(clips, max_new=24), e.run_timestamp_tokens_batch(clips, max_new=24),
                 e.compute_mel(pcm))
        assert before[:3] == after[:3] and np.array_equal(before[3], after[3])
    finally:
        e.close()


def test_refusals(model, built_lib, monkeypatch):
    """A call beyond the memory cap, a log that does not fit, and the openai front-end are refused with an error text."""
    monkeypatch.setenv("AX_WHISPER_LONG_MAX_BYTES", "1000000")
    with pytest.raises(RuntimeError, match="AX_WHISPER_LONG_MAX_BYTES"):
        model.e.run_long_windows([model.files[4]], max_new=2)
    monkeypatch.delenv("AX_WHISPER_LONG_MAX_BYTES")
    assert len(model.e.run_long_windows([model.files[1]], max_new=2)[0]) == 1  # the handle still works
    # win_cap too small: -1 with the needed count, nothing written
    import ctypes as C

    pcm = model.files[3]
    ptrs, lens = (built_lib.fp * 1)(pcm.ctypes.data_as(built_lib.fp)), (C.c_int * 1)(len(pcm))
    info, ids, nw = np.full((1, 7), -7, dtype=np.int32), np.full((1, model.e.n_text_ctx), -7, dtype=np.int32), C.c_int(-1)
    rc = model.e.L.AX_WHISPER_RunPCMLongWindows(model.e.h, ptrs, lens, 1, 6, 0, 1, info.ctypes.data_as(C.POINTER(C.c_int)),
                                                ids.ctypes.data_as(built_lib.ip), C.byref(nw))
    assert rc == -1 and b"2 windows were decoded, win_cap is 1" in model.e.L.AX_WHISPER_LastError(model.e.h)
    assert nw.value == 0 and (info == -7).all() and (ids == -7).all()
    assert model.e.bench("frontend_long", 2, 45, 2) > 0  # the bench target runs (whole-file front-end + window kernel)
    monkeypatch.setenv("AX_WHISPER_FEATURE_MODE", "openai")
    o = built_lib.Whisper(model.case.model_type, model.case.root, "zh", device=0, max_batch=1)
    try:
        with pytest.raises(RuntimeError, match="openai"):
            o.run_long_windows([model.files[1]], max_new=2)
        with pytest.raises(RuntimeError, match="openai"):
            o.compute_mel_window(model.files[1], 0)
    finally:
        o.close()


def test_cli_long_lines(model, built_lib, tmp_path):
    """Check 8: whisper_cli --long on a 75 s WAV; without the flag the output is the first window's plain text as before."""
    cli = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_cli")
    wav = str(tmp_path / "long75.wav")
    pcm16 = np.clip(np.round(model.files[4] * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm16.tobytes())
    pcm = pcm16.astype(np.float32) / np.float32(32768.0)
    args = [cli, "-w", wav, "-t", model.case.model_type, "-p", model.case.root, "--language", "zh"]
    plain = subprocess.run(args, capture_output=True, timeout=600)
    r = subprocess.run(args + ["--long"], capture_output=True, timeout=600)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr
    out, ref = r.stdout.decode("utf-8", "replace"), plain.stdout.decode("utf-8", "replace")
    head, rest = out.split("\nResult: ", 1)
    rhead, rrest = ref.split("\nResult: ", 1)
    strip = lambda h: [l for l in h.splitlines() if not l.startswith("Init whisper success")]
    assert strip(head) == strip(rhead)
    assert rrest[: rrest.rindex("\nRTF: ")] == model.e.run(wav)  # without --long: the first window's plain text, as before
    assert re.fullmatch(r"RTF: \d+\.\d{4}\n", rrest[rrest.rindex("RTF: "):]) and re.fullmatch(r"RTF: \d+\.\d{4}\n", rest[rest.rindex("RTF: "):])
    want = model.e.run_long(pcm)
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
    assert parsed[-1][1] > 30.0  # times from the file's start
