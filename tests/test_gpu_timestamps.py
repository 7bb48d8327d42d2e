"""GPU: segment timestamps — the rules kernel against the Python rules (tests/ts_reference.py) on crafted rows and on the
engine's own logits, timestamp-mode greedy ids against the oracle loop, ragged budgets and sharding, isolation from the
plain mode, and the CLI's --timestamps lines."""
import os
import re
import subprocess

import numpy as np
import pytest

import ts_reference as tsr
from conftest import GOLDEN, ModelCase, load_demo_pcm

pytestmark = pytest.mark.gpu

MAX_NEW = 48


def _clips():
    pcm = load_demo_pcm()
    n = len(pcm)
    return [pcm, pcm[: n * 2 // 3] * np.float32(0.7), pcm[n // 5:], np.concatenate([pcm[n // 3:], pcm[: n // 3]]) * np.float32(1.3)]


class Model:
    def __init__(self, built_lib, tmp, model_type, seed, dtype):
        import oracle

        self.case = ModelCase(tmp, model_type, seed, dtype=dtype)
        self.e = built_lib.Whisper(model_type, self.case.root, "zh", device=0, max_batch=24)
        self.T, self.E = self.e.timestamp_begin, self.e.eot
        assert self.T == int(self.case.cfg["no_timestamps"]) + 1 and self.e.n_vocab - self.T == 1501
        self.clips = _clips()
        self.mels = [oracle.log_mel(c, self.case.dims["n_mels"])[0] for c in self.clips]
        self.prefix = self.case.oracle_bf16.sot_seq("zh")[:3]
        self._orc = {}

    def oracle_run(self, k):
        """(ids, infos, logits rows) of the oracle's timestamp-mode loop on clip k"""
        if k not in self._orc:
            orc = self.case.oracle_bf16
            ck, cv = orc.encoder(self.mels[k])
            self._orc[k] = tsr.greedy_ts(orc, ck, cv, self.prefix, max_new=MAX_NEW, want_logits=True)
        return self._orc[k]


@pytest.fixture(scope="module", params=[("micro", 11, "BF16"), ("miniturbo", 21, "F16")], ids=["micro_bf16", "miniturbo_fp16"])
def model(request, built_lib, oracle_mod, tmp_path_factory):
    m = Model(built_lib, tmp_path_factory.mktemp("ts_" + request.param[0]), *request.param)
    yield m
    m.e.close()


def test_kernel_on_crafted_rows(model):
    cases = tsr.crafted_cases(model.e.n_vocab)
    got = model.e.apply_timestamp_rules(np.stack([x for _, x, _, _ in cases]), [seq for _, _, seq, _ in cases])
    for (name, x, seq, want), g in zip(cases, got):
        assert g == want, (name, g, want)


@pytest.mark.parametrize("batch", [1, 3])
def test_kernel_on_real_rows(model, batch):
    """Teacher-forced with the oracle's ids: each step's choice equals the Python rules on the GPU's own dumped row, except
    where that row's decision margin is below 1e-4."""
    ids, _, _ = model.oracle_run(0)
    model.e.encode_mel(np.stack(model.mels[:batch]))
    logits, chosen = model.e.decode_forced_timestamps(batch, np.array([ids] * batch, dtype=np.int32).reshape(batch, len(ids)))
    assert chosen.shape == (batch, len(ids) + 1)
    for b in range(batch):
        for i in range(len(ids) + 1):
            py, info = tsr.decide(logits[b, i], ids[:i], model.T, model.E)
            if chosen[b, i] != py:
                assert info["margin"] < 1e-4, (b, i, int(chosen[b, i]), py, info)


@pytest.mark.parametrize("batch", [1, 2, 4, 16, 24])
def test_greedy_ids_match_the_oracle(model, batch):
    clips = [model.clips[b % len(model.clips)] for b in range(batch)]
    got = model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW)
    seen5, seen2 = set(), set()
    for b in range(batch):
        k = b % len(model.clips)
        ids, infos, rows = model.oracle_run(k)
        seen5 |= {i["rule5"] for i in infos}
        seen2 |= {i["branch2"] for i in infos}
        g = got[b]
        if g == ids:
            continue
        n = min(len(g), len(ids))
        i = next((i for i in range(n) if g[i] != ids[i]), n)
        # the first divergence only as a measured tie: the oracle's decision margin there below 2x the logit error at that step
        model.e.encode_mel(model.mels[k])
        lg, _ = model.e.decode_forced_timestamps(1, np.array([ids[:i]], dtype=np.int32).reshape(1, i))
        err = float(np.abs(lg[0, i] - rows[i]).max())
        assert infos[i]["margin"] < 2 * err + 1e-4, (batch, b, "step", i, infos[i], "logit err", err, ids, g)
    assert seen5 == {True, False} and {"open", "closed"} <= seen2  # both outcomes of rule 5, both branches of rule 2


def test_ragged_budgets_and_sharding(model, built_lib, monkeypatch):
    clips = model.clips[:4]
    budgets = [5, 0, 17, 9]
    full = model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW)
    rag = model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW, max_new_clip=budgets)
    for f, r, m in zip(full, rag, budgets):
        assert r == (f[:m] if m > 0 else f)
    one = [model.e.run_timestamp_tokens_batch([c], max_new=m if m > 0 else MAX_NEW)[0] for c, m in zip(clips[:2], budgets[:2])]
    monkeypatch.setenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES", "1")
    two = built_lib.Whisper(model.case.model_type, model.case.root, "zh", devices=[0, 0], max_batch=2)
    try:
        assert two.run_timestamp_tokens_batch(clips[:2], max_new=MAX_NEW, max_new_clip=budgets[:2]) == one  # one clip per engine
    finally:
        two.close()


def test_plain_mode_is_unchanged_by_timestamp_calls(model):
    clips = model.clips[:4]
    before = model.e.run_tokens_batch(clips, max_new=MAX_NEW)
    one_before = model.e.run_tokens(clips[0], max_new=MAX_NEW)
    ts = model.e.run_timestamp_tokens_batch(clips, max_new=MAX_NEW)
    assert any(t >= model.T for t in ts[0])
    assert model.e.run_tokens_batch(clips, max_new=MAX_NEW) == before
    assert model.e.run_tokens(clips[0], max_new=MAX_NEW) == one_before
    assert all(t < model.T for ids in before for t in ids)  # plain ids hold no timestamp


def test_cli_timestamp_lines(model, built_lib):
    cli = os.path.join(os.path.dirname(built_lib.LIB_PATH), "whisper_cli")
    wav = os.path.join(GOLDEN, "demo.wav")
    args = [cli, "-w", wav, "-t", model.case.model_type, "-p", model.case.root, "--language", "zh"]
    plain = subprocess.run(args, capture_output=True, timeout=300)
    r = subprocess.run(args + ["--timestamps"], capture_output=True, timeout=300)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr
    out, ref = r.stdout.decode("utf-8", "replace"), plain.stdout.decode("utf-8", "replace")
    head, rest = out.split("\nResult: ", 1)
    rhead, rrest = ref.split("\nResult: ", 1)
    strip = lambda h: [l for l in h.splitlines() if not l.startswith("Init whisper success")]
    assert strip(head) == strip(rhead)
    result = rrest[: rrest.rindex("\nRTF: ")]
    assert rest.startswith(result + "\n")  # Result: as without the flag, then the segment lines, then RTF
    block = rest[len(result) + 1: rest.rindex("RTF: ")]
    hdr = re.compile(r"(?m)^\[(\d\d):(\d\d)\.(\d\d\d) --> (\d\d):(\d\d)\.(\d\d\d)\] ")
    heads = list(hdr.finditer(block))
    assert heads and heads[0].start() == 0, block[:200]
    parsed = []
    for j, m in enumerate(heads):
        g = m.groups()
        text = block[m.end(): heads[j + 1].start() if j + 1 < len(heads) else len(block)]
        assert text.endswith("\n")
        parsed.append((int(g[0]) * 60 + int(g[1]) + int(g[2]) / 1000, int(g[3]) * 60 + int(g[4]) + int(g[5]) / 1000, text[:-1]))
    pcm = load_demo_pcm()
    ids = model.e.run_timestamp_tokens_batch([pcm])[0]
    want = model.e.segments(ids, len(pcm))
    assert len(parsed) == len(want) and len(want) >= 1
    for (s, e, t), (ws, we, wt) in zip(parsed, want):
        assert abs(s - ws) < 6e-4 and abs(e - we) < 6e-4 and t == wt
