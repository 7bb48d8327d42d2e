"""GPU: the long-form entry points against each other (DESIGN.md "Long-form entry points"). Every kind of result has one body in
api.cpp and every export is an adapter to it, so what is asserted here is that the adapters of one kind agree: the PCM form and the
file form of every text pair return the same string, that string is the text of the windows the matching window-log call returns
on the same handle, and the Lang and Words window logs are the same call when word timestamps are off.
Micro model, two files (12 s: one window; 40 s: at least two), seed 77. The text forms have no id budget in the C ABI, so the window
logs they are compared with run without one; the Lang / Words comparison runs under a budget of 8 ids.
Already asserted elsewhere and not repeated: RunPCMLong against the windows of RunPCMLongWindows
(test_gpu_longform.py::test_text_entry_points)."""
import ctypes as C
import wave

import numpy as np
import pytest

import longform_reference as lfr
from conftest import load_demo_pcm

pytestmark = pytest.mark.gpu

SEED = 77
PROMPT = [100, 200, 300]
W_MIN, W_MAX = 600, 1000  # the cut bounds of the chunked pair


@pytest.fixture(scope="module")
def setup(built_lib, micro_case, tmp_path_factory):
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=8)
    demo = load_demo_pcm()
    tmp = tmp_path_factory.mktemp("entry_points")
    files, wavs = [], []
    for name, pcm in (("f12", lfr.make_file(demo, 1)), ("f40", lfr.make_file(demo, 3)[: 40 * 16000])):
        pcm16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype(np.int16)  # what the file holds is what the PCM form gets
        wavs.append(str(tmp / (name + ".wav")))
        with wave.open(wavs[-1], "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(pcm16.tobytes())
        files.append(pcm16.astype(np.float32) / np.float32(32768.0))
    yield built_lib, e, files, wavs
    e.close()


def _joined(lib, e, windows, language=None):
    """the text of one file's window log: its kept, not skipped windows, the segments of the window rule, their transcripts"""
    text = ""
    for w in windows:
        seek, wf, _adv, ids = w[:4]
        if (len(w) > 8 and w[8]) or (len(w) > 12 and not w[12]):
            continue
        for _s, _e, tb, te in lib.split_window(ids, e.timestamp_begin, e.eot, wf)[0]:
            text += e.transcript_lang(ids[tb:te], language) if language else e.transcript(ids[tb:te])
    return text


TEXT_FORMS = {
    "plain": dict(),
    "opts": dict(no_speech_threshold=0.6, logprob_threshold=-1.0),
    "fallback": dict(compression_ratio_threshold=0.0, temperatures=[0.0, 0.5, 1.0], seed=SEED),
    "prompted": dict(initial_prompt_ids=PROMPT, condition_on_previous_text=True),
    "lang": dict(languages=["en"]),
}


@pytest.mark.parametrize("form", list(TEXT_FORMS))
def test_text_pairs(setup, form):
    lib, e, files, wavs = setup
    opts = dict(TEXT_FORMS[form])
    texts = [e.run_long_text(pcm, **opts) for pcm in files]
    assert all(texts) and texts[0] != texts[1]
    assert [e.run_long_text(wav, **opts) for wav in wavs] == texts
    if form == "plain":
        return
    # the window-log call of the same form over both files; a file's noise follows its id, and a text form's one file has id 0
    if "initial_prompt_ids" in opts:
        opts["initial_prompt_ids"] = [PROMPT, PROMPT]
    if "languages" in opts:
        opts["languages"] = ["en", "en"]
    if "temperatures" in opts:
        opts["file_ids"] = [0, 0]
    logs = e.run_long_windows(files, **opts)
    if form == "lang":
        logs, codes = logs
        assert codes == ["en", "en"]
    assert len(logs[0]) >= 1 and len({w[0] for w in logs[1]}) >= 2
    assert [_joined(lib, e, log, "en" if form == "lang" else None) for log in logs] == texts


def test_chunked_text_pair(setup):
    lib, e, files, wavs = setup
    chunk = lib.ChunkOptions(W_MAX, W_MIN, 25, 1)
    texts = []
    for pcm, wav in zip(files, wavs):
        a, b = C.c_void_p(), C.c_void_p()
        e._check(e.L.AX_WHISPER_RunPCMLongChunked(e.h, pcm.ctypes.data_as(lib.fp), len(pcm), C.byref(chunk), None, C.byref(a)), "RunPCMLongChunked")
        e._check(e.L.AX_WHISPER_RunFileLongChunked(e.h, wav.encode(), C.byref(chunk), None, C.byref(b)), "RunFileLongChunked")
        texts.append(e._take(a.value))
        assert texts[-1] and e._take(b.value) == texts[-1]
    logs = e.run_long_chunked_windows(files, min_frames=W_MIN, max_frames=W_MAX)
    assert len(logs[0]) >= 2 and len(logs[1]) >= 2
    for log, text in zip(logs, texts):
        want = ""
        for seek, wf, _adv, ids, _p, _s in log:
            for _s0, _e0, tb, te in lib.chunked_segments(ids, e.timestamp_begin, e.eot, seek, wf):
                want += e.transcript(ids[tb:te])
        assert want == text


def test_lang_and_words_logs_are_one_call(setup):
    lib, e, files, wavs = setup
    opts = dict(max_new=8, languages=["en", None], tasks=["transcribe", "translate"], initial_prompt_ids=[PROMPT, None],
                compression_ratio_threshold=0.0, temperatures=[0.0, 1.0], seed=SEED, file_ids=[5, 3])
    lang = e.run_long_windows(files, **opts)
    words = e.run_long_windows(files, word_timestamps=False, **opts)
    assert lang == words
    assert lang[1] == ["en", "zh"] and len(lang[0][0]) >= 1 and len(lang[0][1]) >= 2
