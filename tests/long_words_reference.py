"""The host rules of long-form word timestamps in Python (openai-whisper transcribe(word_timestamps=True)), on top of
tests/word_reference.py and tests/longform_reference.py: the word rule of a window that starts time_offset seconds into its file, the
seek rule, and the replay of a whole window log.

words_from_alignment_at is word_reference.words_from_alignment with one change, as add_word_timestamps has it inside transcribe():
a word's times are round(time_offset + jump / 50, 2), so the segment times it is compared with, last_speech_timestamp and the
max(0, .) clamps are all in FILE time; the word durations (median, sentence-end cut) are taken before the offset is added."""
import numpy as np

import word_reference as wr


def words_from_alignment_at(table, ids, eot, language, seg_tokens, seg_start, seg_end, jump, token_logprob, last_speech_timestamp=0.0,
                            time_offset=0.0):
    """-> ([(segment, word bytes, start, end, probability)], seg_start, seg_end after the rule), everything in file time"""
    seg_start, seg_end = [float(x) for x in seg_start], [float(x) for x in seg_end]
    if len(seg_tokens) == 0:
        return [], seg_start, seg_end
    ids = [int(t) for t in ids]
    al = []
    if ids:
        words = wr.split_words(table, ids + [eot], eot, language)
        if words and words[-1][1][0] == eot:
            words = words[:-1]
        b = 0
        for wb, toks in words:
            e = b + len(toks)
            probs = np.exp(np.asarray(token_logprob[b:e], dtype=np.float32).astype(np.float64))
            al.append(dict(word=wb.decode("utf-8"), tokens=toks, start=int(jump[b]) / 50.0, end=int(jump[e]) / 50.0, probability=float(np.mean(probs))))
            b = e
    dur = np.array([t["end"] - t["start"] for t in al])
    dur = dur[dur.nonzero()]
    median = min(0.7, float(np.median(dur)) if len(dur) else 0.0)
    max_duration = median * 2
    if len(dur):
        for i in range(1, len(al)):
            if al[i]["end"] - al[i]["start"] > max_duration:
                if wr._one(al[i]["word"], wr.SENTENCE_END):
                    al[i]["end"] = al[i]["start"] + max_duration
                elif wr._one(al[i - 1]["word"], wr.SENTENCE_END):
                    al[i]["start"] = al[i]["end"] - max_duration
    wr.merge_punctuations(al)
    out, wi = [], 0
    for s, n_tok in enumerate(seg_tokens):
        saved, words = 0, []
        while wi < len(al) and saved < n_tok:
            t = al[wi]
            if t["word"]:
                words.append(dict(word=t["word"], start=round(time_offset + t["start"], 2), end=round(time_offset + t["end"], 2),
                                  probability=t["probability"]))
            saved += len(t["tokens"])
            wi += 1
        if words:
            if words[0]["end"] - last_speech_timestamp > median * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            if seg_start[s] < words[0]["end"] and seg_start[s] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median, seg_start[s]))
            else:
                seg_start[s] = words[0]["start"]
            if seg_end[s] > words[-1]["start"] and seg_end[s] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median, seg_end[s])
            else:
                seg_end[s] = words[-1]["end"]
            last_speech_timestamp = seg_end[s]
        out += [(s, w["word"].encode("utf-8"), float(w["start"]), float(w["end"]), w["probability"]) for w in words]
    return out, seg_start, seg_end


def long_word_advance(ids, T, seek, window_frames, split_advance, last_word_end):
    """The seek rule -> (advance, whether the word end was taken). last_word_end: file time, None without a word. Unless the ids end
    in a single timestamp: a last word that ends behind the window's start moves the seek to round(end * 100); an advance <= 0 or
    beyond the window keeps split_window's."""
    ids = [int(t) for t in ids]
    single_end = len(ids) >= 2 and ids[-1] >= T and ids[-2] < T
    if single_end or last_word_end is None or not last_word_end > seek / 100:
        return split_advance, False
    advance = round(last_word_end * 100) - seek  # (Python's round: to the nearest frame, ties to even)
    if advance <= 0 or advance > window_frames:
        return split_advance, False
    return advance, True


def split_window(ids, T, E, window_frames):
    """tests/longform_reference.py's window rule -> ([(start, end, tok_begin, tok_end)], advance)"""
    import longform_reference as lr

    segs, advance, _ = lr.split_window(ids, T, E, window_frames)
    return segs, advance


def replay_window(table, language, T, E, n_text_ctx, seek, window_frames, ids, jump, token_logprob, last_speech_timestamp):
    """One kept, non-skipped window from what the log holds -> dict(text_ids, seg_tokens, seg_start, seg_end, words, advance,
    by_word_end, last_speech_timestamp): the segments of split_window, their ids below eot (at most n_text_ctx - 5 in all), the word
    rule in file time, the seek rule."""
    segs, split_advance = split_window(ids, T, E, window_frames)
    offset = seek / 100
    text_ids, seg_tokens, ss, se = [], [], [], []
    for s, e, tb, te in segs:
        count = 0
        for t in ids[tb:te]:
            if t < E and len(text_ids) + 5 < n_text_ctx:
                text_ids.append(int(t))
                count += 1
        seg_tokens.append(count)
        ss.append(offset + float(np.float32(s)))
        se.append(offset + float(np.float32(e)))
    words = []
    if window_frames >= 2 and text_ids:
        words, ss, se = words_from_alignment_at(table, text_ids, E, language, seg_tokens, ss, se, jump, token_logprob, last_speech_timestamp, offset)
    else:
        text_ids, seg_tokens = [], [0] * len(seg_tokens)
    last_end = words[-1][3] if words else None
    advance, by = long_word_advance(ids, T, seek, window_frames, split_advance, last_end)
    return dict(text_ids=text_ids, seg_tokens=seg_tokens, seg_start=ss, seg_end=se, words=words, advance=advance, by_word_end=by,
                last_speech_timestamp=last_end if words else last_speech_timestamp)


# ---------------------------------------------------------------------------------------------- the DTW path a jump list stands for
def dtw_cost(x, allowed=None):
    """float64: the cost of the cheapest DTW path over x [N][F] (openai-whisper's dtw: from (0, 0) to (N - 1, F - 1), steps right,
    down and diagonal, the cost of a path the sum of its cells), over the cells where `allowed` is true (None: all); inf: no path"""
    x = np.asarray(x, dtype=np.float64)
    N, F = x.shape
    if allowed is not None:
        x = np.where(allowed, x, np.inf)
    prev = np.full(F + 1, np.inf)
    prev[0] = 0.0
    for i in range(N):
        cur = np.full(F + 1, np.inf)
        best = np.minimum(prev[:-1], prev[1:])  # diagonal and down
        xi = x[i]
        c = np.inf
        for j in range(F):
            c = xi[j] + min(best[j], c)
            cur[j + 1] = c
        prev = cur
    return float(prev[F])


def jump_path_excess(matrix_rows, jump):
    """How much dearer than the optimum the cheapest path that begins every row at jump[i] is, on -matrix_rows [N][F] in float64
    -> (excess >= 0, path cells N + F). A path with these jumps visits row i exactly on frames [jump[i], jump[i + 1]] (the last
    row up to F - 1), so the constraint is a mask. An engine whose matrix is within eps of this one everywhere and whose path is
    optimal on its own matrix gives an excess of at most 2 (N + F) eps: the path's cost moves by at most (N + F) eps between the
    two matrices, and so does the optimum's."""
    x = -np.asarray(matrix_rows, dtype=np.float64)
    N, F = x.shape
    jump = [int(j) for j in jump]
    assert len(jump) == N
    f = np.arange(F)[None, :]
    lo = np.asarray(jump)[:, None]
    hi = np.asarray(jump[1:] + [F - 1])[:, None]
    return dtw_cost(x, (f >= lo) & (f <= hi)) - dtw_cost(x), N + F
