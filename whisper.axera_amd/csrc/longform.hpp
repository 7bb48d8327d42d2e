// longform.hpp — long-form transcription, host side (no HIP types): the window rule and the log entry of one decoded window.
//
// Whisper's answer to audio longer than its 30 s window is a loop (openai-whisper transcribe(), here without its temperature /
// no-speech / prompt parts): decode the window at `seek` in timestamp mode, cut it at the last complete segment, move the
// window's start there. split_window is the cut: one window's ids -> segments + the frames to advance by (DESIGN.md
// "Long-form"). The single-clip split (AX_WHISPER_SplitSegments) keeps a trailing piece and is a different contract.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace axw {

struct WindowSegment {
  float start, end;        // seconds, relative to the window
  int tok_begin, tok_end;  // text ids of the segment: ids[tok_begin .. tok_end)
};

// ids: one window's ids (eot excluded), T = timestamp_begin, E = eot, window_frames = frames (10 ms) of audio in the window.
// Returns the frames the window start moves by (1 .. window_frames for window_frames >= 1).
//   pairs of consecutive timestamps ("cuts") close segments; ids after the last one belong to no segment and advance stops
//   at the last closed pair (that audio is decoded again), unless the ids end in a single timestamp (then the window is used up);
//   without cuts: one segment over the whole window.
//   Progress guard (not in openai-whisper, where a pair closing at 0.00 s loops for ever): advance <= 0 becomes window_frames.
inline int split_window(const int32_t* ids, int n, int T, int E, int window_frames, std::vector<WindowSegment>& segs) {
  segs.clear();
  auto ts = [&](int i) { return ids[i] >= T; };
  auto time = [&](int i) { return (float)((double)(ids[i] - T) * 0.02); };  // the double product, rounded once
  auto emit = [&](int lo, int hi, float t0, float t1) {
    int tb = -1, te = -1;
    for (int i = lo; i < hi; ++i)
      if (ids[i] < E) { if (tb < 0) tb = i; te = i + 1; }
    if (tb >= 0) segs.push_back({t0, t1, tb, te});  // a segment without text is not emitted
  };
  std::vector<int> bounds;
  for (int i = 1; i < n; ++i)
    if (ts(i - 1) && ts(i)) bounds.push_back(i);
  long advance;
  if (!bounds.empty()) {
    const bool single_end = n >= 2 && ts(n - 1) && !ts(n - 2);
    if (single_end) bounds.push_back(n);
    int lo = 0;
    for (int hi : bounds) {
      emit(lo, hi, time(lo), time(hi - 1));
      lo = hi;
    }
    advance = single_end ? window_frames : 2L * (ids[bounds.back() - 1] - T);
  } else {
    int last = -1;
    for (int i = 0; i < n; ++i)
      if (ts(i)) last = i;
    emit(0, n, 0.f, (last >= 0 && ids[last] != T) ? time(last) : (float)((double)window_frames * 0.01));
    advance = window_frames;
  }
  if (advance <= 0 || advance > window_frames) advance = window_frames;
  return (int)advance;
}

// The silent-window rule of the seek loop (DESIGN.md "Confidence"; openai-whisper transcribe(): should_skip). no_speech_logprob:
// log p(<|nospeech|>) at the step that fed sot; avg_logprob: the window's average token log-probability. A window is skipped iff
// the no-speech PROBABILITY exceeds its threshold and the average log-probability does not exceed its own: logprob_threshold
// = +inf skips on no-speech alone, a NaN no_speech_threshold never skips. All in float32, both comparisons strict.
inline bool long_window_is_silent(float no_speech_logprob, float avg_logprob, float no_speech_threshold, float logprob_threshold) {
  return std::exp(no_speech_logprob) > no_speech_threshold && !(avg_logprob > logprob_threshold);
}

// scored long-form: thresholds of the silent-window rule (NaN no_speech_threshold: the rule is off, scores are still fetched)
struct LongScoreOptions {
  float no_speech_threshold, logprob_threshold;
};

// one decoded window of AX_WHISPER_RunPCMLongWindows, in execution order
struct LongWindow {
  int file, seek, window_frames, advance, pass, slot;
  std::vector<int32_t> ids;  // all of them, also those after the last boundary
  // scored calls only: the window's two numbers and whether the silent-window rule dropped it (then advance == window_frames)
  float no_speech_logprob = 0.f, avg_logprob = 0.f;
  bool skipped = false;
};

}  // namespace axw
