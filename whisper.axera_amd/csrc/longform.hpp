// longform.hpp — long-form transcription, host side (no HIP types): the window rule and the log entry of one decoded window.
//
// Whisper's answer to audio longer than its 30 s window is a loop (openai-whisper transcribe(); its temperature, no-speech and
// prompt parts are the options further down): decode the window at `seek` in timestamp mode, cut it at the last complete segment, move the
// window's start there. split_window is the cut: one window's ids -> segments + the frames to advance by (DESIGN.md
// "Long-form"). The single-clip split (AX_WHISPER_SplitSegments) keeps a trailing piece and is a different contract.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <dlfcn.h>

#include "long_cuts.hpp"

namespace axw {

// Chunked long-form (DESIGN.md "Chunked long-form"; long_cuts.hpp: the definitions): the options of one call. Windows are decoded
// independently, so everything that feeds one window's result into the next one has no meaning here and is refused, as is what the
// mode does not cover yet; the members below the line only carry what was asked for to the one place that refuses it.
struct ChunkedOptions {
  CutParams cut;
  // the scored decode mode: every window carries its two numbers, long_window_is_silent under the thresholds drops a window's segments
  bool scored = false;
  float no_speech_threshold = NAN, logprob_threshold = NAN;
  // a language (>= 0, or -1: the handle's) and a task per file of the WHOLE call (empty: the handle's, transcribe)
  std::vector<int> file_lang, file_task;
  int file_base = 0;  // index of this engine's first file in the whole call
  // ---- refused
  int n_temperatures = 0;
  bool compression_ratio_threshold = false, initial_prompt = false, condition_on_previous_text = false, word_timestamps = false;
  int beam_size = 1;
};
// empty: the call can run; else the text of the refusal (n_files: files of the WHOLE call)
inline std::string chunked_options_error(const ChunkedOptions& o, int n_files) {
  const std::string bad = cut_params_error(o.cut.w_min, o.cut.w_max, o.cut.smooth);
  if (!bad.empty()) return bad;
  for (const std::vector<int>* v : {&o.file_lang, &o.file_task})
    if (!v->empty() && (long)v->size() < (long)n_files) return "chunked long-form: fewer languages or tasks than files";
  for (int l : o.file_lang)
    if (l == -2) return "chunked long-form: language detection (-2) is not covered: detect the language first (AX_WHISPER_DetectLanguage)";
  if (o.n_temperatures > 0 || o.compression_ratio_threshold)
    return "chunked long-form: temperatures and temperature fallback are not covered (windows are decoded once, greedily)";
  if (o.initial_prompt || o.condition_on_previous_text)
    return "chunked long-form: prompts and condition_on_previous_text are not covered (windows are decoded independently)";
  if (o.word_timestamps) return "chunked long-form: word timestamps are not covered";
  if (o.beam_size != 1) return "chunked long-form: beam search is not covered (beam_size must be 1)";
  return std::string();
}

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
// ranges (optional): for every emitted segment the ids it spans, [lo, hi) from its opening timestamp to its closing one — what the
// previous-text carry appends (carry_prompt below).
inline int split_window(const int32_t* ids, int n, int T, int E, int window_frames, std::vector<WindowSegment>& segs,
                        std::vector<std::pair<int, int>>* ranges = nullptr) {
  segs.clear();
  if (ranges) ranges->clear();
  auto ts = [&](int i) { return ids[i] >= T; };
  auto time = [&](int i) { return (float)((double)(ids[i] - T) * 0.02); };  // the double product, rounded once
  auto emit = [&](int lo, int hi, float t0, float t1) {
    int tb = -1, te = -1;
    for (int i = lo; i < hi; ++i)
      if (ids[i] < E) { if (tb < 0) tb = i; te = i + 1; }
    if (tb >= 0) {  // a segment without text is not emitted
      segs.push_back({t0, t1, tb, te});
      if (ranges) ranges->push_back({lo, hi});
    }
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

// The seek rule under word timestamps (DESIGN.md "Word-level timestamps", long-form; openai-whisper transcribe() with
// word_timestamps=True). ids: the window's ids (eot excluded), seek: its start in frames of 10 ms, split_advance: what split_window
// gave; has_word / last_word_end: whether the window yielded a word and the end of its last one, seconds in FILE time.
// Unless the ids end in a single timestamp (last id >= T, the one before it < T): if the last word ends behind the window's start
// (last_word_end > seek / 100), the next window starts there, at round(last_word_end * 100) (to the nearest frame, ties to even, as
// Python's round). Progress guard, in the spirit of split_window's: an advance <= 0 or > window_frames keeps split_window's.
// Returns the advance; *by_word_end (optional): whether the word-end seek was taken.
inline int long_word_advance(const int32_t* ids, int n, int T, int seek, int window_frames, int split_advance, bool has_word, double last_word_end,
                             bool* by_word_end = nullptr) {
  if (by_word_end) *by_word_end = false;
  const bool single_end = n >= 2 && ids[n - 1] >= T && ids[n - 2] < T;
  if (single_end || !has_word || !(last_word_end > (double)seek / 100.0)) return split_advance;
  const double target = std::nearbyint(last_word_end * 100.0);
  const double advance = target - (double)seek;
  if (!(advance > 0) || advance > (double)window_frames) return split_advance;
  if (by_word_end) *by_word_end = true;
  return (int)advance;
}

// The silent-window rule of the seek loop (DESIGN.md "Confidence"; openai-whisper transcribe(): should_skip). no_speech_logprob:
// log p(<|nospeech|>) at the step that fed sot; avg_logprob: the window's average token log-probability. A window is skipped iff
// the no-speech PROBABILITY exceeds its threshold and the average log-probability does not exceed its own: logprob_threshold
// = +inf skips on no-speech alone, a NaN no_speech_threshold never skips. All in float32, both comparisons strict.
inline bool long_window_is_silent(float no_speech_logprob, float avg_logprob, float no_speech_threshold, float logprob_threshold) {
  return std::exp(no_speech_logprob) > no_speech_threshold && !(avg_logprob > logprob_threshold);
}

// Temperature fallback (DESIGN.md "Temperature fallback"; openai-whisper transcribe(): decode_with_fallback). A decoded window is
// decoded again at the next temperature iff its text compresses too well (a repetition loop) or its average log-probability is too
// low — unless it looks silent, which the silent-window rule then handles. A NaN threshold switches its part off. All in float32.
inline bool window_needs_fallback(float compression_ratio, float avg_logprob, float no_speech_logprob, float compression_ratio_threshold,
                                  float logprob_threshold, float no_speech_threshold) {
  bool need = false;
  if (compression_ratio > compression_ratio_threshold) need = true;
  if (avg_logprob < logprob_threshold) need = true;
  if (std::exp(no_speech_logprob) > no_speech_threshold && avg_logprob < logprob_threshold) need = false;  // silence
  return need;
}

// The text the compression ratio is taken of: the window's bytes without ASCII whitespace at both ends
inline std::string strip_ascii_space(const std::string& s) {
  auto sp = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; };
  size_t lo = 0, hi = s.size();
  while (lo < hi && sp(s[lo])) ++lo;
  while (hi > lo && sp(s[hi - 1])) --hi;
  return s.substr(lo, hi - lo);
}

// n / len(zlib.compress(bytes)) at zlib's default level, as openai-whisper's compression_ratio (n = 0: 0 / 8 = 0). zlib's runtime
// library is loaded at first use (libz.so.1: present wherever Python runs; its development symlink need not be); throws without it.
inline float compression_ratio(const unsigned char* bytes, size_t n) {
  typedef unsigned long (*bound_fn)(unsigned long);
  typedef int (*compress_fn)(unsigned char*, unsigned long*, const unsigned char*, unsigned long);
  struct Z { bound_fn bound = nullptr; compress_fn compress = nullptr; };
  static const Z z = [] {
    Z r;
    if (void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL)) {
      r.bound = reinterpret_cast<bound_fn>(dlsym(h, "compressBound"));
      r.compress = reinterpret_cast<compress_fn>(dlsym(h, "compress"));
    }
    return r;
  }();
  if (!z.bound || !z.compress) throw std::runtime_error("compression ratio: libz.so.1 (zlib's runtime library) could not be loaded");
  static const unsigned char none = 0;
  unsigned long len = z.bound((unsigned long)n);
  std::vector<unsigned char> out(len);
  if (z.compress(out.data(), &len, n ? bytes : &none, (unsigned long)n) != 0 || len == 0) throw std::runtime_error("compression ratio: zlib compress failed");
  return (float)((double)n / (double)len);
}

// Prompt conditioning across windows (DESIGN.md "Prompt conditioning"; openai-whisper transcribe(): all_tokens / prompt_reset_since),
// per file. A window's prompt is all_ids[reset_since:], of which the decoder takes the last n_text_ctx / 2 - 1.
struct PromptCarry {
  std::vector<int32_t> all_ids;  // starts as the file's initial prompt ids
  int reset_since = 0;
};
// One step of the carry rule, after a KEPT window (ids: all of them, eot excluded): unless the window was skipped as silent, append
// the ids of its emitted segments, timestamps included (ids after the last closed pair are dropped as split_window drops them;
// segments without text add nothing); then, if conditioning is off or the kept attempt's temperature is above 0.5, the next prompt
// starts behind everything so far.
inline void carry_prompt(PromptCarry& st, const int32_t* ids, int n, int T, int E, int window_frames, bool skipped, bool condition_on_previous_text,
                         float temperature) {
  if (!skipped) {
    std::vector<WindowSegment> segs;
    std::vector<std::pair<int, int>> ranges;
    split_window(ids, n, T, E, window_frames, segs, &ranges);
    for (const auto& r : ranges) st.all_ids.insert(st.all_ids.end(), ids + r.first, ids + r.second);
  }
  if (!condition_on_previous_text || temperature > 0.5f) st.reset_since = (int)st.all_ids.size();
}

// scored long-form: thresholds of the silent-window rule (NaN no_speech_threshold: the rule is off, scores are still fetched)
// With `temperatures` non-empty the call is the fallback loop: sampled decode mode throughout, attempt a of a window at
// temperatures[a] (at most 16 attempts), a window that needs fallback is decoded again in the next pass. (openai-whisper's list
// 0, 0.2, .. 1.0 is the default of the CLI and of the Python mirror: an empty list here keeps every existing call what it was.)
struct LongScoreOptions {
  float no_speech_threshold, logprob_threshold;
  float compression_ratio_threshold = NAN;
  std::vector<float> temperatures;
  uint64_t seed = 0;
  int file_base = 0;  // index of this engine's first file in the whole call (set per engine when the files are sharded)
  // The random stream of a window is (seek, file id * 16 + attempt). file_ids (empty, or one id >= 0 per file of the WHOLE call): the
  // caller's names for its files, so that a file draws the same noise whatever its position in the call; empty: the file's index
  // in the whole call.
  std::vector<int> file_ids;
  int file_id(int local_file) const { return file_ids.empty() ? file_base + local_file : file_ids[(size_t)(file_base + local_file)]; }
  // Prompt conditioning (DESIGN.md "Prompt conditioning"): initial_prompt_ids (empty, or one list per file of the WHOLE call) start each
  // file's carried text; condition_on_previous_text: every window is prompted with the text kept before it. Both off: the loop as it was.
  std::vector<std::vector<int32_t>> initial_prompt_ids;
  bool condition_on_previous_text = false;
  bool prompted() const {
    if (condition_on_previous_text) return true;
    for (const auto& p : initial_prompt_ids)
      if (!p.empty()) return true;
    return false;
  }
  // Language and task per file (DESIGN.md "Language and task per clip"): file_lang / file_task (empty, or one entry per file of the
  // WHOLE call): >= 0 a language index, -1 the handle's language, -2 detect it on the file's window at seek 0 (openai-whisper detects
  // once on the first 30 s, also when that window is then skipped as silent; every later window uses the result); task 0
  // transcribe, 1 translate. file_lang_out (or null): [files of the WHOLE call], the index every file was decoded under. All empty /
  // null: the loop as it was.
  std::vector<int> file_lang, file_task;
  int* file_lang_out = nullptr;
  bool per_file_language() const { return !file_lang.empty() || !file_task.empty() || file_lang_out; }
  // Word timestamps (DESIGN.md "Word-level timestamps", long-form): after the decisions of a pass every kept, non-skipped window is
  // aligned (one align_tokens call per pass), the word rule runs in file time with the file's last_speech_timestamp, and
  // long_word_advance may move the seek to the last word's end. word_logprob_route: the route of the token probabilities
  // (0 rows, 1 fused). Off: the loop as it was.
  bool word_timestamps = false;
  int word_logprob_route = 1;
};

struct LongWord {
  int segment;          // index among the window's segments
  std::string text;     // the word's bytes
  double start, end;    // seconds in file time
  float probability;
};

// one decoded window of AX_WHISPER_RunPCMLongWindows, in execution order
struct LongWindow {
  int file, seek, window_frames, advance, pass, slot;
  std::vector<int32_t> ids;  // all of them, also those after the last boundary
  // scored calls only: the window's two numbers and whether the silent-window rule dropped it (then advance == window_frames)
  float no_speech_logprob = 0.f, avg_logprob = 0.f;
  bool skipped = false;
  // fallback calls only: every attempt is an entry. kept: this attempt's result stands (the others advance by 0 and emit nothing)
  int attempt = 0;
  float temperature = 0.f, compression_ratio = 0.f;
  bool kept = true;
  int n_prompt = 0;  // prompted calls only: ids the window was conditioned on (after the truncation to n_text_ctx / 2 - 1)
  // word-timestamp calls only, on kept windows that were not skipped (else empty): the text ids that were aligned (those below eot
  // of split_window's segments, seg_tokens[s] of them in segment s), the alignment's raw jump [n + 1] and token_logprob [n], the
  // segment starts and ends the word rule left and the words, both in file time, and which advance was taken
  std::vector<int32_t> text_ids;
  std::vector<int> seg_tokens, jump;
  std::vector<float> word_logprob;
  std::vector<double> seg_start, seg_end;
  std::vector<LongWord> words;
  bool by_word_end = false;  // advance is long_word_advance's word-end seek, not split_window's
};

}  // namespace axw
