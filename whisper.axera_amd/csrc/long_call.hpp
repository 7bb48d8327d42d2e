// long_call.hpp — what one seek-loop export of the C ABI asks for, and its one way to axw::LongScoreOptions (host side, no HIP types).
//
// Every AX_WHISPER_Run{PCM,File}Long* export of the seek loop fills a LongCall from its own (legacy) arguments with one of the
// adapters below and hands it to one of the three bodies of api.cpp (window log, text, segments and words); long_run_options is the
// only place where those arguments are checked and become the engine's options. Engine::run_long_windows chooses the decode mode and
// the prefill route by predicates on what it gets, so every export must reach it exactly as this table says:
//
//   exports                                          opts   temperatures accepted   file_lang_out (so per_file_language())
//   RunPCMLongWindows, RunPCMLong, RunFileLong       null   -                       -
//   ...WindowsScored, ...LongOpts                    set    none (empty list)       null
//   ...WindowsFallback, ...LongFallback              set    1 .. 16, else -1        null
//   ...WindowsPrompted, ...LongPrompted              set    0 .. 16                 null
//   ...WindowsLang, ...LongLang,                     set    0 .. 16                 always set (the caller's or a scratch array),
//   ...WindowsWords, ...LongWords                                                   also with lang and task NULL
//
// (PCM and file forms alike; word_timestamps comes from the *Words exports only, and RunPCMLongWords forces it on.)
// Refused (false, the export answers -1): a temperature count outside the row's range or a count > 0 with a NULL list; a file id below
// 0 or >= 2^27; n_initial[f] below 0 or above prompt_stride, or > 0 with NULL ids; a negative prompt_stride with n_initial given;
// n_files < 1; a NULL AX_WHISPER_LONG_OPTIONS where the export takes one.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ax_whisper_api.h"
#include "longform.hpp"

namespace axw {

struct LongCall {
  AX_WHISPER_LONG_OPTIONS o{};
  bool scored = false;       // false: the engine gets no options at all (the unscored decode mode)
  bool lang_always = false;  // the language result is collected whatever lang / task are
  int min_temperatures = 0;  // the fewest temperatures the call accepts (at most 16 always)
  bool bad = false;          // the export was handed no AX_WHISPER_LONG_OPTIONS
};

// ---- the legacy argument lists (the one-file forms pass the addresses of their own n_initial / lang / task, stride n_initial)
inline LongCall long_call_plain() { return LongCall{}; }

inline LongCall long_call_scored(float no_speech_threshold, float logprob_threshold) {
  LongCall c;
  c.scored = true;
  c.o.no_speech_threshold = no_speech_threshold; c.o.logprob_threshold = logprob_threshold; c.o.compression_ratio_threshold = NAN;
  return c;
}

inline LongCall long_call_fallback(float no_speech_threshold, float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                   int n_temperatures, uint64_t seed, const int* file_ids) {
  LongCall c = long_call_scored(no_speech_threshold, logprob_threshold);
  c.min_temperatures = 1;
  c.o.compression_ratio_threshold = compression_ratio_threshold;
  c.o.temperatures = temperatures; c.o.n_temperatures = n_temperatures; c.o.seed = seed; c.o.file_ids = file_ids;
  return c;
}

inline LongCall long_call_prompted(float no_speech_threshold, float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                   int n_temperatures, uint64_t seed, const int* file_ids, const int32_t* initial_prompt_ids, int prompt_stride,
                                   const int* n_initial, int condition_on_previous_text) {
  LongCall c = long_call_fallback(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, n_temperatures, seed, file_ids);
  c.min_temperatures = 0;
  c.o.initial_prompt_ids = initial_prompt_ids; c.o.prompt_stride = prompt_stride; c.o.n_initial = n_initial;
  c.o.condition_on_previous_text = condition_on_previous_text;
  return c;
}

inline LongCall long_call_lang(LongCall prompted, const int* lang, const int* task) {
  prompted.lang_always = true;
  prompted.o.lang = lang; prompted.o.task = task;
  return prompted;
}

// the *Words exports: the caller's struct as it is; words_always (RunPCMLongWords): word_timestamps is taken as 1
inline LongCall long_call_options(const AX_WHISPER_LONG_OPTIONS* o, bool words_always) {
  LongCall c;
  c.scored = c.lang_always = true;
  if (o) c.o = *o;
  else c.bad = true;
  if (words_always) c.o.word_timestamps = 1;
  return c;
}

// ---- the NULL and size checks of the window-log forms
inline bool long_files_ok(const float* const* pcm, const int* num_samples, int n_files) {
  if (!pcm || !num_samples || n_files < 1) return false;
  for (int b = 0; b < n_files; ++b)
    if (!pcm[b] || num_samples[b] < 1) return false;
  return true;
}

// where a window log goes: win_cap rows of each array; NULL: the export has no such output
struct WindowLogOut {
  int win_cap;
  int* win_info;
  int32_t* ids;
  float* win_score;
  int* win_prompt;
  int* n_windows;
  int* lang_out;
  AX_WHISPER_LONG_WORD_LOG* words;
};
inline bool window_log_ok(const WindowLogOut& out, bool scored) {
  return out.win_cap >= 0 && out.n_windows && (out.win_cap == 0 || (out.win_info && out.ids && (!scored || out.win_score)));
}
// the word log of a call with word_timestamps on
inline bool word_log_ok(const AX_WHISPER_LONG_WORD_LOG* w, int win_cap) {
  if (!w || w->seg_cap < 0 || w->word_cap < 0) return false;
  if (win_cap > 0 && (!w->win_words || !w->text_ids || !w->jump || !w->token_logprob)) return false;
  if (w->seg_cap > 0 && (!w->seg_tokens || !w->seg_start || !w->seg_end)) return false;
  return w->word_cap <= 0 || (w->word_segment && w->word_text_end && w->word_start && w->word_end && w->word_prob);
}

// what the engine is handed for one call; the language result lands in lang[] unless the caller gave an array of its own
struct LongRun {
  LongScoreOptions opts{};
  bool scored = false;
  std::vector<int> lang;  // [n_files], -1 until the loop has run; used when lang_out is NULL
  const LongScoreOptions* get() const { return scored ? &opts : nullptr; }
};

// rows of initial_prompt_ids [n_files][prompt_stride], n_initial[f] ids of row f -> one list per file; false: refused
inline bool long_initial_prompts(const AX_WHISPER_LONG_OPTIONS& o, int n_files, std::vector<std::vector<int32_t>>& prompts) {
  if (o.prompt_stride < 0) return false;
  prompts.resize((size_t)n_files);
  for (int f = 0; f < n_files; ++f) {
    if (o.n_initial[f] < 0 || o.n_initial[f] > o.prompt_stride || (o.n_initial[f] > 0 && !o.initial_prompt_ids)) return false;
    if (o.n_initial[f] == 0) continue;
    const int32_t* p = o.initial_prompt_ids + (size_t)f * o.prompt_stride;
    prompts[(size_t)f].assign(p, p + o.n_initial[f]);
  }
  return true;
}

// false: the call is refused (the list above)
inline bool long_run_options(const LongCall& c, int n_files, int* lang_out, LongRun& run) {
  const AX_WHISPER_LONG_OPTIONS& o = c.o;
  run.scored = c.scored;
  if (!c.scored) return true;
  if (c.bad || n_files < 1) return false;
  if (o.n_temperatures < c.min_temperatures || o.n_temperatures > 16 || (o.n_temperatures > 0 && !o.temperatures)) return false;
  LongScoreOptions& opts = run.opts;
  opts.no_speech_threshold = o.no_speech_threshold; opts.logprob_threshold = o.logprob_threshold;
  opts.compression_ratio_threshold = o.compression_ratio_threshold;
  if (o.n_temperatures > 0) opts.temperatures.assign(o.temperatures, o.temperatures + o.n_temperatures);
  opts.seed = o.seed;
  for (int f = 0; o.file_ids && f < n_files; ++f) {
    if (o.file_ids[f] < 0 || o.file_ids[f] >= (1 << 27)) return false;  // (id * 16 + attempt is the stream's high word)
    opts.file_ids.push_back(o.file_ids[f]);
  }
  opts.condition_on_previous_text = o.condition_on_previous_text != 0;
  if (o.n_initial && !long_initial_prompts(o, n_files, opts.initial_prompt_ids)) return false;
  if (o.lang) opts.file_lang.assign(o.lang, o.lang + n_files);
  if (o.task) opts.file_task.assign(o.task, o.task + n_files);
  if (c.lang_always) {
    run.lang.assign((size_t)n_files, -1);
    opts.file_lang_out = lang_out ? lang_out : run.lang.data();
  }
  opts.word_timestamps = o.word_timestamps != 0;
  return true;
}

}  // namespace axw
