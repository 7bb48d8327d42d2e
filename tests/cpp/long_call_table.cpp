// long_call_table.cpp — the table of whisper.axera_amd/csrc/long_call.hpp, asserted: legacy arguments of every kind of seek-loop
// export go through the adapters and long_run_options, and what the engine would be handed is compared with expectations written
// out here (the engine chooses its decode mode and prefill route by these predicates). Plain g++, no GPU, no library.
// Arguments: 2 files; prompts of 0 and 3 ids at stride 3; 0 / 1 / 16 / 17 temperatures; file ids 0 and 2^27.
#include <cstdio>
#include <cstring>

#include "long_call.hpp"

using axw::LongCall;
using axw::LongRun;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, what, #cond); ++failures; } \
  } while (0)

static const float kTemps[17] = {0.f, .06f, .12f, .18f, .24f, .3f, .36f, .42f, .48f, .54f, .6f, .66f, .72f, .78f, .84f, .9f, .96f};
static const int32_t kPrompt[6] = {1, 2, 3, 4, 5, 6};  // stride 3: file 0's row is unused (0 ids), file 1's is 4 5 6
static const int kInitial[2] = {0, 3};
static const int kIdsGood[2] = {0, (1 << 27) - 1}, kIdsBig[2] = {0, 1 << 27}, kIdsNeg[2] = {-1, 0};

static void refused(const char* what, const LongCall& c, int n_files = 2) {
  LongRun run;
  int lang_out[2] = {77, 77};
  CHECK(!axw::long_run_options(c, n_files, lang_out, run));
  CHECK(lang_out[0] == 77 && lang_out[1] == 77);
}

// what an accepted call must look like to the engine
struct Expect {
  bool null_opts;
  size_t n_temperatures;
  bool prompted, per_file_language, word_timestamps;
  int file_id1;  // opts.file_id(1)
};
static LongRun accepted(const char* what, const LongCall& c, const Expect& e, int* lang_out = nullptr, int n_files = 2) {
  LongRun run;
  CHECK(axw::long_run_options(c, n_files, lang_out, run));
  CHECK((run.get() == nullptr) == e.null_opts);
  if (run.get()) {
    const axw::LongScoreOptions& o = *run.get();
    CHECK(o.temperatures.size() == e.n_temperatures);
    CHECK(o.prompted() == e.prompted);
    CHECK(o.per_file_language() == e.per_file_language);
    CHECK(o.word_timestamps == e.word_timestamps);
    if (n_files > 1) CHECK(o.file_id(1) == e.file_id1);
    CHECK(o.file_base == 0);
    if (e.per_file_language) {
      CHECK(o.file_lang_out == (lang_out ? lang_out : run.lang.data()));
      CHECK((int)run.lang.size() == n_files && run.lang[0] == -1);
    } else {
      CHECK(o.file_lang_out == nullptr);
    }
  }
  return run;
}

// the prompted argument list shared by the Prompted, Lang and Words rows
static LongCall prompted(int n_temperatures, const int* file_ids = nullptr, const int32_t* ids = kPrompt, int stride = 3,
                         const int* n_initial = kInitial, int condition = 0, const float* temps = kTemps) {
  return axw::long_call_prompted(0.6f, -1.f, 2.4f, n_temperatures ? temps : nullptr, n_temperatures, 11, file_ids, ids, stride, n_initial, condition);
}
static AX_WHISPER_LONG_OPTIONS options_struct(int n_temperatures, int word_timestamps) {
  AX_WHISPER_LONG_OPTIONS o = prompted(n_temperatures).o;
  o.word_timestamps = word_timestamps;
  return o;
}

// the refusals that the Prompted, Lang and Words rows share; wrap: the row's adapter over a prompted argument list
template <typename Wrap>
static void prompted_refusals(const char* what, Wrap wrap) {
  static const int over[2] = {0, 4}, neg[2] = {-1, 0};
  refused(what, wrap(prompted(17)));
  refused(what, wrap(prompted(-1)));
  refused(what, wrap(prompted(1, nullptr, kPrompt, 3, kInitial, 0, nullptr)));  // a count without a list
  refused(what, wrap(prompted(0, kIdsBig)));
  refused(what, wrap(prompted(0, kIdsNeg)));
  refused(what, wrap(prompted(0, nullptr, kPrompt, 3, over)));      // n_initial above the stride
  refused(what, wrap(prompted(0, nullptr, kPrompt, 3, neg)));       // n_initial below 0
  refused(what, wrap(prompted(0, nullptr, nullptr, 3, kInitial)));  // ids NULL with a non-zero count
  refused(what, wrap(prompted(0, nullptr, kPrompt, -1, kInitial)));
  refused(what, wrap(prompted(0)), 0);  // no files
  int n1 = -1;  // the one-file forms pass their own count as stride and list
  refused(what, wrap(axw::long_call_prompted(0.6f, -1.f, 2.4f, nullptr, 0, 11, nullptr, kPrompt, n1, &n1, 0)), 1);
}

int main() {
  const char* what;

  what = "plain";  // RunPCMLongWindows, RunPCMLong, RunFileLong
  accepted(what, axw::long_call_plain(), {true, 0, false, false, false, 1});

  what = "scored";  // ...WindowsScored, ...LongOpts
  {
    const LongRun r = accepted(what, axw::long_call_scored(0.6f, -1.f), {false, 0, false, false, false, 1});
    CHECK(r.opts.no_speech_threshold == 0.6f && r.opts.logprob_threshold == -1.f && std::isnan(r.opts.compression_ratio_threshold));
    CHECK(r.opts.seed == 0 && r.opts.file_ids.empty() && r.opts.initial_prompt_ids.empty());
  }

  what = "fallback";  // ...WindowsFallback, ...LongFallback: 1 .. 16 temperatures
  refused(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, kTemps, 0, 11, nullptr));
  refused(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, kTemps, 17, 11, nullptr));
  refused(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, nullptr, 1, 11, nullptr));
  refused(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, nullptr, 0, 11, nullptr));
  refused(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, kTemps, 1, 11, kIdsBig));
  refused(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, kTemps, 1, 11, kIdsNeg));
  accepted(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, kTemps, 1, 11, nullptr), {false, 1, false, false, false, 1});
  {
    const LongRun r = accepted(what, axw::long_call_fallback(0.6f, -1.f, 2.4f, kTemps, 16, 11, kIdsGood), {false, 16, false, false, false, (1 << 27) - 1});
    CHECK(r.opts.temperatures[15] == .9f && r.opts.seed == 11 && r.opts.compression_ratio_threshold == 2.4f);
    CHECK(r.opts.file_id(0) == 0);
  }

  what = "prompted";  // ...WindowsPrompted, ...LongPrompted: 0 .. 16 temperatures, file_lang_out null
  prompted_refusals(what, [](const LongCall& c) { return c; });
  for (int n : {0, 1, 16}) accepted(what, prompted(n), {false, (size_t)n, true, false, false, 1});
  accepted(what, prompted(0, kIdsGood), {false, 0, true, false, false, (1 << 27) - 1});
  {
    const LongRun r = accepted(what, prompted(0), {false, 0, true, false, false, 1});
    CHECK(r.opts.initial_prompt_ids.size() == 2 && r.opts.initial_prompt_ids[0].empty());
    CHECK(r.opts.initial_prompt_ids[1] == (std::vector<int32_t>{4, 5, 6}));
    CHECK(!r.opts.condition_on_previous_text);
  }
  {
    static const int none[2] = {0, 0};
    accepted(what, prompted(0, nullptr, nullptr, 0, nullptr, 0), {false, 0, false, false, false, 1});  // no prompts, no carry
    accepted(what, prompted(0, nullptr, nullptr, 0, none, 0), {false, 0, false, false, false, 1});     // empty prompts are no prompts
    accepted(what, prompted(0, nullptr, nullptr, 0, nullptr, 1), {false, 0, true, false, false, 1});   // the carry alone
    int n1 = 3;  // a one-file form
    const LongRun r = accepted(what, axw::long_call_prompted(0.6f, -1.f, 2.4f, nullptr, 0, 11, nullptr, kPrompt, n1, &n1, 0),
                               {false, 0, true, false, false, 0}, nullptr, 1);
    CHECK(r.opts.initial_prompt_ids[0] == (std::vector<int32_t>{1, 2, 3}));
  }

  what = "lang";  // ...WindowsLang, ...LongLang: as prompted, the language result always collected
  {
    static const int lang[2] = {-2, 3}, task[2] = {0, 1};
    prompted_refusals(what, [](const LongCall& c) { return axw::long_call_lang(c, lang, task); });
    int lang_out[2] = {9, 9};
    for (int n : {0, 1, 16}) accepted(what, axw::long_call_lang(prompted(n), lang, task), {false, (size_t)n, true, true, false, 1}, lang_out);
    const LongRun r = accepted(what, axw::long_call_lang(prompted(0, kIdsGood), lang, task), {false, 0, true, true, false, (1 << 27) - 1});
    CHECK(r.opts.file_lang == (std::vector<int>{-2, 3}) && r.opts.file_task == (std::vector<int>{0, 1}));
    // lang and task NULL, no prompts: still the per-file-language route
    const LongRun q = accepted(what, axw::long_call_lang(prompted(0, nullptr, nullptr, 0, nullptr, 0), nullptr, nullptr), {false, 0, false, true, false, 1});
    CHECK(q.opts.file_lang.empty() && q.opts.file_task.empty());
    int n1 = 0, l1 = 5, t1 = 1;  // a one-file form
    const LongRun s = accepted(what, axw::long_call_lang(axw::long_call_prompted(0.6f, -1.f, NAN, nullptr, 0, 0, nullptr, nullptr, n1, &n1, 0), &l1, &t1),
                               {false, 0, false, true, false, 0}, nullptr, 1);
    CHECK(s.opts.file_lang == std::vector<int>{5} && s.opts.file_task == std::vector<int>{1});
  }

  what = "words";  // ...WindowsWords, ...LongWords: the caller's struct; lang's row plus word_timestamps
  {
    prompted_refusals(what, [](const LongCall& c) { return axw::long_call_options(&c.o, false); });
    refused(what, axw::long_call_options(nullptr, false));
    refused(what, axw::long_call_options(nullptr, true));
    int lang_out[2] = {9, 9};
    for (int n : {0, 1, 16}) {
      const AX_WHISPER_LONG_OPTIONS off = options_struct(n, 0), on = options_struct(n, 1);
      accepted(what, axw::long_call_options(&off, false), {false, (size_t)n, true, true, false, 1}, lang_out);
      accepted(what, axw::long_call_options(&on, false), {false, (size_t)n, true, true, true, 1});
      accepted(what, axw::long_call_options(&off, true), {false, (size_t)n, true, true, true, 1});  // RunPCMLongWords forces it on
    }
    AX_WHISPER_LONG_OPTIONS bare{};  // every part off, as a zeroed struct with NaN thresholds would be
    accepted(what, axw::long_call_options(&bare, false), {false, 0, false, true, false, 1});
    AX_WHISPER_LONG_OPTIONS named = options_struct(0, 0);
    named.file_ids = kIdsGood;
    accepted(what, axw::long_call_options(&named, false), {false, 0, true, true, false, (1 << 27) - 1});
    // the word-log pointer checks of RunPCMLongWindowsWords
    int i[8];
    int32_t t[8];
    float f[8];
    double d[8];
    const AX_WHISPER_LONG_WORD_LOG full{1, 1, i, t, i, f, i, d, d, i, i, d, d, f, nullptr};
    CHECK(axw::word_log_ok(&full, 1));
    CHECK(!axw::word_log_ok(nullptr, 0));
    AX_WHISPER_LONG_WORD_LOG w = full;
    w.seg_cap = -1; CHECK(!axw::word_log_ok(&w, 1));
    w = full; w.word_cap = -1; CHECK(!axw::word_log_ok(&w, 1));
    w = full; w.jump = nullptr; CHECK(!axw::word_log_ok(&w, 1)); CHECK(axw::word_log_ok(&w, 0));
    w = full; w.win_words = nullptr; CHECK(!axw::word_log_ok(&w, 1));
    w = full; w.text_ids = nullptr; CHECK(!axw::word_log_ok(&w, 1));
    w = full; w.token_logprob = nullptr; CHECK(!axw::word_log_ok(&w, 1));
    w = full; w.seg_end = nullptr; CHECK(!axw::word_log_ok(&w, 1)); w.seg_cap = 0; CHECK(axw::word_log_ok(&w, 1));
    w = full; w.word_prob = nullptr; CHECK(!axw::word_log_ok(&w, 1)); w.word_cap = 0; CHECK(axw::word_log_ok(&w, 1));
  }

  what = "outputs";  // the NULL and size checks of the window-log forms
  {
    const float x[4] = {0, 0, 0, 0};
    const float* pcm[2] = {x, x};
    const float* hole[2] = {x, nullptr};
    const int n[2] = {4, 4}, zero[2] = {4, 0};
    CHECK(axw::long_files_ok(pcm, n, 2));
    CHECK(!axw::long_files_ok(nullptr, n, 2) && !axw::long_files_ok(pcm, nullptr, 2) && !axw::long_files_ok(pcm, n, 0));
    CHECK(!axw::long_files_ok(hole, n, 2) && !axw::long_files_ok(pcm, zero, 2));
    int info[7], nw;
    int32_t ids[8];
    float sc[7];
    CHECK(axw::window_log_ok({1, info, ids, nullptr, nullptr, &nw, nullptr, nullptr}, false));
    CHECK(!axw::window_log_ok({1, info, ids, nullptr, nullptr, &nw, nullptr, nullptr}, true));  // a scored call needs win_score
    CHECK(axw::window_log_ok({1, info, ids, sc, nullptr, &nw, nullptr, nullptr}, true));
    CHECK(axw::window_log_ok({0, nullptr, nullptr, nullptr, nullptr, &nw, nullptr, nullptr}, true));  // win_cap 0 asks for the count only
    CHECK(!axw::window_log_ok({-1, info, ids, sc, nullptr, &nw, nullptr, nullptr}, true));
    CHECK(!axw::window_log_ok({1, info, ids, sc, nullptr, nullptr, nullptr, nullptr}, true));
    CHECK(!axw::window_log_ok({1, nullptr, ids, sc, nullptr, &nw, nullptr, nullptr}, false));
    CHECK(!axw::window_log_ok({1, info, nullptr, sc, nullptr, &nw, nullptr, nullptr}, false));
  }

  printf("long_call_table: %d failures\n", failures);
  return failures ? 1 : 0;
}
