// whisper_cli.cpp — command-line entry point, MI355X build.
//
// Keeps the reference CLI's contract (cpp/whisper_cli.cpp:19-110): flags --wav/-w (required),
// --model_type/-t (default "turbo"), --model_path/-p, --language (no short flag), and the stdout
// lines "wav_file:", "model_path:", "model_type:", "language:", "Init whisper success, take
// %.4fseconds", "Result: %s", "RTF: %.4f" where RTF = wall time of AX_WHISPER_RunFile / true clip
// duration (:76,93-103). The AX_SYS_Init / AX_ENGINE_Init block (:37-61) is gone: the library
// initialises the GPU itself. Only the C ABI is used.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ax_whisper_api.h"
#include "suppress_flag.hpp"

static void usage(const char* prog) {
  fprintf(stderr,
          "usage: %s --wav=string [options] ...\noptions:\n"
          "  -w, --wav           wav file (string)\n"
          "  -t, --model_type    tiny, base, small, turbo, large (string [=turbo])\n"
          "  -p, --model_path    model path which contains tiny/ base/ small/ turbo/ (string [=../models-mi355x])\n"
          "      --language      en, zh (string [=zh])\n"
          "      --timestamps    after Result:, one line per segment: [mm:ss.mmm --> mm:ss.mmm] text\n"
          "      --word_timestamps   (with --timestamps alone, or with --long) under every segment line one indented line per word:\n"
          "                      [mm:ss.mmm --> mm:ss.mmm] word (probability); the segment times are those the word rule leaves.\n"
          "                      With --long the seek follows the last word's end, as openai-whisper's transcribe(word_timestamps=True)\n"
          "      --beam_size N   (with --timestamps, not with --long) the segment lines are those of beam search's winner over N\n"
          "                      hypotheses (1 .. 8; openai-whisper's CLI uses 5) instead of the greedy decode's\n"
          "      --chunked       (with --long) choose every window before decoding, cut at the quietest frame of a search range, and decode\n"
          "                      the windows side by side: faster on one long file; windows are decoded independently (no fallback, prompts,\n"
          "                      language detection or word timestamps)\n"
          "      --chunk_max_s S, --chunk_min_s S, --chunk_smooth_ms MS   (with --chunked) the longest and shortest window [=30, 20] and\n"
          "                      the width of the level's smoothing box [=510]\n"
          "      --long          transcribe the whole file, not only its first 30 s: Result: is the whole text, followed by\n"
          "                      one [mm:ss.mmm --> mm:ss.mmm] line per segment with times from the file's start (hours\n"
          "                      roll into the minutes: 75:03.120). RTF: is wall time over the file's duration; without\n"
          "                      --long it divides by the whole duration although at most 30 s are decoded\n"
          "      --no_speech_threshold X, --logprob_threshold Y   (with --long) skip a window whose no-speech probability is above X\n"
          "                      unless its average token log-probability is above Y (without X nothing is skipped, without Y the\n"
          "                      no-speech probability alone decides; openai-whisper uses 0.6 and -1.0). Each segment line then ends\n"
          "                      in (avg_logprob ..., no_speech ...)\n"
          "      --compression_ratio_threshold Z   (with --long) temperature fallback: a window whose text compresses by more than Z\n"
          "                      (a repetition loop), or whose average log-probability is below Y, is decoded again with sampling\n"
          "                      at temperatures 0.2, 0.4, .. 1.0 until one attempt passes (openai-whisper uses 2.4)\n"
          "      --temperature_increment D, --seed N   the step between those temperatures [=0.2], the seed of the draws [=0]\n"
          "      --condition_on_previous_text   (with --long) every window is prompted with the text kept before it (openai-whisper's\n"
          "                      default); a window kept at a temperature above 0.5 starts the prompt afresh\n"
          "      --prompt_ids 1,2,3   (with --long) the file's initial prompt, as token ids (there is no text encoder here)\n"
          "      --detect_language   (with --timestamps or --long, not with --beam_size) detect the language from the first 30 s and\n"
          "                      decode under it; prints Detected language: <code> (p = ...) before Result:. (--language keeps its\n"
          "                      meaning: the handle's language, where an unknown code silently becomes zh; it has no \"auto\")\n"
          "      --resample      a file whose sample rate is not 16000 Hz is converted to 16 kHz on the GPU first, by the file's own\n"
          "                      rate (1000 .. 384000 Hz; AX_WHISPER_LoadAudioFile16k); every mode above then works on it, and the\n"
          "                      duration behind RTF: is the file's real one. Without the flag nothing changes: such a file is fed\n"
          "                      as it is, with a warning, and its duration is counted at 16000 Hz\n"
          "      --task T        transcribe or translate (with --timestamps or --long, not with --beam_size) [=transcribe]\n"
          "      --cross_kv h16|fp8   fp8: keep the cross K/V as e4m3fn codes too; decoder steps of more than two clips read them\n"
          "                      (opt-in, results differ from h16; not under --beam_size)\n"
          "      --suppress_tokens -1|1,2,3   (with --timestamps or --long) ids the decode never samples, as openai-whisper's\n"
          "                      suppress_tokens: -1 the non-speech ids of the model's tokens file (brackets, quotes, musical signs),\n"
          "                      or a list; replaces what the config file's \"suppress_tokens\" gave\n"
          "  -?, --help          print this message\n",
          prog);
}

// frame count of a RIFF/WAVE or FORM/AIFF file (the reference loads the file with AudioFile only to get
// duration = n_samples / 16000, whisper_cli.cpp:68-76)
static bool wav_frames(const char* path, long* frames) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  unsigned char h[12];
  if (fread(h, 1, 12, f) != 12) { fclose(f); return false; }
  if (!memcmp(h, "FORM", 4) && (!memcmp(h + 8, "AIFF", 4) || !memcmp(h + 8, "AIFC", 4))) {  // AIFF: frames from the COMM chunk
    for (;;) {
      unsigned char c[8];
      if (fread(c, 1, 8, f) != 8) { fclose(f); return false; }
      const unsigned len = ((unsigned)c[4] << 24) | (c[5] << 16) | (c[6] << 8) | c[7];
      if (!memcmp(c, "COMM", 4)) {
        unsigned char cm[6];
        if (len < 18 || fread(cm, 1, 6, f) != 6) { fclose(f); return false; }
        fclose(f);
        *frames = (long)(((unsigned)cm[2] << 24) | (cm[3] << 16) | (cm[4] << 8) | cm[5]);
        return true;
      }
      fseek(f, (long)(len + (len & 1)), SEEK_CUR);
    }
  }
  if (memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) { fclose(f); return false; }
  int ch = 0, bits = 0;
  for (;;) {
    unsigned char c[8];
    if (fread(c, 1, 8, f) != 8) { fclose(f); return false; }
    unsigned len = c[4] | (c[5] << 8) | (c[6] << 16) | ((unsigned)c[7] << 24);
    if (!memcmp(c, "fmt ", 4)) {
      unsigned char fm[16];
      if (len < 16 || fread(fm, 1, 16, f) != 16) { fclose(f); return false; }
      ch = fm[2] | (fm[3] << 8);
      bits = fm[14] | (fm[15] << 8);
      fseek(f, (long)(len - 16 + (len & 1)), SEEK_CUR);
    } else if (!memcmp(c, "data", 4)) {
      fclose(f);
      const int frame_bytes = ch * (bits / 8);  // 0 for a bit depth below 8: not a format load_wav accepts either
      if (frame_bytes <= 0) return false;
      *frames = (long)len / frame_bytes;
      return true;
    } else {
      fseek(f, (long)(len + (len & 1)), SEEK_CUR);
    }
  }
}

// --resample: the file's samples at 16 kHz (AX_WHISPER_LoadAudioFile16k: file decode + GPU resampling); else the file's samples as
// they are. info3 (or null): the file's sample rate, channels, samples per channel.
static bool g_resample = false;
static int load_pcm(AX_WHISPER_HANDLE h, const char* wav, float** pcm, int* n, int* info3 = nullptr) {
  if (g_resample) return AX_WHISPER_LoadAudioFile16k(h, wav, pcm, n, info3);
  return AX_WHISPER_LoadAudioFile(wav, pcm, n, nullptr);
}

static std::string mmss_ms(long ms) {
  char b[32];
  snprintf(b, sizeof b, "%02ld:%02ld.%03ld", ms / 60000, (ms / 1000) % 60, ms % 1000);
  return b;
}
static std::string mmss(float t) { return mmss_ms((long)(t * 1000.f + 0.5f)); }

// the language of the first 30 s (AX_WHISPER_DetectLanguage) and its "Detected language:" line; -1 on failure
static int detect_and_print(AX_WHISPER_HANDLE h, const float* pcm, int n) {
  const int n_lang = AX_WHISPER_GetConfigInt(h, "n_lang");
  if (n_lang < 1) return -1;
  std::vector<float> lp((size_t)n_lang);
  const float* clips[1] = {pcm};
  const int n30 = n < 480000 ? n : 480000;
  int idx = -1;
  if (AX_WHISPER_DetectLanguage(h, clips, &n30, 1, &idx, lp.data()) != 0 || idx < 0 || idx >= n_lang) return -1;
  const char* code = AX_WHISPER_LanguageCode(h, idx);
  printf("Detected language: %s (p = %.4f)\n", code ? code : "?", std::exp(lp[(size_t)idx]));
  return idx;
}

// detect / task >= 0 (--detect_language, --task): the clip is decoded under the detected (else the handle's) language and that task
// (AX_WHISPER_RunPCMBatchTimestampLang); then Result: is printed here too, from the same ids, and the text follows that language
static int print_segments(AX_WHISPER_HANDLE h, const char* wav, int beam_size, bool detect = false, int task = -1) {
  const bool per_lang = detect || task >= 0;
  float* pcm = nullptr;
  int n = 0;
  if (load_pcm(h, wav, &pcm, &n) != 0 || n < 1) { free(pcm); return -1; }
  const int n_ctx = AX_WHISPER_GetConfigInt(h, "n_text_ctx");
  std::vector<int32_t> ids(n_ctx > 0 ? n_ctx : 448);
  int n_ids = 0;
  const float* clips[1] = {pcm};
  float sum_lp = 0.f, avg_lp = 0.f, nsp = 0.f;
  int ended = 0, lang = -1;
  int rc;
  if (per_lang) {
    if (detect && (lang = detect_and_print(h, pcm, n)) < 0) { free(pcm); return -1; }
    const int tk = task > 0 ? 1 : 0;
    std::vector<float> tok_lp(ids.size());
    const int want = lang;
    rc = AX_WHISPER_RunPCMBatchTimestampLang(h, clips, &n, 1, 0, nullptr, nullptr, 0, nullptr, &want, &tk, ids.data(), &n_ids, tok_lp.data(), &avg_lp,
                                             &nsp, &ended, &lang, nullptr);
    if (rc == 0) {
      std::vector<int32_t> text_ids;
      const int E = AX_WHISPER_GetConfigInt(h, "eot");
      for (int i = 0; i < n_ids; ++i)
        if (ids[i] < E) text_ids.push_back(ids[i]);
      char* text = nullptr;
      if (AX_WHISPER_TranscriptLang(h, text_ids.data(), (int)text_ids.size(), lang, &text) != 0) { free(pcm); return -1; }
      printf("Result: %s\n", text ? text : "");
      free(text);
    }
  } else {
    rc = beam_size > 1 ? AX_WHISPER_RunPCMBatchBeam(h, clips, &n, 1, beam_size, 0, ids.data(), &n_ids, &sum_lp, &avg_lp, &nsp, &ended)
                       : AX_WHISPER_RunPCMBatchTimestampTokens(h, clips, &n, 1, 0, nullptr, ids.data(), &n_ids);
  }
  free(pcm);
  if (rc != 0) return -1;
  const float clip_s = n / 16000.f < 30.f ? n / 16000.f : 30.f;
  const int n_max = n_ids / 2 + 1;
  std::vector<float> st(n_max), en(n_max);
  std::vector<int> tb(n_max), te(n_max);
  int n_seg = 0;
  if (AX_WHISPER_SplitSegments(ids.data(), n_ids, AX_WHISPER_GetConfigInt(h, "timestamp_begin"), AX_WHISPER_GetConfigInt(h, "eot"), clip_s,
                               n_max, st.data(), en.data(), tb.data(), te.data(), &n_seg) != 0)
    return -1;
  for (int k = 0; k < n_seg; ++k) {
    char* text = nullptr;
    if ((per_lang ? AX_WHISPER_TranscriptLang(h, ids.data() + tb[k], te[k] - tb[k], lang, &text)
                  : AX_WHISPER_Transcript(h, ids.data() + tb[k], te[k] - tb[k], &text)) != 0)
      return -1;
    printf("[%s --> %s] %s\n", mmss(st[k]).c_str(), mmss(en[k]).c_str(), text ? text : "");
    free(text);
  }
  return 0;
}

// --timestamps --word_timestamps: the segment lines of the greedy timestamp decode with the times the word rule leaves them, and under
// each one indented line per word (AX_WHISPER_RunPCMBatchWordTimestamps)
static int print_words(AX_WHISPER_HANDLE h, const char* wav) {
  float* pcm = nullptr;
  int n = 0;
  if (load_pcm(h, wav, &pcm, &n) != 0 || n < 1) { free(pcm); return -1; }
  const int n_ctx = AX_WHISPER_GetConfigInt(h, "n_text_ctx") > 0 ? AX_WHISPER_GetConfigInt(h, "n_text_ctx") : 448;
  std::vector<int32_t> ids(n_ctx);
  std::vector<int> wseg(n_ctx), wte(n_ctx);
  std::vector<double> ss(n_ctx), se(n_ctx), ws(n_ctx), we(n_ctx);
  std::vector<float> wp(n_ctx);
  int n_ids = 0, n_seg = 0, n_words = 0;
  char* text = nullptr;
  const float* clips[1] = {pcm};
  const int rc = AX_WHISPER_RunPCMBatchWordTimestamps(h, clips, &n, 1, 0, nullptr, nullptr, ids.data(), &n_ids, nullptr, n_ctx, &n_seg, ss.data(), se.data(),
                                                      &n_words, wseg.data(), wte.data(), ws.data(), we.data(), wp.data(), &text, nullptr, nullptr);
  free(pcm);
  if (rc != 0) { free(text); return -1; }
  const float clip_s = n / 16000.f < 30.f ? n / 16000.f : 30.f;
  const int n_max = n_ids / 2 + 1;
  std::vector<float> st(n_max), en(n_max);
  std::vector<int> tb(n_max), te(n_max);
  int n_split = 0;
  if (AX_WHISPER_SplitSegments(ids.data(), n_ids, AX_WHISPER_GetConfigInt(h, "timestamp_begin"), AX_WHISPER_GetConfigInt(h, "eot"), clip_s, n_max,
                               st.data(), en.data(), tb.data(), te.data(), &n_split) != 0 || n_split != n_seg) {
    free(text);
    return -1;
  }
  for (int k = 0, w = 0; k < n_seg; ++k) {
    char* seg_text = nullptr;
    if (AX_WHISPER_Transcript(h, ids.data() + tb[k], te[k] - tb[k], &seg_text) != 0) { free(text); return -1; }
    printf("[%s --> %s] %s\n", mmss((float)ss[k]).c_str(), mmss((float)se[k]).c_str(), seg_text ? seg_text : "");
    free(seg_text);
    for (; w < n_words && wseg[w] == k; ++w) {
      const int b = w ? wte[w - 1] : 0;
      printf("  [%s --> %s] %.*s (%.3f)\n", mmss((float)ws[w]).c_str(), mmss((float)we[w]).c_str(), wte[w] - b, text + b, wp[w]);
    }
  }
  free(text);
  return 0;
}

// ---- --long. Shared by its modes: the options as the library's struct, and one file's samples with the buffers of its window log.
// n_initial / lang / task are the caller's own (the struct points at them); no temperatures: a NULL list.
static AX_WHISPER_LONG_OPTIONS long_options(float no_speech_threshold, float logprob_threshold, float compression_ratio_threshold,
                                            const std::vector<float>& temps, unsigned long long seed, const std::vector<int32_t>& prompt_ids,
                                            const int* n_initial, bool condition, const int* lang, const int* task, bool word_timestamps) {
  AX_WHISPER_LONG_OPTIONS o{};
  o.no_speech_threshold = no_speech_threshold; o.logprob_threshold = logprob_threshold; o.compression_ratio_threshold = compression_ratio_threshold;
  o.temperatures = temps.empty() ? nullptr : temps.data(); o.n_temperatures = (int)temps.size(); o.seed = seed;
  o.initial_prompt_ids = prompt_ids.data(); o.prompt_stride = *n_initial; o.n_initial = n_initial; o.condition_on_previous_text = condition ? 1 : 0;
  o.lang = lang; o.task = task; o.word_timestamps = word_timestamps ? 1 : 0;
  return o;
}

struct LongLog {
  float* pcm = nullptr;
  int n = 0, n_ctx = 448, n_win = 0;
  size_t sw = 0;  // floats per score row: 0 (unscored), 3, or 7 with fallback
  std::vector<int> info;
  std::vector<int32_t> ids;
  std::vector<float> score;
  ~LongLog() { free(pcm); }
  bool load(AX_WHISPER_HANDLE h, const char* wav) {
    if (AX_WHISPER_GetConfigInt(h, "n_text_ctx") > 0) n_ctx = AX_WHISPER_GetConfigInt(h, "n_text_ctx");
    return load_pcm(h, wav, &pcm, &n) == 0 && n >= 1;
  }
  void size(int cap, size_t score_width) { sw = score_width; info.resize((size_t)cap * 7); ids.resize((size_t)cap * n_ctx); score.resize((size_t)cap * sw); }
  // Text and lines of the log: silent windows and attempts that were decoded again print nothing, the other lines end in their
  // window's numbers. segs(info row, ids, n_max, start_ms, end_ms, tok_begin, tok_end) -> the window's segments in file time, or -1.
  // (absolute times in integer milliseconds: a float second loses the millisecond after a few hours)
  template <typename Segs>
  int print(AX_WHISPER_HANDLE h, bool per_lang, int lang, Segs&& segs, std::string& text, std::string& lines) const {
    for (int k = 0; k < n_win; ++k) {
      const float* sc = sw ? &score[(size_t)k * sw] : nullptr;
      if ((sw && sc[2] != 0.f) || (sw == 7 && sc[6] == 0.f)) continue;
      char tail[160] = "";
      if (sw) snprintf(tail, sizeof tail, " (avg_logprob %.4f, no_speech %.3g)", sc[1], std::exp(sc[0]));
      if (sw == 7)
        snprintf(tail, sizeof tail, " (avg_logprob %.4f, no_speech %.3g, temperature %.1f, compression_ratio %.3f)", sc[1], std::exp(sc[0]), sc[4], sc[5]);
      const int* w = &info[(size_t)k * 7];
      const int32_t* wi = &ids[(size_t)k * n_ctx];
      const int n_max = w[4] / 2 + 1;
      std::vector<long> st(n_max), en(n_max);
      std::vector<int> tb(n_max), te(n_max);
      const int n_seg = segs(w, wi, n_max, st.data(), en.data(), tb.data(), te.data());
      if (n_seg < 0) return -1;
      for (int s = 0; s < n_seg; ++s) {
        char* t = nullptr;
        if ((per_lang ? AX_WHISPER_TranscriptLang(h, wi + tb[s], te[s] - tb[s], lang, &t) : AX_WHISPER_Transcript(h, wi + tb[s], te[s] - tb[s], &t)) != 0)
          return -1;
        text += t ? t : "";
        lines += "[" + mmss_ms(st[s]) + " --> " + mmss_ms(en[s]) + "] " + (t ? t : "") + tail + "\n";
        free(t);
      }
    }
    return 0;
  }
};

// --long: the seek loop over the whole file (AX_WHISPER_RunPCMLongWindows), its text, then one line per segment.
// scored: under the silent-window rule (AX_WHISPER_RunPCMLongWindowsScored); skipped windows print nothing, the other lines end
// in their window's two numbers
// temps non-empty: with temperature fallback (AX_WHISPER_RunPCMLongWindowsFallback): only kept attempts print
// prompted: under prompt conditioning (AX_WHISPER_RunPCMLongWindowsPrompted; always scored)
// detect / task >= 0: under a detected language (its line is printed here) or a task (AX_WHISPER_RunPCMLongWindowsLang; always
// scored, prompts and fallback as asked for); the text then follows the file's language
static int run_long(AX_WHISPER_HANDLE h, const char* wav, bool scored, float no_speech_threshold, float logprob_threshold,
                    float compression_ratio_threshold, const std::vector<float>& temps, unsigned long long seed, bool prompted,
                    const std::vector<int32_t>& prompt_ids, bool condition, std::string& text, std::string& lines, bool detect = false,
                    int task = -1) {
  const bool per_lang = detect || task >= 0;
  const bool fallback = !temps.empty();
  LongLog L;
  if (!L.load(h, wav)) return -1;
  const int cap = (L.n / 160 + 1) * (fallback ? (int)temps.size() : 1);  // every window advances by at least one frame (after at most temps.size() attempts)
  L.size(cap, !scored ? 0 : fallback ? 7 : 3);
  const float* files[1] = {L.pcm};
  const int n_initial = (int)prompt_ids.size(), tk = task > 0 ? 1 : 0;
  int lang = -1;
  if (detect && (lang = detect_and_print(h, L.pcm, L.n)) < 0) return -1;
  const int want = lang;
  const AX_WHISPER_LONG_OPTIONS o = long_options(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temps, seed, prompt_ids, &n_initial,
                                                 condition, &want, &tk, false);
  int* const info = L.info.data();
  int32_t* const ids = L.ids.data();
  float* const score = L.score.data();
  const int rc = per_lang ? AX_WHISPER_RunPCMLongWindowsLang(h, files, &L.n, 1, 0, 0, o.no_speech_threshold, o.logprob_threshold, o.compression_ratio_threshold,
                                                             o.temperatures, o.n_temperatures, o.seed, nullptr, o.initial_prompt_ids, o.prompt_stride,
                                                             o.n_initial, o.condition_on_previous_text, o.lang, o.task, cap, info, ids, score, nullptr,
                                                             &L.n_win, &lang)
                 : prompted ? AX_WHISPER_RunPCMLongWindowsPrompted(h, files, &L.n, 1, 0, 0, o.no_speech_threshold, o.logprob_threshold,
                                                                 o.compression_ratio_threshold, o.temperatures, o.n_temperatures, o.seed, nullptr,
                                                                 o.initial_prompt_ids, o.prompt_stride, o.n_initial, o.condition_on_previous_text, cap,
                                                                 info, ids, score, nullptr, &L.n_win)
                 : fallback ? AX_WHISPER_RunPCMLongWindowsFallback(h, files, &L.n, 1, 0, 0, o.no_speech_threshold, o.logprob_threshold,
                                                                 o.compression_ratio_threshold, o.temperatures, o.n_temperatures, o.seed, nullptr, cap,
                                                                 info, ids, score, &L.n_win)
                 : scored ? AX_WHISPER_RunPCMLongWindowsScored(h, files, &L.n, 1, 0, 0, o.no_speech_threshold, o.logprob_threshold, cap, info, ids, score,
                                                             &L.n_win)
                        : AX_WHISPER_RunPCMLongWindows(h, files, &L.n, 1, 0, 0, cap, info, ids, &L.n_win);
  if (rc != 0) return -1;
  const int T = AX_WHISPER_GetConfigInt(h, "timestamp_begin"), E = AX_WHISPER_GetConfigInt(h, "eot");
  return L.print(h, per_lang, lang, [&](const int* w, const int32_t* wi, int n_max, long* st, long* en, int* tb, int* te) {
    std::vector<float> s(n_max), e(n_max);
    int n_seg = 0, adv = 0;
    if (AX_WHISPER_SplitWindow(wi, w[4], T, E, w[2], n_max, s.data(), e.data(), tb, te, &n_seg, &adv) != 0) return -1;
    for (int k = 0; k < n_seg; ++k) { st[k] = w[1] * 10L + (long)(s[k] * 1000.f + 0.5f); en[k] = w[1] * 10L + (long)(e[k] * 1000.f + 0.5f); }
    return n_seg;
  }, text, lines);
}

// --long --chunked: the windows are chosen before decoding (cuts at quiet frames) and decoded side by side
// (AX_WHISPER_RunPCMLongChunkedWindows); the text, then one line per segment of AX_WHISPER_ChunkedSegments in file time. What the
// mode does not cover (fallback, prompts, detection, words) is handed on and refused by the library with its text.
static int run_long_chunked(AX_WHISPER_HANDLE h, const char* wav, const AX_WHISPER_CHUNK_OPTIONS& chunk, bool scored, float no_speech_threshold,
                            float logprob_threshold, float compression_ratio_threshold, const std::vector<float>& temps, const std::vector<int32_t>& prompt_ids,
                            bool condition, bool detect, int task, bool word_timestamps, std::string& text, std::string& lines) {
  LongLog L;
  if (!L.load(h, wav)) return -1;
  const int cap = L.n / 160 / (chunk.min_frames > 0 ? chunk.min_frames : 1) + 2;
  L.size(cap, scored ? 3 : 0);
  const float* files[1] = {L.pcm};
  const int n_initial = (int)prompt_ids.size(), lang = detect ? -2 : -1, tk = task > 0 ? 1 : 0;
  const bool per_lang = detect || task >= 0;
  AX_WHISPER_LONG_OPTIONS o = long_options(scored ? no_speech_threshold : NAN, scored ? logprob_threshold : NAN, compression_ratio_threshold, temps, 0,
                                           prompt_ids, &n_initial, condition, per_lang ? &lang : nullptr, per_lang ? &tk : nullptr, word_timestamps);
  if (prompt_ids.empty()) { o.initial_prompt_ids = nullptr; o.n_initial = nullptr; }
  if (AX_WHISPER_RunPCMLongChunkedWindows(h, files, &L.n, 1, 0, 0, &chunk, &o, cap, L.info.data(), L.ids.data(), scored ? L.score.data() : nullptr,
                                          &L.n_win) != 0)
    return -1;
  const int T = AX_WHISPER_GetConfigInt(h, "timestamp_begin"), E = AX_WHISPER_GetConfigInt(h, "eot");
  return L.print(h, false, -1, [&](const int* w, const int32_t* wi, int n_max, long* st, long* en, int* tb, int* te) {
    std::vector<double> s(n_max), e(n_max);
    int n_seg = 0;
    if (AX_WHISPER_ChunkedSegments(wi, w[4], T, E, w[1], w[2], n_max, s.data(), e.data(), tb, te, &n_seg) != 0) return -1;
    for (int k = 0; k < n_seg; ++k) { st[k] = (long)(s[k] * 1000.0 + 0.5); en[k] = (long)(e[k] * 1000.0 + 0.5); }
    return n_seg;
  }, text, lines);
}

// --long --word_timestamps: the seek loop with words (AX_WHISPER_RunPCMLongWords) under the same thresholds, fallback, prompts, language
// and task as run_long: the whole text, then one line per segment (the times the word rule left) and under it one indented line per word
static int run_long_words(AX_WHISPER_HANDLE h, const char* wav, float no_speech_threshold, float logprob_threshold, float compression_ratio_threshold,
                          const std::vector<float>& temps, unsigned long long seed, const std::vector<int32_t>& prompt_ids, bool condition,
                          std::string& text, std::string& lines, bool detect, int task) {
  LongLog L;  // (the samples only)
  if (!L.load(h, wav)) return -1;
  int lang = -1;
  if (detect && (lang = detect_and_print(h, L.pcm, L.n)) < 0) return -1;
  const int want = lang, tk = task > 0 ? 1 : 0, n_initial = (int)prompt_ids.size();
  const AX_WHISPER_LONG_OPTIONS o = long_options(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temps, seed, prompt_ids, &n_initial,
                                                 condition, &want, &tk, true);
  AX_WHISPER_LONG_WORDS r{};
  if (AX_WHISPER_RunPCMLongWords(h, L.pcm, L.n, &o, nullptr, &r) != 0) return -1;
  for (int k = 0, w = 0; k < r.n_segments; ++k) {
    const int sb = k ? r.seg_text_end[k - 1] : 0;
    const std::string seg(r.seg_text + sb, r.seg_text + r.seg_text_end[k]);
    text += seg;
    lines += "[" + mmss_ms((long)(r.seg_start[k] * 1000.0 + 0.5)) + " --> " + mmss_ms((long)(r.seg_end[k] * 1000.0 + 0.5)) + "] " + seg + "\n";
    for (; w < r.n_words && r.word_segment[w] == k; ++w) {
      const int b = w ? r.word_text_end[w - 1] : 0;
      char p[32];
      snprintf(p, sizeof p, " (%.3f)", r.word_prob[w]);
      lines += "  [" + mmss_ms((long)(r.word_start[w] * 1000.0 + 0.5)) + " --> " + mmss_ms((long)(r.word_end[w] * 1000.0 + 0.5)) + "] " +
               std::string(r.word_text + b, r.word_text + r.word_text_end[w]) + p + "\n";
    }
  }
  AX_WHISPER_FreeLongWords(&r);
  return 0;
}

int main(int argc, char** argv) {
  std::string wav, model_type = "turbo", model_path = "../models-mi355x", language = "zh";
  bool timestamps = false, longform = false, word_timestamps = false;
  bool condition = false, detect = false, chunked = false;
  std::string task_arg, cmax_arg, cmin_arg, csmooth_arg;
  std::string nst_arg, lpt_arg, crt_arg, tinc_arg, seed_arg, beam_arg, prompt_arg, suppress_arg, cross_kv_arg;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto val = [&](const char* lng, const char* sht, std::string& dst) -> bool {
      std::string l = std::string("--") + lng;
      if (a.rfind(l + "=", 0) == 0) { dst = a.substr(l.size() + 1); return true; }
      if (a == l || (sht && a == sht)) {
        if (i + 1 >= argc) { fprintf(stderr, "option needs value: %s\n", a.c_str()); usage(argv[0]); exit(1); }
        dst = argv[++i];
        return true;
      }
      return false;
    };
    if (val("wav", "-w", wav) || val("model_type", "-t", model_type) || val("model_path", "-p", model_path) ||
        val("language", nullptr, language) || val("no_speech_threshold", nullptr, nst_arg) || val("logprob_threshold", nullptr, lpt_arg) ||
        val("compression_ratio_threshold", nullptr, crt_arg) || val("temperature_increment", nullptr, tinc_arg) || val("seed", nullptr, seed_arg) ||
        val("beam_size", nullptr, beam_arg) || val("prompt_ids", nullptr, prompt_arg) || val("task", nullptr, task_arg) ||
        val("chunk_max_s", nullptr, cmax_arg) || val("chunk_min_s", nullptr, cmin_arg) || val("chunk_smooth_ms", nullptr, csmooth_arg) ||
        val("suppress_tokens", nullptr, suppress_arg) || val("cross_kv", nullptr, cross_kv_arg))
      continue;
    if (a == "--help" || a == "-?") { usage(argv[0]); return 0; }
    if (a == "--timestamps") { timestamps = true; continue; }
    if (a == "--word_timestamps") { word_timestamps = true; continue; }
    if (a == "--long") { longform = true; continue; }
    if (a == "--chunked") { chunked = true; continue; }
    if (a == "--resample") { g_resample = true; continue; }
    if (a == "--condition_on_previous_text") { condition = true; continue; }
    if (a == "--detect_language") { detect = true; continue; }
    fprintf(stderr, "undefined option: %s\n", a.c_str());
    usage(argv[0]);
    return 1;
  }
  if (wav.empty()) { fprintf(stderr, "need option: --wav\n"); usage(argv[0]); return 1; }
  // --cross_kv h16 | fp8: the library reads the mode from AX_WHISPER_CROSS_KV when the handle is made (a bad value fails Init)
  if (!cross_kv_arg.empty()) setenv("AX_WHISPER_CROSS_KV", cross_kv_arg.c_str(), 1);
  int beam_size = 1;
  if (!beam_arg.empty()) {
    char* end = nullptr;
    const long v = strtol(beam_arg.c_str(), &end, 10);
    if (*end || v < 1 || v > 8) { fprintf(stderr, "bad value: --beam_size %s (1 .. 8)\n", beam_arg.c_str()); return 1; }
    beam_size = (int)v;
    if (!timestamps || longform) { fprintf(stderr, "--beam_size needs --timestamps and does not go with --long\n"); usage(argv[0]); return 1; }
  }
  if ((chunked || !cmax_arg.empty() || !cmin_arg.empty() || !csmooth_arg.empty()) && (!longform || !chunked)) {
    fprintf(stderr, "--chunked needs --long; --chunk_max_s / --chunk_min_s / --chunk_smooth_ms need --long --chunked\n");
    usage(argv[0]);
    return 1;
  }
  AX_WHISPER_CHUNK_OPTIONS chunk = {3000, 2000, 25, 1};
  {
    // seconds -> frames of 10 ms, milliseconds of box width -> R (the box is 2 R + 1 frames); the library checks the ranges
    char* end = nullptr;
    if (!cmax_arg.empty()) { chunk.max_frames = (int)std::lround(strtod(cmax_arg.c_str(), &end) * 100.0); if (*end) { fprintf(stderr, "bad value: --chunk_max_s %s\n", cmax_arg.c_str()); return 1; } }
    if (!cmin_arg.empty()) { chunk.min_frames = (int)std::lround(strtod(cmin_arg.c_str(), &end) * 100.0); if (*end) { fprintf(stderr, "bad value: --chunk_min_s %s\n", cmin_arg.c_str()); return 1; } }
    if (!csmooth_arg.empty()) { chunk.smooth_frames = (int)std::lround((strtod(csmooth_arg.c_str(), &end) / 10.0 - 1.0) / 2.0); if (*end) { fprintf(stderr, "bad value: --chunk_smooth_ms %s\n", csmooth_arg.c_str()); return 1; } }
  }
  int task = -1;  // not given
  if (!task_arg.empty()) {
    if (task_arg != "transcribe" && task_arg != "translate") { fprintf(stderr, "bad value: --task %s (transcribe or translate)\n", task_arg.c_str()); return 1; }
    task = task_arg == "translate" ? 1 : 0;
  }
  const bool per_lang = detect || task >= 0;
  if (per_lang && ((!timestamps && !longform) || beam_size > 1)) {
    fprintf(stderr, "--detect_language / --task need --timestamps or --long and do not go with --beam_size\n");
    usage(argv[0]);
    return 1;
  }
  if (word_timestamps && !longform && (!timestamps || beam_size > 1 || per_lang)) {
    fprintf(stderr, "--word_timestamps needs --timestamps or --long; with --timestamps it does not go with --beam_size, --detect_language or --task\n");
    usage(argv[0]);
    return 1;
  }
  // --compression_ratio_threshold turns temperature fallback on: attempts at 0, inc, 2 inc, .. 1.0 (inc 0.2 unless given)
  const bool fallback = !crt_arg.empty();
  if ((!tinc_arg.empty() || !seed_arg.empty()) && !fallback) { fprintf(stderr, "--temperature_increment / --seed need --compression_ratio_threshold\n"); usage(argv[0]); return 1; }
  if (fallback && !longform) { fprintf(stderr, "--compression_ratio_threshold needs --long\n"); usage(argv[0]); return 1; }
  std::vector<int32_t> prompt_ids;
  for (size_t p = 0; p < prompt_arg.size();) {
    char* end = nullptr;
    const long v = strtol(prompt_arg.c_str() + p, &end, 10);
    if (end == prompt_arg.c_str() + p || v < 0 || (*end && *end != ',')) { fprintf(stderr, "bad value: --prompt_ids %s\n", prompt_arg.c_str()); return 1; }
    prompt_ids.push_back((int32_t)v);
    p = (size_t)(end - prompt_arg.c_str()) + (*end ? 1 : 0);
  }
  // --suppress_tokens -1 | 1,2,3 (suppress_flag.hpp)
  std::vector<int> suppress_ids;
  if (!suppress_arg.empty() && !timestamps && !longform) { fprintf(stderr, "--suppress_tokens needs --timestamps or --long (plain mode is not filtered)\n"); usage(argv[0]); return 1; }
  if (!suppress_arg.empty()) {
    std::string err;
    if (!suppress_flag_ids(suppress_arg, model_path, model_type, suppress_ids, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  }
  const bool prompted = condition || !prompt_ids.empty();
  if (prompted && !longform) { fprintf(stderr, "--condition_on_previous_text / --prompt_ids need --long\n"); usage(argv[0]); return 1; }
  const bool scored = prompted || fallback || !nst_arg.empty() || !lpt_arg.empty() || (per_lang && longform);
  if (scored && !longform) { fprintf(stderr, "--no_speech_threshold / --logprob_threshold need --long\n"); usage(argv[0]); return 1; }
  // one flag alone: no threshold on the average = no-speech alone decides (+inf); no threshold on no-speech = nothing is skipped
  // (NaN; as in openai-whisper, where the average only ever overrides a no-speech verdict) and the lines just carry their numbers
  float no_speech_threshold = NAN, logprob_threshold = INFINITY;
  {
    char* end = nullptr;
    if (!nst_arg.empty()) { no_speech_threshold = strtof(nst_arg.c_str(), &end); if (*end) { fprintf(stderr, "bad value: --no_speech_threshold %s\n", nst_arg.c_str()); return 1; } }
    if (!lpt_arg.empty()) { logprob_threshold = strtof(lpt_arg.c_str(), &end); if (*end) { fprintf(stderr, "bad value: --logprob_threshold %s\n", lpt_arg.c_str()); return 1; } }
  }
  float compression_ratio_threshold = NAN;
  std::vector<float> temps;
  unsigned long long seed = 0;
  if (fallback) {
    char* end = nullptr;
    compression_ratio_threshold = strtof(crt_arg.c_str(), &end);
    if (*end) { fprintf(stderr, "bad value: --compression_ratio_threshold %s\n", crt_arg.c_str()); return 1; }
    float inc = 0.2f;
    if (!tinc_arg.empty()) { inc = strtof(tinc_arg.c_str(), &end); if (*end || !(inc > 0.f) || inc > 1.f) { fprintf(stderr, "bad value: --temperature_increment %s\n", tinc_arg.c_str()); return 1; } }
    if (inc < 1.f / 15.f) { fprintf(stderr, "bad value: --temperature_increment %s (at most 16 attempts)\n", tinc_arg.c_str()); return 1; }
    for (int k = 0; (float)k * inc <= 1.f + 1e-6f; ++k) temps.push_back((float)k * inc);
    if (!seed_arg.empty()) { seed = strtoull(seed_arg.c_str(), &end, 0); if (*end) { fprintf(stderr, "bad value: --seed %s\n", seed_arg.c_str()); return 1; } }
    if (lpt_arg.empty()) logprob_threshold = NAN;  // (no threshold on the average: that part of the fallback rule is off)
  }

  printf("wav_file: %s\n", wav.c_str());
  printf("model_path: %s\n", model_path.c_str());
  printf("model_type: %s\n", model_type.c_str());
  printf("language: %s\n", language.c_str());

  long frames = 0;
  if (!wav_frames(wav.c_str(), &frames) || frames <= 0) { printf("load wav failed!\n"); return -1; }
  float duration = frames * 1.f / 16000;

  auto t0 = std::chrono::steady_clock::now();
  // (beam search: one decoder slot per hypothesis)
  // (chunked long-form: 16 windows side by side unless AX_WHISPER_MAX_BATCH says otherwise)
  AX_WHISPER_HANDLE handle = beam_size > 1 ? AX_WHISPER_InitEx(model_type.c_str(), model_path.c_str(), language.c_str(), -1, beam_size)
                             : chunked && !getenv("AX_WHISPER_MAX_BATCH") ? AX_WHISPER_InitEx(model_type.c_str(), model_path.c_str(), language.c_str(), -1, 16)
                                           : AX_WHISPER_Init(model_type.c_str(), model_path.c_str(), language.c_str());
  auto t1 = std::chrono::steady_clock::now();
  if (!handle) { printf("AX_WHISPER_Init failed!\n"); return -1; }
  printf("Init whisper success, take %.4fseconds\n", std::chrono::duration<double>(t1 - t0).count());
  if (!suppress_ids.empty()) {
    if (AX_WHISPER_SetSuppressTokens(handle, suppress_ids.data(), (int)suppress_ids.size()) != 0) {
      printf("--suppress_tokens failed! %s\n", AX_WHISPER_LastError(handle));
      AX_WHISPER_Uninit(handle);
      return -1;
    }
    printf("suppress_tokens: %d ids\n", (int)suppress_ids.size());
  }
  if (g_resample) {  // the file's real duration: its frames at its own rate
    float* pcm = nullptr;
    int n = 0, info[3] = {0, 0, 0};
    if (load_pcm(handle, wav.c_str(), &pcm, &n, info) != 0 || info[0] < 1) {
      printf("load wav failed! %s\n", AX_WHISPER_LastError(handle));
      free(pcm);
      AX_WHISPER_Uninit(handle);
      return -1;
    }
    free(pcm);
    duration = info[2] * 1.f / info[0];
  }

  if (longform) {
    t0 = std::chrono::steady_clock::now();
    std::string text, lines;
    if ((chunked ? run_long_chunked(handle, wav.c_str(), chunk, !nst_arg.empty() || !lpt_arg.empty(), no_speech_threshold, logprob_threshold,
                                    compression_ratio_threshold, temps, prompt_ids, condition, detect, task, word_timestamps, text, lines)
         : word_timestamps ? run_long_words(handle, wav.c_str(), no_speech_threshold, logprob_threshold, compression_ratio_threshold, temps, seed, prompt_ids,
                                          condition, text, lines, detect, task)
                         : run_long(handle, wav.c_str(), scored, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temps, seed, prompted,
                                    prompt_ids, condition, text, lines, detect, task)) != 0) {
      printf("AX_WHISPER_Run failed! %s\n", AX_WHISPER_LastError(handle));
      AX_WHISPER_Uninit(handle);
      return -1;
    }
    t1 = std::chrono::steady_clock::now();
    printf("Result: %s\n%s", text.c_str(), lines.c_str());
    printf("RTF: %.4f\n", std::chrono::duration<double>(t1 - t0).count() / duration);
    AX_WHISPER_Uninit(handle);
    return 0;
  }

  if (per_lang) {  // --timestamps under a language or task: one decode gives Result: and the segment lines
    t0 = std::chrono::steady_clock::now();
    if (print_segments(handle, wav.c_str(), 1, detect, task) != 0) {
      printf("AX_WHISPER_Run failed! %s\n", AX_WHISPER_LastError(handle));
      AX_WHISPER_Uninit(handle);
      return -1;
    }
    t1 = std::chrono::steady_clock::now();
    printf("RTF: %.4f\n", std::chrono::duration<double>(t1 - t0).count() / duration);
    AX_WHISPER_Uninit(handle);
    return 0;
  }

  t0 = std::chrono::steady_clock::now();
  char* result = nullptr;
  if (0 != (g_resample ? AX_WHISPER_RunFileResampled(handle, wav.c_str(), &result) : AX_WHISPER_RunFile(handle, wav.c_str(), &result))) {
    printf("AX_WHISPER_Run failed!\n");
    AX_WHISPER_Uninit(handle);
    return -1;
  }
  t1 = std::chrono::steady_clock::now();
  printf("Result: %s\n", result);
  const double rtf = std::chrono::duration<double>(t1 - t0).count() / duration;  // of AX_WHISPER_RunFile alone
  if (timestamps && (word_timestamps ? print_words(handle, wav.c_str()) : print_segments(handle, wav.c_str(), beam_size)) != 0) {
    printf("AX_WHISPER_Run failed! %s\n", AX_WHISPER_LastError(handle));
    free(result);
    AX_WHISPER_Uninit(handle);
    return -1;
  }
  printf("RTF: %.4f\n", rtf);
  free(result);
  AX_WHISPER_Uninit(handle);
  return 0;
}
