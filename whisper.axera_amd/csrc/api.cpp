// api.cpp — the C ABI of libax_whisper.so (include/ax_whisper_api.h).
//
// The four legacy entry points keep the reference's contract (cpp/src/api/ax_whisper_api.cpp:
// 48-56 Init, 69-74 Uninit, 88-124 RunFile, 139-163 RunPCM): NULL / -1 on failure, *result set to
// NULL before any failure after the argument checks, result strdup'd for the caller to free().
// Differences, all fixes of reference defects: no exception crosses the ABI
// (json / file errors become NULL), a failed Init does not leak, a handle is serialised by a
// mutex (the reference's handle is not re-entrant although whisper_srv calls it from a thread
// pool). The OpenCC Traditional->Simplified pass of zh transcripts (Whisper.cpp:231-236) is applied by t2s.hpp when
// the reference's t2s.json + .ocd2 dictionaries are found; AX_WHISPER_Detokenize returns the raw bytes.
#include "../../include/ax_whisper_api.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "iengine.hpp"
#include "owned.hpp"
#include "host_io.hpp"
#include "t2s.hpp"
#include "multi_device.hpp"
#include "resample.hpp"
#include "words.hpp"
#include "suppress.hpp"
#include "vocab_logprob_plan.hpp"
#include "long_call.hpp"

using Engine = axw::IEngine;

namespace axw {
std::recursive_mutex& device_capture_mutex(int device) {
  // Default: ONE mutex for the whole process, not one per device: whether an allocation on device 1 can invalidate a
  // thread-local capture on device 0 was never observable on a one-GPU box, so the exclusion does not depend on the answer.
  // The cost is that engines of one AX_WHISPER_InitMulti handle are constructed one after the other (seconds, once per
  // handle), and that creating a handle at run time stalls StreamOpen / capacity growth / first-time graph capture of every
  // serving handle for that long (INTEGRATION.md "Threading"). AX_WHISPER_CAPTURE_MUTEX=device: one mutex per device — for
  // multi-GPU hosts once the first 8-GPU run has shown that captures on different devices do not disturb each other.
  static std::recursive_mutex mu[65];
  static const bool per_device = [] { const char* e = getenv("AX_WHISPER_CAPTURE_MUTEX"); return e && !strcmp(e, "device"); }();
  return per_device ? mu[1 + (device & 63)] : mu[0];
}
std::mutex& persistent_launch_mutex(int device) {
  static std::mutex mu[64];  // one per device: engines of different GPUs never wait for each other
  return mu[device & 63];
}
}  // namespace axw

namespace {
thread_local std::string g_init_error;
struct Handle {
  axw::DeviceGroup<Engine> group;  // one engine per device; the legacy entry points create exactly one
  std::string last_error;
  std::mutex err_mu;
  void set_error(const std::string& e) {
    std::lock_guard<std::mutex> lk(err_mu);
    last_error = e;
  }
};
inline Handle* H(AX_WHISPER_HANDLE h) { return static_cast<Handle*>(h); }

// f(primary engine) under that engine's mutex; exceptions become -1 + last_error
template <typename F>
int guarded(AX_WHISPER_HANDLE handle, F&& f) {
  Handle* h = H(handle);
  if (!h || h->group.size() == 0) return -1;
  try {
    Engine& e = h->group.primary();
    std::lock_guard<std::mutex> lock(e.mutex());
    f(e);
    return 0;
  } catch (const std::exception& e) {
    h->set_error(e.what());
    fprintf(stderr, "[ax_whisper] %s\n", e.what());
    return -1;
  } catch (...) {
    h->set_error("unknown error");
    return -1;
  }
}

// f(device group): the sharded entry points; every shard locks its own engine (multi_device.hpp)
template <typename F>
int guarded_group(AX_WHISPER_HANDLE handle, F&& f) {
  Handle* h = H(handle);
  if (!h || h->group.size() == 0) return -1;
  try {
    f(h->group);
    return 0;
  } catch (const std::exception& e) {
    h->set_error(e.what());
    fprintf(stderr, "[ax_whisper] %s\n", e.what());
    return -1;
  } catch (...) {
    h->set_error("unknown error");
    return -1;
  }
}

// f(): the host-only entry points (no handle); exceptions become -1 + the thread's init error text
template <typename F>
int guarded_host(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    g_init_error = e.what();
    return -1;
  } catch (...) {
    g_init_error = "unknown error";
    return -1;
  }
}

int visible_devices() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    throw std::runtime_error("no HIP device visible: the MI355X engine has no CPU fallback");
  return n;
}
AX_WHISPER_HANDLE init_devices(const char* model_type, const char* model_path, const char* language,
                               const std::vector<int>& devices, int max_batch) {
  std::unique_ptr<Handle> h(new Handle());
  const int G = (int)devices.size();
  (void)visible_devices();  // no GPU: fail with that message, before any file is touched (there is no CPU fallback)
  std::vector<std::unique_ptr<Engine>> engines(G);
  // engines load side by side (one host thread per device): each uploads its own replica of the weights
  // 16-bit storage type of the engine: AX_WHISPER_DTYPE=bf16|fp16 when set, else the dtype of the weights file
  // (F16 -> half; BF16 and F32 -> bfloat16)
  const std::string wfile = std::string(model_path) + "/" + model_type + "/" + model_type + ".safetensors";
  bool f16 = false;
  if (const char* e = getenv("AX_WHISPER_DTYPE")) {
    const std::string v = e;
    if (v == "fp16" || v == "f16" || v == "half") f16 = true;
    else if (v != "bf16") throw std::runtime_error("AX_WHISPER_DTYPE must be bf16 or fp16");
  } else {
    axw::SafeTensors st(wfile);
    f16 = st.get("decoder.token_embedding.weight").dtype == "F16";
  }
  axw::run_sharded(G, G, [&](int w, int, int) {
    engines[w].reset(f16 ? axw::make_engine_f16(model_type, model_path, language, devices[w], max_batch)
                         : axw::make_engine_bf16(model_type, model_path, language, devices[w], max_batch));
  });
  for (auto& e : engines) h->group.add(std::move(e));
  return h.release();  // a throw above destroys every engine already built (the reference leaks: ax_whisper_api.cpp:49-53)
}

template <typename F>
AX_WHISPER_HANDLE init_guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    g_init_error = e.what();
    fprintf(stderr, "[ax_whisper] init failed: %s\n", e.what());
    return nullptr;
  } catch (...) {
    g_init_error = "unknown error";
    return nullptr;
  }
}

// the file decode of RunFile / RunFileLong: false (and the handle's error text set) when the file cannot be used
bool load_wav_for_run(AX_WHISPER_HANDLE handle, const char* wav_file, axw::WavData& wav) {
  std::string err;
  if (!axw::load_audio_file(wav_file, wav, err)) {
    H(handle)->set_error("load wav failed: " + err);
    fprintf(stderr, "[ax_whisper] load wav failed: %s\n", err.c_str());
    return false;
  }
  if (wav.mono.empty()) {
    H(handle)->set_error("wav file holds no samples");
    return false;
  }
  if (wav.sample_rate != 16000)  // the reference silently mis-transcribes (no resampler anywhere in its C++)
    fprintf(stderr, "[ax_whisper] warning: %s is %d Hz, expected 16000 Hz (see cpp/resample_wav.sh of the reference)\n",
            wav_file, wav.sample_rate);
  return true;
}

// every Run*File* form: load the file, then pcm_form(samples, n), the PCM form of the same call; *out is cleared first
template <typename T, typename F>
int run_wav(AX_WHISPER_HANDLE handle, const char* wav_file, T* out, F&& pcm_form) {
  if (!handle || !wav_file || !out) return -1;
  *out = T{};
  axw::WavData wav;
  if (!load_wav_for_run(handle, wav_file, wav)) return -1;
  return pcm_form(wav.mono.data(), (int)wav.mono.size());
}

// ---- long-form: the three bodies behind the Run*Long* exports (long_call.hpp: what an export asks for; DESIGN.md "Long-form entry
// points"). An export fills a LongCall and names its outputs; the chunked exports share the row writer and the text join.
using axw::WindowLogOut;

// Nothing of a log is written unless everything fits: the refusal names the count, and the caller comes again with that capacity.
void require_win_cap(const char* who, size_t n_windows, int win_cap) {
  if ((long)n_windows > win_cap)
    throw std::runtime_error(std::string(who) + ": " + std::to_string(n_windows) + " windows were decoded, win_cap is " + std::to_string(win_cap));
}

// the rows of a log that fits; score_width: floats per win_score row (0 unscored, 3 scored, 7 with fallback)
void write_window_rows(const std::vector<axw::LongWindow>& log, int Tc, int score_width, const WindowLogOut& out) {
  for (size_t k = 0; k < log.size(); ++k) {
    const axw::LongWindow& w = log[k];
    const int row[7] = {w.file, w.seek, w.window_frames, w.advance, (int)w.ids.size(), w.pass, w.slot};
    memcpy(out.win_info + k * 7, row, sizeof row);
    memcpy(out.ids + k * (size_t)Tc, w.ids.data(), w.ids.size() * sizeof(int32_t));
    float* sc = out.win_score + k * (size_t)score_width;
    if (score_width >= 3) { sc[0] = w.no_speech_logprob; sc[1] = w.avg_logprob; sc[2] = w.skipped ? 1.f : 0.f; }
    if (score_width == 7) { sc[3] = (float)w.attempt; sc[4] = w.temperature; sc[5] = w.compression_ratio; sc[6] = w.kept ? 1.f : 0.f; }
    if (out.win_prompt) out.win_prompt[k] = w.n_prompt;
  }
  *out.n_windows = (int)log.size();
}

// the word part of a log (word-timestamp calls), under the same rule
void write_word_log(const char* who, const std::vector<axw::LongWindow>& log, int Tc, AX_WHISPER_LONG_WORD_LOG* words) {
  size_t n_seg = 0, n_word = 0;
  for (const axw::LongWindow& w : log) { n_seg += w.seg_tokens.size(); n_word += w.words.size(); }
  if (n_seg > (size_t)words->seg_cap) throw std::runtime_error(std::string(who) + ": " + std::to_string(n_seg) + " segments, seg_cap is " + std::to_string(words->seg_cap));
  if (n_word > (size_t)words->word_cap) throw std::runtime_error(std::string(who) + ": " + std::to_string(n_word) + " words, word_cap is " + std::to_string(words->word_cap));
  std::string all;
  size_t sg = 0, wd = 0;
  for (size_t k = 0; k < log.size(); ++k) {
    const axw::LongWindow& w = log[k];
    const int row[4] = {(int)w.text_ids.size(), (int)w.seg_tokens.size(), (int)w.words.size(), w.by_word_end ? 1 : 0};
    memcpy(words->win_words + k * 4, row, sizeof row);
    std::copy(w.text_ids.begin(), w.text_ids.end(), words->text_ids + k * (size_t)Tc);
    std::copy(w.word_logprob.begin(), w.word_logprob.end(), words->token_logprob + k * (size_t)Tc);
    std::copy(w.jump.begin(), w.jump.end(), words->jump + k * (size_t)(Tc + 1));
    for (size_t s = 0; s < w.seg_tokens.size(); ++s, ++sg) {
      words->seg_tokens[sg] = w.seg_tokens[s]; words->seg_start[sg] = w.seg_start[s]; words->seg_end[sg] = w.seg_end[s];
    }
    for (const axw::LongWord& x : w.words) {
      all += x.text;
      words->word_segment[wd] = x.segment; words->word_text_end[wd] = (int)all.size(); words->word_start[wd] = x.start; words->word_end[wd] = x.end;
      words->word_prob[wd] = x.probability;
      ++wd;
    }
  }
  words->text = static_cast<char*>(malloc(all.size() + 1));
  if (!words->text) throw std::runtime_error(std::string(who) + ": out of memory");
  memcpy(words->text, all.data(), all.size());
  words->text[all.size()] = 0;
}

// Window log: the seek loop over the files of export `who`, then its log written to `out`
int long_windows(AX_WHISPER_HANDLE handle, const char* who, const float* const* pcm, const int* num_samples, int n_files, int max_new,
                 int max_passes, const axw::LongCall& call, const WindowLogOut& out) {
  axw::LongRun run;
  if (!axw::long_run_options(call, n_files, out.lang_out, run)) return -1;
  if (out.words) out.words->text = nullptr;
  if (run.opts.word_timestamps && !axw::word_log_ok(out.words, out.win_cap)) return -1;
  if (!handle || !axw::long_files_ok(pcm, num_samples, n_files) || !axw::window_log_ok(out, run.scored)) return -1;
  *out.n_windows = 0;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    std::vector<axw::LongWindow> log;
    g.run_long_windows(pcm, num_samples, n_files, max_new, max_passes, run.get(), log);
    const int Tc = g.primary().config().n_text_ctx;
    require_win_cap(who, log.size(), out.win_cap);
    if (run.opts.word_timestamps) write_word_log(who, log, Tc, out.words);
    write_window_rows(log, Tc, !run.scored ? 0 : run.opts.temperatures.empty() ? 3 : 7, out);
  });
}

// the text of a log: the segments (segs(w): tok_begin / tok_end into w.ids) of every window that stands (kept, not skipped as silent),
// joined; lang (or null: the handle's): the language index the text follows
template <typename Segs>
std::string join_segment_texts(Engine& e, const std::vector<axw::LongWindow>& log, const int* lang, Segs&& segs) {
  std::string text;
  for (const axw::LongWindow& w : log) {
    if (w.skipped || !w.kept) continue;
    for (const auto& sg : segs(w))  // host only
      text += lang ? e.transcript_lang(w.ids.data() + sg.tok_begin, sg.tok_end - sg.tok_begin, *lang)
                   : e.transcript(w.ids.data() + sg.tok_begin, sg.tok_end - sg.tok_begin);
  }
  return text;
}

// Text: the seek loop over one file, then the text of its windows. Calls that collect the language (the *Lang forms) answer it in
// *lang_out (may be NULL), and the text follows it.
int long_text(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, const axw::LongCall& call, int* lang_out, char** result) {
  axw::LongRun run;
  if (!axw::long_run_options(call, 1, nullptr, run)) return -1;
  if (!handle || !pcm_data || !result || num_samples < 1) return -1;
  *result = nullptr;
  const int rc = guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    Engine& e = g.primary();
    std::vector<axw::LongWindow> log;
    const float* files[1] = {pcm_data};
    g.run_long_windows(files, &num_samples, 1, 0, 0, run.get(), log);
    const int T = (int)e.config().ints.at("timestamp_begin"), E = e.config().eot;
    std::vector<axw::WindowSegment> segs;
    *result = strdup(join_segment_texts(e, log, run.lang.empty() ? nullptr : run.lang.data(), [&](const axw::LongWindow& w) -> const std::vector<axw::WindowSegment>& {
      axw::split_window(w.ids.data(), (int)w.ids.size(), T, E, w.window_frames, segs);
      return segs;
    }).c_str());
  });
  if (rc == 0 && lang_out && !run.lang.empty()) *lang_out = run.lang[0];
  return rc;
}

}  // namespace

extern "C" {

AX_WHISPER_API AX_WHISPER_HANDLE AX_WHISPER_InitMulti(const char* model_type, const char* model_path, const char* language,
                                                      const int* devices, int n_devices, int max_batch_per_device) {
  if (!model_type || !model_path || !language) {
    g_init_error = "null argument";
    return nullptr;
  }
  return init_guarded([&]() -> AX_WHISPER_HANDLE {
    const int n_vis = visible_devices();
    std::vector<int> devs;
    if (devices && n_devices > 0) {
      // test hook: AX_WHISPER_ALLOW_DUPLICATE_DEVICES=1 lets a one-GPU box run several engines (the sharding, the
      // worker threads, the join) against real devices; production lists must name each device once
      const char* dup = getenv("AX_WHISPER_ALLOW_DUPLICATE_DEVICES");
      if (dup && dup[0] == '1') {
        for (int i = 0; i < n_devices; ++i) {
          if (devices[i] < 0 || devices[i] >= n_vis) throw std::runtime_error("device ordinal out of range");
          devs.push_back(devices[i]);
        }
      } else {
        std::string list;
        for (int i = 0; i < n_devices; ++i) list += (i ? "," : "") + std::to_string(devices[i] < 0 ? n_vis : devices[i]);
        devs = axw::parse_device_list(list, n_vis);  // range + duplicate checks
      }
    } else {
      const char* e = getenv("AX_WHISPER_DEVICES");
      devs = axw::parse_device_list(e ? e : "all", n_vis);
    }
    return init_devices(model_type, model_path, language, devs, max_batch_per_device);
  });
}

AX_WHISPER_API AX_WHISPER_HANDLE AX_WHISPER_InitEx(const char* model_type, const char* model_path, const char* language,
                                                   int device, int max_batch) {
  if (!model_type || !model_path || !language) {
    g_init_error = "null argument";
    return nullptr;
  }
  // device < 0 and AX_WHISPER_DEVICES set ("all" or "0,1,..."): the unchanged callers of the legacy Init (whisper_cli,
  // a reference-side application) get one engine per listed device without a source change
  if (device < 0 && getenv("AX_WHISPER_DEVICES")) return AX_WHISPER_InitMulti(model_type, model_path, language, nullptr, 0, max_batch);
  return init_guarded([&]() -> AX_WHISPER_HANDLE { return init_devices(model_type, model_path, language, {device}, max_batch); });
}

AX_WHISPER_API AX_WHISPER_HANDLE AX_WHISPER_Init(const char* model_type, const char* model_path, const char* language) {
  return AX_WHISPER_InitEx(model_type, model_path, language, -1, 0);
}

AX_WHISPER_API void AX_WHISPER_Uninit(AX_WHISPER_HANDLE handle) {
  delete H(handle);  // NULL-safe (ax_whisper_api.cpp:69-74); the group destroys its engines
}

AX_WHISPER_API int AX_WHISPER_VisibleDeviceCount(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

AX_WHISPER_API int AX_WHISPER_GetDeviceCount(AX_WHISPER_HANDLE handle) {
  Handle* h = H(handle);
  return h ? h->group.size() : -1;
}

AX_WHISPER_API int AX_WHISPER_RunPCM(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, char** result) {
  if (!handle || !pcm_data || !result) return -1;
  *result = nullptr;
  return AX_WHISPER_RunPCMBatch(handle, &pcm_data, &num_samples, 1, result);
}

AX_WHISPER_API int AX_WHISPER_RunFile(AX_WHISPER_HANDLE handle, const char* wav_file, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) { return AX_WHISPER_RunPCM(handle, pcm, n, result); });
}

// What every clip-batch and stage-level function below does: fill a request (iengine.hpp) and make the one call that takes it.
static Engine::DecodeRequest timestamp_request(Engine::DecodeMode mode, int max_new, const int* max_new_clip, const Engine::ClipScores* scores) {
  Engine::DecodeRequest rq;
  rq.mode = mode; rq.max_new = max_new; rq.max_new_clip = max_new_clip;
  if (scores) rq.scores = *scores;
  return rq;
}

// prompts: present when the caller gave prompt lengths
static Engine::ClipContexts clip_contexts(const int32_t* prompt_ids, int prompt_stride, const int* n_prompt,
                                          std::optional<Engine::LangSpec> lang = std::nullopt, Engine::LangResult lang_out = {}) {
  Engine::ClipContexts c;
  if (n_prompt) c.prompts = Engine::PromptSpec{prompt_ids, prompt_stride, n_prompt};
  c.lang = lang; c.lang_out = lang_out;
  return c;
}

static void run_request(axw::DeviceGroup<Engine>& g, const Engine::DecodeRequest& rq, const float* const* pcm, const int* num_samples, int batch,
                        int32_t* ids, int* n_ids) {
  const auto& cfg = g.primary().config();
  g.run_tokens(rq, pcm, num_samples, batch, cfg.n_text_ctx, (int)cfg.lang_tokens.size(), ids, n_ids);
}

AX_WHISPER_API int AX_WHISPER_RunPCMBatchTokens(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                int batch, int max_new, int32_t* ids, int* n_ids) {
  if (!handle || !pcm || !num_samples || !ids || !n_ids || batch < 1) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    Engine::DecodeRequest rq;
    rq.max_new = max_new;
    run_request(g, rq, pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampTokens(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                         int batch, int max_new, const int* max_new_clip, int32_t* ids, int* n_ids) {
  if (!handle || !pcm || !num_samples || !ids || !n_ids || batch < 1) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    run_request(g, timestamp_request(Engine::kDecodeTimestamps, max_new, max_new_clip, nullptr), pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_RunDeviceBatchTokens(AX_WHISPER_HANDLE handle, const float* d_pcm, int stride,
                                                   const int* num_samples, int batch, int max_new, int32_t* ids, int* n_ids) {
  if (!handle || !d_pcm || !num_samples || !ids || !n_ids || batch < 1) return -1;
  return AX_WHISPER_RunDeviceBatchTokensRagged(handle, d_pcm, stride, num_samples, batch, max_new, nullptr, ids, n_ids);
}

AX_WHISPER_API int AX_WHISPER_RunDeviceBatchTokensRagged(AX_WHISPER_HANDLE handle, const float* d_pcm, int stride,
                                                         const int* num_samples, int batch, int max_new,
                                                         const int* max_new_clip, int32_t* ids, int* n_ids) {
  if (!handle || !d_pcm || !num_samples || !ids || !n_ids || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    Engine::DecodeRequest rq;
    rq.max_new = max_new; rq.max_new_clip = max_new_clip;
    e.run_tokens(rq, nullptr, d_pcm, stride, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_RunPCMBatch(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                          char** results) {
  if (!handle || !pcm || !num_samples || !results || batch < 1) return -1;
  for (int b = 0; b < batch; ++b) results[b] = nullptr;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    Engine& e = g.primary();
    const int Tc = e.config().n_text_ctx;
    std::vector<int32_t> ids((size_t)batch * Tc);
    std::vector<int> n(batch);
    run_request(g, Engine::DecodeRequest{}, pcm, num_samples, batch, ids.data(), n.data());
    for (int b = 0; b < batch; ++b) results[b] = strdup(e.transcript(ids.data() + (size_t)b * Tc, n[b]).c_str());  // host only
  });
}

AX_WHISPER_API int AX_WHISPER_Detokenize(AX_WHISPER_HANDLE handle, const int32_t* ids, int n, char** result) {
  if (!handle || (!ids && n > 0) || !result) return -1;
  *result = nullptr;
  return guarded(handle, [&](Engine& e) { *result = strdup(e.detokenize(ids, n).c_str()); });
}

AX_WHISPER_API int AX_WHISPER_Transcript(AX_WHISPER_HANDLE handle, const int32_t* ids, int n, char** result) {
  if (!handle || (!ids && n > 0) || !result) return -1;
  *result = nullptr;
  return guarded(handle, [&](Engine& e) { *result = strdup(e.transcript(ids, n).c_str()); });
}

AX_WHISPER_API int AX_WHISPER_TranscriptLang(AX_WHISPER_HANDLE handle, const int32_t* ids, int n, int lang_index, char** result) {
  if (!handle || (!ids && n > 0) || !result) return -1;
  *result = nullptr;
  return guarded(handle, [&](Engine& e) { *result = strdup(e.transcript_lang(ids, n, lang_index).c_str()); });
}

AX_WHISPER_API int AX_WHISPER_ConvertT2S(const char* config_path, const char* text, char** result) {
  if (!config_path || !text || !result) return -1;
  *result = nullptr;
  return guarded_host([&] {
    axw::T2SConverter conv(config_path);
    *result = strdup(conv.convert(text).c_str());
    return *result ? 0 : -1;
  });
}

// the two byte paths of the drop-in boundary on their own, host only (no handle, no GPU): parity tests hold them bit-equal to
// the reference's AudioFile.h / base64.cpp compiled into oracle/_ref (tests/test_byte_paths.py)
AX_WHISPER_API int AX_WHISPER_LoadAudioFile(const char* path, float** samples, int* n_samples, int* info) {
  if (!path || !samples || !n_samples) return -1;
  *samples = nullptr;
  *n_samples = 0;
  return guarded_host([&] {
    axw::WavData wav;
    std::string err;
    if (!axw::load_audio_file(path, wav, err)) { g_init_error = "load wav failed: " + err; return -1; }
    *samples = static_cast<float*>(malloc(std::max<size_t>(wav.mono.size(), 1) * sizeof(float)));
    if (!*samples) return -1;
    memcpy(*samples, wav.mono.data(), wav.mono.size() * sizeof(float));
    *n_samples = (int)wav.mono.size();
    if (info) { info[0] = wav.sample_rate; info[1] = wav.channels; }
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_DetokenizeWithTable(const char* tokens_path, const int32_t* ids, int n, char** result, int* n_bytes) {
  if (!tokens_path || (n > 0 && !ids) || !result || !n_bytes) return -1;
  *result = nullptr;
  *n_bytes = 0;
  return guarded_host([&] {
    const std::vector<std::string> table = axw::load_token_table(tokens_path);
    std::string s;
    for (int i = 0; i < n; ++i)
      if (ids[i] >= 0 && (size_t)ids[i] < table.size()) s += table[(size_t)ids[i]];
    *result = static_cast<char*>(malloc(s.size() + 1));
    if (!*result) return -1;
    memcpy(*result, s.data(), s.size());
    (*result)[s.size()] = 0;
    *n_bytes = (int)s.size();
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_GetConfigInt(AX_WHISPER_HANDLE handle, const char* key) {
  Handle* h = H(handle);
  if (!h || !key || h->group.size() == 0) return INT_MIN;
  if (!strcmp(key, "n_devices")) return h->group.size();
  if (!strcmp(key, "live_hip_objects")) return (int)axw::live_owned.load();  // test hook: of every handle of the process
  if (!strcmp(key, "persistent_giveups") || !strcmp(key, "persistent_ts_launches") || !strcmp(key, "cross_kv_fp8_launches")) {  // counts: summed over the handle's engines
    long sum = 0;
    for (int i = 0; i < h->group.size(); ++i) {
      Engine& e = h->group.at(i);
      std::lock_guard<std::mutex> lock(e.mutex());
      auto it = e.config().ints.find(key);
      if (it != e.config().ints.end()) sum += it->second;
    }
    return (int)sum;
  }
  Engine& e = h->group.primary();
  std::lock_guard<std::mutex> lock(e.mutex());  // a few values change while the engine runs (persistent_decode, ...)
  auto& m = e.config().ints;
  auto it = m.find(key);
  return it == m.end() ? INT_MIN : (int)it->second;
}

AX_WHISPER_API int AX_WHISPER_PersistentDecodePlan(int d_model, int n_head, int n_layer, int n_cu, int n_clips, int t0, int n_slots,
                                                   int* plan4, int* units) {
  return axw::persistent_decode_plan(d_model, n_head, n_layer, n_cu, n_clips, t0, n_slots, plan4, units);
}

AX_WHISPER_API const char* AX_WHISPER_LastError(AX_WHISPER_HANDLE handle) {
  Handle* h = H(handle);
  if (!h) return g_init_error.c_str();
  // a copy taken under the lock: server threads and device workers may set_error() concurrently, and the pointer handed
  // out must not dangle when they do (valid until this thread's next call)
  thread_local std::string copy;
  {
    std::lock_guard<std::mutex> lk(h->err_mu);
    copy = h->last_error;
  }
  return copy.c_str();
}

AX_WHISPER_API int AX_WHISPER_SetStream(AX_WHISPER_HANDLE handle, void* hip_stream) {
  return guarded(handle, [&](Engine& e) { e.set_stream(hip_stream); });
}

AX_WHISPER_API int AX_WHISPER_ComputeMel(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, float* mel_out) {
  if (!handle || !pcm || !mel_out || num_samples < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.compute_mel(pcm, num_samples, mel_out); });
}

AX_WHISPER_API int AX_WHISPER_EncodeMel(AX_WHISPER_HANDLE handle, const float* mel, int batch) {
  if (!handle || !mel || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.encode_mel(mel, batch); });
}

AX_WHISPER_API int AX_WHISPER_GetCrossKV(AX_WHISPER_HANDLE handle, int slot, float* k_out, float* v_out) {
  if (!handle || !k_out || !v_out) return -1;
  return guarded(handle, [&](Engine& e) { e.get_cross_kv(slot, k_out, v_out); });
}

AX_WHISPER_API int AX_WHISPER_GetCrossKVFp8(AX_WHISPER_HANDLE handle, int slot, uint8_t* k_codes, uint8_t* v_codes, float* scales) {
  if (!handle || !k_codes || !v_codes || !scales) return -1;
  return guarded(handle, [&](Engine& e) { e.get_cross_kv_fp8(slot, k_codes, v_codes, scales); });
}

AX_WHISPER_API int AX_WHISPER_CrossKVQuantize(AX_WHISPER_HANDLE handle) {
  if (!handle) return -1;
  return guarded(handle, [&](Engine& e) { e.cross_kv_quantize(); });
}

AX_WHISPER_API int AX_WHISPER_ScanStored16(AX_WHISPER_HANDLE handle, int batch, int n_max, char* names, int64_t* nonfinite,
                                           float* maxabs, int* n_out) {
  if (!handle || !names || !nonfinite || !maxabs || !n_out || n_max < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    static_assert(sizeof(long long) == sizeof(int64_t), "int64_t");
    *n_out = e.scan_stored16(batch, n_max, reinterpret_cast<char(*)[32]>(names), reinterpret_cast<long long*>(nonfinite), maxabs);
  });
}

AX_WHISPER_API int AX_WHISPER_DecodeForced(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                           float* logits, int32_t* argmax_ids) {
  if (!handle || (n_forced > 0 && !forced)) return -1;
  return guarded(handle, [&](Engine& e) { e.decode_forced(Engine::kDecodePlain, {}, batch, forced, n_forced, logits, argmax_ids, nullptr, nullptr); });
}

AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestamps(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                                     float* logits, int32_t* chosen) {
  if (!handle || (n_forced > 0 && !forced)) return -1;
  return guarded(handle, [&](Engine& e) { e.decode_forced(Engine::kDecodeTimestamps, {}, batch, forced, n_forced, logits, chosen, nullptr, nullptr); });
}

AX_WHISPER_API int AX_WHISPER_ApplyTimestampRules(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                                  int batch, int32_t* chosen) {
  if (!handle || !logits || !hist || !n_hist || !chosen || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.timestamp_rules(logits, hist, n_hist, batch, chosen, nullptr); });
}

// ---- confidence (DESIGN.md "Confidence")
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampScores(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                         int batch, int max_new, const int* max_new_clip, int32_t* ids, int* n_ids,
                                                         float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot) {
  if (!handle || !pcm || !num_samples || !ids || !n_ids || !token_logprob || !avg_logprob || !no_speech_logprob || !ended_eot || batch < 1) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    const Engine::ClipScores scores{token_logprob, avg_logprob, no_speech_logprob, ended_eot};
    run_request(g, timestamp_request(Engine::kDecodeScored, max_new, max_new_clip, &scores), pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampScores(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                                          float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob,
                                                          float* logits0) {
  if (!handle || (n_forced > 0 && !forced)) return -1;
  return guarded(handle, [&](Engine& e) {
    const Engine::ForcedScores scores{logprob, no_speech_logprob, logits0};
    e.decode_forced(Engine::kDecodeScored, {}, batch, forced, n_forced, logits, chosen, &scores, nullptr);
  });
}

AX_WHISPER_API int AX_WHISPER_ScoreTimestampRules(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                                  int batch, int32_t* chosen, float* logprob) {
  if (!handle || !logits || !hist || !n_hist || !chosen || !logprob || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.timestamp_rules(logits, hist, n_hist, batch, chosen, logprob); });
}

AX_WHISPER_API int AX_WHISPER_NoSpeechLogProb(AX_WHISPER_HANDLE handle, const float* logits, int batch, float* out) {
  if (!handle || !logits || !out || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.no_speech_logprob(logits, batch, out); });
}

// ---- beam search (DESIGN.md "Beam search")
AX_WHISPER_API int AX_WHISPER_RunPCMBatchBeam(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                              int beam_size, int max_new, int32_t* ids, int* n_ids, float* sum_logprob,
                                              float* avg_logprob, float* no_speech_logprob, int* ended_eot) {
  if (!handle || !pcm || !num_samples || !ids || !n_ids || !sum_logprob || !avg_logprob || !no_speech_logprob || !ended_eot || batch < 1) return -1;
  for (int b = 0; b < batch; ++b)
    if (!pcm[b] || num_samples[b] < 1) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    const axw::BeamResult out{ids, n_ids, sum_logprob, avg_logprob, ended_eot, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    g.run_beam(pcm, num_samples, batch, beam_size, max_new, g.primary().config().n_text_ctx, out, no_speech_logprob);
  });
}

AX_WHISPER_API int AX_WHISPER_DecodeBeam(AX_WHISPER_HANDLE handle, int batch, int beam_size, int max_new, int32_t* ids, int* n_ids,
                                         float* sum_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot,
                                         int32_t* rec_ids, int* rec_len, float* rec_score, int* rec_pool, int* n_rec, int* winner,
                                         int trace_cap, float* tr_rows, int32_t* tr_cand_id, float* tr_cand_logprob, int* tr_n_cand,
                                         float* tr_S, int* tr_slot, int* tr_src, int32_t* tr_tok, int* tr_pool_n, int* n_steps) {
  if (!handle || !ids || !n_ids || batch < 1 || trace_cap < 0) return -1;
  return guarded(handle, [&](Engine& e) {
    const axw::BeamResult out{ids, n_ids, sum_logprob, avg_logprob, ended_eot, rec_ids, rec_len, rec_score, rec_pool, n_rec, winner};
    Engine::BeamTrace tr{trace_cap, tr_rows, tr_cand_id, tr_cand_logprob, tr_n_cand, tr_S, tr_slot, tr_src, tr_tok, tr_pool_n, 0};
    e.decode_beam(batch, beam_size, max_new, out, no_speech_logprob, &tr);
    if (n_steps) *n_steps = tr.n_steps;
  });
}

AX_WHISPER_API int AX_WHISPER_BeamCandidates(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                             int rows, int n_cand_max, int32_t* cand_id, float* cand_logprob, int* n_cand) {
  if (!handle || !logits || !hist || !n_hist || !cand_id || !cand_logprob || !n_cand || rows < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.beam_candidates(logits, hist, n_hist, rows, n_cand_max, cand_id, cand_logprob, n_cand); });
}

AX_WHISPER_API int AX_WHISPER_BeamSelect(AX_WHISPER_HANDLE handle, int clips, int beam_size, int eot, int n, int stride,
                                         const int32_t* cand_id, const float* cand_logprob, const int* n_cand, const int32_t* hist,
                                         float* S, int* slot, int* pool_n, int32_t* pool_ids, int* pool_len, float* pool_score,
                                         int* complete, int32_t* tok, int* src, float* slot_score, int* n_completed) {
  if (!handle || !cand_id || !cand_logprob || !n_cand || !hist || !S || !slot || !pool_n || !pool_ids || !pool_len || !pool_score || !complete ||
      !tok || !src || !slot_score || !n_completed || clips < 1)
    return -1;
  return guarded(handle, [&](Engine& e) {
    const Engine::BeamSelectIO io{clips, beam_size, eot, n, stride, cand_id, cand_logprob, n_cand, hist, S, slot, pool_n, pool_ids, pool_len,
                                  pool_score, complete, tok, src, slot_score};
    *n_completed = e.beam_select(io);
  });
}

AX_WHISPER_API int AX_WHISPER_BeamFinalize(int clips, int beam_size, int n, int stride, const int32_t* hist, const float* S,
                                           const int* slot, const int* pool_n, const int32_t* pool_ids, const int* pool_len,
                                           const float* pool_score, int32_t* rec_ids, int* rec_len, float* rec_score, int* rec_pool,
                                           int* n_rec, int* winner, int32_t* ids, int* n_ids, float* sum_logprob, float* avg_logprob,
                                           int* ended_eot) {
  if (!hist || !S || !slot || !pool_n || !pool_ids || !pool_len || !pool_score || clips < 1 || beam_size < 1 || beam_size > axw::kBeamSizeMax ||
      n < 0 || n > stride)
    return -1;
  for (int c = 0; c < clips; ++c)
    if (pool_n[c] < 0 || pool_n[c] > beam_size) return -1;
  for (int i = 0; i < clips * beam_size; ++i)
    if (slot[i] < 0 || slot[i] >= clips * beam_size || pool_len[i] < 0 || pool_len[i] > stride) return -1;
  return guarded_host([&] {
    const axw::BeamState st{clips, beam_size, n, stride, hist, S, slot, pool_n, pool_ids, pool_len, pool_score};
    axw::beam_finalize(st, axw::BeamResult{ids, n_ids, sum_logprob, avg_logprob, ended_eot, rec_ids, rec_len, rec_score, rec_pool, n_rec, winner});
    return 0;
  });
}

// Host only: one clip's ids (eot excluded) -> segments (DESIGN.md "Segment timestamps": openai-whisper's single-window split,
// plus the tail rule). Any ids are accepted; the result never exceeds n_max entries.
AX_WHISPER_API int AX_WHISPER_SplitSegments(const int32_t* ids, int n, int timestamp_begin, int eot, float clip_seconds, int n_max,
                                            float* start, float* end, int* tok_begin, int* tok_end, int* n_seg) {
  if ((n > 0 && !ids) || n < 0 || !n_seg || n_max < 0 || (n_max > 0 && (!start || !end || !tok_begin || !tok_end))) return -1;
  *n_seg = 0;
  const int T = timestamp_begin;
  auto ts = [&](int i) { return ids[i] >= T; };
  auto time = [&](int i) { return (float)(ids[i] - T) * 0.02f; };
  int count = 0;
  // [lo, hi): a segment's slice; its text ids are the ids < eot
  auto emit = [&](int lo, int hi, float t0, float t1) {
    int tb = -1, te = -1;
    for (int i = lo; i < hi; ++i)
      if (ids[i] < eot) { if (tb < 0) tb = i; te = i + 1; }
    if (tb < 0 || count >= n_max) return;  // no text: dropped
    start[count] = t0; end[count] = t1; tok_begin[count] = tb; tok_end[count] = te;
    ++count;
  };
  std::vector<int> bounds;
  for (int i = 1; i < n; ++i)
    if (ts(i - 1) && ts(i)) bounds.push_back(i);
  if (!bounds.empty()) {
    if (n >= 2 && ts(n - 1) && !ts(n - 2)) bounds.push_back(n);
    int prev = 0;
    float prev_end = 0.f;
    for (int b : bounds) {
      prev_end = time(b - 1);
      emit(prev, b, time(prev), prev_end);
      prev = b;
    }
    if (prev < n) emit(prev, n, ts(prev) ? time(prev) : prev_end, clip_seconds);  // the tail: one window keeps it
  } else {
    int last = -1;
    for (int i = 0; i < n; ++i)
      if (ts(i)) last = i;
    emit(0, n, 0.f, (last >= 0 && ids[last] != T) ? time(last) : clip_seconds);
  }
  *n_seg = count;
  return 0;
}

// ---- long-form (DESIGN.md "Long-form")
// Host only: the window rule of the seek loop (longform.hpp). Any ids are accepted; at most n_max segments are written.
AX_WHISPER_API int AX_WHISPER_SplitWindow(const int32_t* ids, int n, int timestamp_begin, int eot, int window_frames, int n_max,
                                          float* start, float* end, int* tok_begin, int* tok_end, int* n_seg, int* advance) {
  if ((n > 0 && !ids) || n < 0 || !n_seg || !advance || n_max < 0 || (n_max > 0 && (!start || !end || !tok_begin || !tok_end))) return -1;
  *n_seg = 0;
  *advance = 0;
  try {
    std::vector<axw::WindowSegment> segs;
    *advance = axw::split_window(ids, n, timestamp_begin, eot, window_frames, segs);
    const int count = (int)std::min<size_t>(segs.size(), (size_t)n_max);
    for (int k = 0; k < count; ++k) {
      start[k] = segs[k].start; end[k] = segs[k].end; tok_begin[k] = segs[k].tok_begin; tok_end[k] = segs[k].tok_end;
    }
    *n_seg = count;
    return 0;
  } catch (...) {
    return -1;
  }
}

AX_WHISPER_API int AX_WHISPER_ComputeMelWindow(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, int seek, float* mel_out) {
  if (!handle || !pcm || !mel_out || num_samples < 1 || seek < 0) return -1;
  return guarded(handle, [&](Engine& e) { e.compute_mel_window(pcm, num_samples, seek, mel_out); });
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongWindows(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                int max_new, int max_passes, int win_cap, int* win_info, int32_t* ids, int* n_windows) {
  return long_windows(handle, "RunPCMLongWindows", pcm, num_samples, n_files, max_new, max_passes, axw::long_call_plain(),
                      {win_cap, win_info, ids, nullptr, nullptr, n_windows, nullptr, nullptr});
}

AX_WHISPER_API int AX_WHISPER_RunPCMLong(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, char** result) {
  return long_text(handle, pcm_data, num_samples, axw::long_call_plain(), nullptr, result);
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongOpts(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                             float logprob_threshold, char** result) {
  return long_text(handle, pcm_data, num_samples, axw::long_call_scored(no_speech_threshold, logprob_threshold), nullptr, result);
}

AX_WHISPER_API int AX_WHISPER_RunFileLongOpts(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold,
                                              float logprob_threshold, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) {
    return AX_WHISPER_RunPCMLongOpts(handle, pcm, n, no_speech_threshold, logprob_threshold, result);
  });
}

AX_WHISPER_API int AX_WHISPER_LongWindowIsSilent(float no_speech_logprob, float avg_logprob, float no_speech_threshold,
                                                 float logprob_threshold) {
  return axw::long_window_is_silent(no_speech_logprob, avg_logprob, no_speech_threshold, logprob_threshold) ? 1 : 0;
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsScored(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                      int n_files, int max_new, int max_passes, float no_speech_threshold,
                                                      float logprob_threshold, int win_cap, int* win_info, int32_t* ids, float* win_score,
                                                      int* n_windows) {
  return long_windows(handle, "RunPCMLongWindowsScored", pcm, num_samples, n_files, max_new, max_passes,
                      axw::long_call_scored(no_speech_threshold, logprob_threshold),
                      {win_cap, win_info, ids, win_score, nullptr, n_windows, nullptr, nullptr});
}

// ---- temperature fallback (DESIGN.md "Temperature fallback")
AX_WHISPER_API int AX_WHISPER_SampleTimestampRules(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                                   int batch, const float* temperature, const uint64_t* stream, uint64_t seed,
                                                   int32_t* chosen, float* logprob) {
  if (!handle || !logits || !hist || !n_hist || !temperature || !stream || !chosen || !logprob || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    const Engine::SampleSpec sample{temperature, stream, seed};
    e.timestamp_rules(logits, hist, n_hist, batch, chosen, logprob, &sample);
  });
}

AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampSampled(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                                           const float* temperature, const uint64_t* stream, uint64_t seed,
                                                           float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob,
                                                           float* logits0) {
  if (!handle || (n_forced > 0 && !forced) || !temperature || !stream || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    const Engine::ForcedScores scores{logprob, no_speech_logprob, logits0};
    const Engine::SampleSpec sample{temperature, stream, seed};
    e.decode_forced(Engine::kDecodeSampled, {}, batch, forced, n_forced, logits, chosen, &scores, &sample);
  });
}

AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampSampled(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                          int batch, int max_new, const int* max_new_clip, const float* temperature,
                                                          const uint64_t* stream, uint64_t seed, int32_t* ids, int* n_ids,
                                                          float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot) {
  if (!handle || !pcm || !num_samples || !temperature || !stream || !ids || !n_ids || !token_logprob || !avg_logprob || !no_speech_logprob ||
      !ended_eot || batch < 1)
    return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    const Engine::ClipScores scores{token_logprob, avg_logprob, no_speech_logprob, ended_eot};
    Engine::DecodeRequest rq = timestamp_request(Engine::kDecodeSampled, max_new, max_new_clip, &scores);
    rq.sample = Engine::SampleSpec{temperature, stream, seed};
    run_request(g, rq, pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_CompressionRatio(const unsigned char* bytes, int n, float* ratio) {
  if ((n > 0 && !bytes) || n < 0 || !ratio) return -1;
  return guarded_host([&] {
    *ratio = axw::compression_ratio(bytes, (size_t)n);
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_WindowNeedsFallback(float compression_ratio, float avg_logprob, float no_speech_logprob,
                                                  float compression_ratio_threshold, float logprob_threshold, float no_speech_threshold) {
  return axw::window_needs_fallback(compression_ratio, avg_logprob, no_speech_logprob, compression_ratio_threshold, logprob_threshold,
                                    no_speech_threshold) ? 1 : 0;
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsFallback(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                        int n_files, int max_new, int max_passes, float no_speech_threshold,
                                                        float logprob_threshold, float compression_ratio_threshold,
                                                        const float* temperatures, int n_temperatures, uint64_t seed, const int* file_ids,
                                                        int win_cap, int* win_info, int32_t* ids, float* win_score, int* n_windows) {
  return long_windows(handle, "RunPCMLongWindowsFallback", pcm, num_samples, n_files, max_new, max_passes,
                      axw::long_call_fallback(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, n_temperatures, seed, file_ids),
                      {win_cap, win_info, ids, win_score, nullptr, n_windows, nullptr, nullptr});
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongFallback(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                                 float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                 int n_temperatures, uint64_t seed, char** result) {
  return long_text(handle, pcm_data, num_samples,
                   axw::long_call_fallback(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, n_temperatures, seed, nullptr),
                   nullptr, result);
}

AX_WHISPER_API int AX_WHISPER_RunFileLongFallback(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold,
                                                  float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                  int n_temperatures, uint64_t seed, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) {
    return AX_WHISPER_RunPCMLongFallback(handle, pcm, n, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures,
                                         n_temperatures, seed, result);
  });
}

// ---- prompt conditioning (DESIGN.md "Prompt conditioning")
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampPrompted(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                           int batch, int max_new, const int* max_new_clip, const int32_t* prompt_ids,
                                                           int prompt_stride, const int* n_prompt, int32_t* ids, int* n_ids,
                                                           float* token_logprob, float* avg_logprob, float* no_speech_logprob,
                                                           int* ended_eot) {
  if (!handle || !pcm || !num_samples || !n_prompt || prompt_stride < 0 || (prompt_stride > 0 && !prompt_ids) || !ids || !n_ids || !token_logprob ||
      !avg_logprob || !no_speech_logprob || !ended_eot || batch < 1)
    return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    const Engine::ClipScores scores{token_logprob, avg_logprob, no_speech_logprob, ended_eot};
    Engine::DecodeRequest rq = timestamp_request(Engine::kDecodeScored, max_new, max_new_clip, &scores);
    rq.ctx = clip_contexts(prompt_ids, prompt_stride, n_prompt);
    run_request(g, rq, pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_PrefillPrompts(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids, int prompt_stride,
                                             const int* n_prompt, float* no_speech_logprob, float* sot_logits) {
  if (!handle || !n_prompt || prompt_stride < 0 || (prompt_stride > 0 && !prompt_ids) || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.prefill_stage(batch, clip_contexts(prompt_ids, prompt_stride, n_prompt), no_speech_logprob, sot_logits); });
}

AX_WHISPER_API int AX_WHISPER_GetSelfKV(AX_WHISPER_HANDLE handle, int slot, int n_rows, float* k_out, float* v_out) {
  if (!handle || !k_out || !v_out) return -1;
  return guarded(handle, [&](Engine& e) { e.get_self_kv(slot, n_rows, k_out, v_out); });
}

AX_WHISPER_API int AX_WHISPER_GetPersistentSelfKV(AX_WHISPER_HANDLE handle, int clip, float* k_out, float* v_out) {
  if (!handle || !k_out || !v_out) return -1;
  return guarded(handle, [&](Engine& e) { e.get_persistent_self_kv(clip, k_out, v_out); });
}

AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampPrompted(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids,
                                                            int prompt_stride, const int* n_prompt, const int32_t* forced, int n_forced,
                                                            float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob) {
  if (!handle || !n_prompt || prompt_stride < 1 || !prompt_ids || (n_forced > 0 && !forced) || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    const Engine::ForcedScores scores{logprob, no_speech_logprob, nullptr};
    e.decode_forced(Engine::kDecodeScored, clip_contexts(prompt_ids, prompt_stride, n_prompt), batch, forced, n_forced, logits, chosen, &scores,
                    nullptr);
  });
}

// ---- language and task per clip (DESIGN.md "Language and task per clip")
AX_WHISPER_API int AX_WHISPER_LanguageIndex(AX_WHISPER_HANDLE handle, const char* code) {
  Handle* h = H(handle);
  if (!h || !code || h->group.size() == 0) return -1;
  const auto& codes = h->group.primary().config().lang_codes;  // (fixed at Init)
  const auto it = std::find(codes.begin(), codes.end(), std::string(code));
  return it == codes.end() ? -1 : (int)(it - codes.begin());
}

AX_WHISPER_API const char* AX_WHISPER_LanguageCode(AX_WHISPER_HANDLE handle, int index) {
  Handle* h = H(handle);
  if (!h || h->group.size() == 0) return nullptr;
  const auto& codes = h->group.primary().config().lang_codes;
  return index < 0 || index >= (int)codes.size() ? nullptr : codes[(size_t)index].c_str();
}

AX_WHISPER_API int AX_WHISPER_DetectLanguage(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                             int* lang_out, float* lang_logprob) {
  if (!handle || !pcm || !num_samples || !lang_out || batch < 1) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    Engine::ClipContexts out;
    out.lang_out = {lang_out, lang_logprob, nullptr};
    g.detect_language(pcm, num_samples, batch, (int)g.primary().config().lang_tokens.size(), out);
  });
}

AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampLang(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                                       int max_new, const int* max_new_clip, const int32_t* prompt_ids, int prompt_stride,
                                                       const int* n_prompt, const int* lang, const int* task, int32_t* ids, int* n_ids,
                                                       float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot,
                                                       int* lang_out, float* lang_logprob) {
  if (!handle || !pcm || !num_samples || prompt_stride < 0 || (n_prompt && prompt_stride > 0 && !prompt_ids) || !ids || !n_ids || !token_logprob ||
      !avg_logprob || !no_speech_logprob || !ended_eot || batch < 1)
    return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    const Engine::ClipScores scores{token_logprob, avg_logprob, no_speech_logprob, ended_eot};
    Engine::DecodeRequest rq = timestamp_request(Engine::kDecodeScored, max_new, max_new_clip, &scores);
    rq.ctx = clip_contexts(prompt_ids, prompt_stride, n_prompt, Engine::LangSpec{lang, task}, {lang_out, lang_logprob, nullptr});
    run_request(g, rq, pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_DetectLanguageStage(AX_WHISPER_HANDLE handle, int batch, int* lang_out, float* lang_logprob, float* lang_logit) {
  if (!handle || !lang_out || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.detect_language_stage(batch, Engine::LangResult{lang_out, lang_logprob, lang_logit}); });
}

AX_WHISPER_API int AX_WHISPER_LanguageLogProbRows(AX_WHISPER_HANDLE handle, const float* rows, int n, float* lang_logprob, int* lang_index,
                                                  float* lang_logit) {
  if (!handle || !rows || !lang_logprob || !lang_index || n < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.language_logprob_rows(rows, n, lang_logprob, lang_index, lang_logit); });
}

AX_WHISPER_API int AX_WHISPER_PrefillContexts(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids, int prompt_stride, const int* n_prompt,
                                              const int* lang, const int* task, float* no_speech_logprob, float* sot_logits, int* lang_out,
                                              float* lang_logprob) {
  if (!handle || prompt_stride < 0 || (n_prompt && prompt_stride > 0 && !prompt_ids) || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    e.prefill_stage(batch, clip_contexts(prompt_ids, prompt_stride, n_prompt, Engine::LangSpec{lang, task}, {lang_out, lang_logprob, nullptr}),
                    no_speech_logprob, sot_logits);
  });
}

AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampLang(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids, int prompt_stride,
                                                        const int* n_prompt, const int* lang, const int* task, const int32_t* forced, int n_forced,
                                                        float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob, int* lang_out) {
  if (!handle || prompt_stride < 0 || (n_prompt && prompt_stride > 0 && !prompt_ids) || (n_forced > 0 && !forced) || batch < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    const Engine::ForcedScores scores{logprob, no_speech_logprob, nullptr};
    e.decode_forced(Engine::kDecodeScored, clip_contexts(prompt_ids, prompt_stride, n_prompt, Engine::LangSpec{lang, task}, {lang_out, nullptr, nullptr}),
                    batch, forced, n_forced, logits, chosen, &scores, nullptr);
  });
}

AX_WHISPER_API int AX_WHISPER_CarryPrompt(const int32_t* all_ids, int n_all, int reset_since, const int32_t* window_ids, int n_window,
                                          int timestamp_begin, int eot, int window_frames, int skipped, int condition_on_previous_text,
                                          float temperature, int keep, int cap, int32_t* all_out, int* n_all_out, int* reset_since_out,
                                          int* n_prompt_next) {
  if (n_all < 0 || (n_all > 0 && !all_ids) || n_window < 0 || (n_window > 0 && !window_ids) || reset_since < 0 || reset_since > n_all ||
      window_frames < 0 || keep < 0 || !all_out || !n_all_out || !reset_since_out || !n_prompt_next || cap < n_all + n_window)
    return -1;
  return guarded_host([&] {
    axw::PromptCarry st;
    st.all_ids.assign(all_ids, all_ids + n_all);
    st.reset_since = reset_since;
    axw::carry_prompt(st, window_ids, n_window, timestamp_begin, eot, window_frames, skipped != 0, condition_on_previous_text != 0, temperature);
    std::copy(st.all_ids.begin(), st.all_ids.end(), all_out);
    *n_all_out = (int)st.all_ids.size();
    *reset_since_out = st.reset_since;
    *n_prompt_next = std::min((int)st.all_ids.size() - st.reset_since, keep);
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsPrompted(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                        int n_files, int max_new, int max_passes, float no_speech_threshold,
                                                        float logprob_threshold, float compression_ratio_threshold,
                                                        const float* temperatures, int n_temperatures, uint64_t seed, const int* file_ids,
                                                        const int32_t* initial_prompt_ids, int prompt_stride, const int* n_initial,
                                                        int condition_on_previous_text, int win_cap, int* win_info, int32_t* ids,
                                                        float* win_score, int* win_prompt, int* n_windows) {
  return long_windows(handle, "RunPCMLongWindowsPrompted", pcm, num_samples, n_files, max_new, max_passes,
                      axw::long_call_prompted(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, n_temperatures, seed,
                                              file_ids, initial_prompt_ids, prompt_stride, n_initial, condition_on_previous_text),
                      {win_cap, win_info, ids, win_score, win_prompt, n_windows, nullptr, nullptr});
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongPrompted(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                                 float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                 int n_temperatures, uint64_t seed, const int32_t* initial_prompt_ids, int n_initial,
                                                 int condition_on_previous_text, char** result) {
  return long_text(handle, pcm_data, num_samples,
                   axw::long_call_prompted(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, n_temperatures, seed,
                                           nullptr, initial_prompt_ids, n_initial, &n_initial, condition_on_previous_text),
                   nullptr, result);
}

AX_WHISPER_API int AX_WHISPER_RunFileLongPrompted(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold,
                                                  float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                  int n_temperatures, uint64_t seed, const int32_t* initial_prompt_ids, int n_initial,
                                                  int condition_on_previous_text, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) {
    return AX_WHISPER_RunPCMLongPrompted(handle, pcm, n, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures,
                                         n_temperatures, seed, initial_prompt_ids, n_initial, condition_on_previous_text, result);
  });
}

// ---- long-form under a language and task per file (DESIGN.md "Language and task per clip")
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsLang(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                    int max_new, int max_passes, float no_speech_threshold, float logprob_threshold,
                                                    float compression_ratio_threshold, const float* temperatures, int n_temperatures,
                                                    uint64_t seed, const int* file_ids, const int32_t* initial_prompt_ids, int prompt_stride,
                                                    const int* n_initial, int condition_on_previous_text, const int* lang, const int* task,
                                                    int win_cap, int* win_info, int32_t* ids, float* win_score, int* win_prompt,
                                                    int* n_windows, int* lang_out) {
  return long_windows(handle, "RunPCMLongWindowsLang", pcm, num_samples, n_files, max_new, max_passes,
                      axw::long_call_lang(axw::long_call_prompted(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures,
                                                                  n_temperatures, seed, file_ids, initial_prompt_ids, prompt_stride, n_initial,
                                                                  condition_on_previous_text),
                                          lang, task),
                      {win_cap, win_info, ids, win_score, win_prompt, n_windows, lang_out, nullptr});
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongLang(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                             float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                             int n_temperatures, uint64_t seed, const int32_t* initial_prompt_ids, int n_initial,
                                             int condition_on_previous_text, int lang, int task, int* lang_out, char** result) {
  return long_text(handle, pcm_data, num_samples,
                   axw::long_call_lang(axw::long_call_prompted(no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures,
                                                               n_temperatures, seed, nullptr, initial_prompt_ids, n_initial, &n_initial,
                                                               condition_on_previous_text),
                                       &lang, &task),
                   lang_out, result);
}

AX_WHISPER_API int AX_WHISPER_RunFileLongLang(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold, float logprob_threshold,
                                              float compression_ratio_threshold, const float* temperatures, int n_temperatures, uint64_t seed,
                                              const int32_t* initial_prompt_ids, int n_initial, int condition_on_previous_text, int lang,
                                              int task, int* lang_out, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) {
    return AX_WHISPER_RunPCMLongLang(handle, pcm, n, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, n_temperatures,
                                     seed, initial_prompt_ids, n_initial, condition_on_previous_text, lang, task, lang_out, result);
  });
}

AX_WHISPER_API int AX_WHISPER_RunFileLong(AX_WHISPER_HANDLE handle, const char* wav_file, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) { return AX_WHISPER_RunPCMLong(handle, pcm, n, result); });
}

AX_WHISPER_API int AX_WHISPER_DecodeGreedy(AX_WHISPER_HANDLE handle, int batch, int max_new, int32_t* ids, int* n_ids) {
  return AX_WHISPER_DecodeGreedyRagged(handle, batch, max_new, nullptr, ids, n_ids);
}

AX_WHISPER_API int AX_WHISPER_DecodeGreedyRagged(AX_WHISPER_HANDLE handle, int batch, int max_new, const int* max_new_clip,
                                                 int32_t* ids, int* n_ids) {
  if (!handle || !ids || !n_ids) return -1;
  return guarded(handle, [&](Engine& e) { e.decode_greedy(Engine::kDecodePlain, batch, max_new, max_new_clip, ids, n_ids); });
}

AX_WHISPER_API int AX_WHISPER_StreamOpen(AX_WHISPER_HANDLE handle, int n_slots) {
  return guarded(handle, [&](Engine& e) { e.stream_open(n_slots); });
}
AX_WHISPER_API int AX_WHISPER_StreamAdmit(AX_WHISPER_HANDLE handle, int slot, const float* pcm, int num_samples, int max_new) {
  if (!handle || !pcm || num_samples < 1) return -1;
  return guarded(handle, [&](Engine& e) { const float* arr[1] = {pcm}; e.stream_admit(&slot, arr, &num_samples, &max_new, 1); });
}
AX_WHISPER_API int AX_WHISPER_StreamAdmitBatch(AX_WHISPER_HANDLE handle, const int* slots, const float* const* pcm,
                                               const int* num_samples, const int* max_new, int count) {
  if (!handle || !slots || !pcm || !num_samples || count < 1) return -1;
  for (int i = 0; i < count; ++i) if (!pcm[i] || num_samples[i] < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.stream_admit(slots, pcm, num_samples, max_new, count); });
}
AX_WHISPER_API int AX_WHISPER_StreamStep(AX_WHISPER_HANDLE handle, int n_steps, int* finished_slots, int* n_finished) {
  if (!handle || !finished_slots || !n_finished) return -1;
  *n_finished = 0;
  return guarded(handle, [&](Engine& e) { *n_finished = e.stream_step(n_steps, finished_slots); });
}
AX_WHISPER_API int AX_WHISPER_StreamCollect(AX_WHISPER_HANDLE handle, int slot, int32_t* ids, int* n_ids) {
  if (!handle || !ids || !n_ids) return -1;
  return guarded(handle, [&](Engine& e) { e.stream_collect(slot, ids, n_ids); });
}
AX_WHISPER_API int AX_WHISPER_StreamClose(AX_WHISPER_HANDLE handle) {
  return guarded(handle, [&](Engine& e) { e.stream_close(); });
}

// ---- slot stream in timestamp mode (DESIGN.md "Slot stream in timestamp mode")
AX_WHISPER_API int AX_WHISPER_StreamOpenMode(AX_WHISPER_HANDLE handle, int n_slots, int mode) {
  return guarded(handle, [&](Engine& e) { e.stream_open(n_slots, mode); });
}
AX_WHISPER_API int AX_WHISPER_StreamAdmitBatchLang(AX_WHISPER_HANDLE handle, const int* slots, const float* const* pcm, const int* num_samples,
                                                   const int* rates, const int* max_new, const int* lang, const int* task, int count) {
  if (!handle || !slots || !pcm || !num_samples || count < 1) return -1;
  for (int i = 0; i < count; ++i) if (!pcm[i] || num_samples[i] < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.stream_admit(slots, pcm, num_samples, max_new, count, rates, lang, task); });
}
AX_WHISPER_API int AX_WHISPER_StreamCollectScored(AX_WHISPER_HANDLE handle, int slot, int32_t* ids, int* n_ids, float* token_logprob,
                                                  float* avg_logprob, float* no_speech_logprob, int* ended_eot, int* lang_out,
                                                  float* lang_logprob) {
  if (!handle || !ids || !n_ids) return -1;
  return guarded(handle, [&](Engine& e) {
    e.stream_collect_scored(slot, ids, n_ids, Engine::SlotScores{token_logprob, avg_logprob, no_speech_logprob, ended_eot, lang_out, lang_logprob});
  });
}
AX_WHISPER_API int AX_WHISPER_StreamRulesStage(AX_WHISPER_HANDLE handle, int n, const float* rows, const int* off, const int* done,
                                               const int* detect, const int32_t* hist, const int* n_hist, int* slot_ctx, int32_t* chosen,
                                               float* logprob, float* no_speech, int* lang_out, float* lang_logprob) {
  if (!handle || !rows || !off || !done || !detect || !hist || !n_hist || !slot_ctx || !chosen || !logprob || !no_speech || !lang_out ||
      !lang_logprob || n < 1)
    return -1;
  return guarded(handle, [&](Engine& e) {
    e.stream_rules_stage(Engine::StreamRulesIO{n, rows, off, done, detect, hist, n_hist, slot_ctx, chosen, logprob, no_speech, lang_out, lang_logprob});
  });
}

// ---- word-level timestamps (DESIGN.md "Word-level timestamps")
// Host only: matrix [n_rows][n_frames] (row stride ld floats) -> jump [n_rows] (words.hpp: align_path)
AX_WHISPER_API int AX_WHISPER_AlignPath(const float* matrix, int n_rows, int n_frames, int ld, int* jump) {
  if (!matrix || !jump || n_rows < 1 || n_frames < 1 || ld < n_frames) return -1;
  return guarded_host([&] {
    axw::align_path(matrix, n_rows, n_frames, ld, jump);
    return 0;
  });
}

// words -> the caller's arrays: the texts concatenated into one malloc'ed buffer, word w ending at byte text_end[w]
static int emit_word_text(const std::vector<const std::string*>& words, int* text_end, char** text, int* n_bytes) {
  std::string all;
  for (size_t w = 0; w < words.size(); ++w) {
    all += *words[w];
    text_end[w] = (int)all.size();
  }
  *text = static_cast<char*>(malloc(all.size() + 1));
  if (!*text) return -1;
  memcpy(*text, all.data(), all.size());
  (*text)[all.size()] = 0;
  *n_bytes = (int)all.size();
  return 0;
}

AX_WHISPER_API int AX_WHISPER_SplitWords(const char* tokens_path, const int32_t* ids, int n, int eot, const char* language, int n_max,
                                         int* word_tokens, int* word_text_end, int* n_words, char** text, int* n_bytes) {
  if (!tokens_path || (n > 0 && !ids) || n < 0 || !language || n_max < 0 || (n_max > 0 && (!word_tokens || !word_text_end)) || !n_words || !text || !n_bytes)
    return -1;
  *text = nullptr;
  *n_words = *n_bytes = 0;
  return guarded_host([&] {
    const std::vector<std::string> table = axw::load_token_table(tokens_path);
    const std::vector<axw::WordTokens> words = axw::split_words(table, ids, n, eot, language);
    if ((int)words.size() > n_max) throw std::runtime_error("split_words: more words than n_max");
    for (size_t w = 0; w < words.size(); ++w) word_tokens[w] = (int)words[w].tokens.size();
    *n_words = (int)words.size();
    std::vector<const std::string*> texts;
    for (const axw::WordTokens& w : words) texts.push_back(&w.text);
    return emit_word_text(texts, word_text_end, text, n_bytes);
  });
}

AX_WHISPER_API int AX_WHISPER_WordsFromAlignment(const char* tokens_path, const int32_t* ids, int n, int eot, const char* language,
                                                 const int* seg_tokens, double* seg_start, double* seg_end, int n_seg, const int* jump,
                                                 const float* token_logprob, double last_speech_timestamp, int n_max, int* word_segment,
                                                 int* word_text_end, double* word_start, double* word_end, float* word_prob, int* n_words,
                                                 char** text, int* n_bytes) {
  if (!tokens_path || (n > 0 && (!ids || !token_logprob)) || n < 0 || !language || n_seg < 0 || (n_seg > 0 && (!seg_tokens || !seg_start || !seg_end)) ||
      !jump || n_max < 0 || (n_max > 0 && (!word_segment || !word_text_end || !word_start || !word_end || !word_prob)) || !n_words || !text || !n_bytes)
    return -1;
  *text = nullptr;
  *n_words = *n_bytes = 0;
  return guarded_host([&] {
    const std::vector<std::string> table = axw::load_token_table(tokens_path);
    const std::vector<axw::WordOut> words =
        axw::words_from_alignment(table, ids, n, eot, language, seg_tokens, seg_start, seg_end, n_seg, jump, token_logprob, last_speech_timestamp);
    if ((int)words.size() > n_max) throw std::runtime_error("words_from_alignment: more words than n_max");
    for (size_t w = 0; w < words.size(); ++w) {
      word_segment[w] = words[w].segment; word_start[w] = words[w].start; word_end[w] = words[w].end; word_prob[w] = (float)words[w].probability;
    }
    *n_words = (int)words.size();
    std::vector<const std::string*> texts;
    for (const axw::WordOut& w : words) texts.push_back(&w.text);
    return emit_word_text(texts, word_text_end, text, n_bytes);
  });
}

AX_WHISPER_API int AX_WHISPER_WordsFromAlignmentAt(const char* tokens_path, const int32_t* ids, int n, int eot, const char* language,
                                                   const int* seg_tokens, double* seg_start, double* seg_end, int n_seg, const int* jump,
                                                   const float* token_logprob, double last_speech_timestamp, double time_offset, int n_max,
                                                   int* word_segment, int* word_text_end, double* word_start, double* word_end,
                                                   float* word_prob, int* n_words, char** text, int* n_bytes) {
  if (!tokens_path || (n > 0 && (!ids || !token_logprob)) || n < 0 || !language || n_seg < 0 || (n_seg > 0 && (!seg_tokens || !seg_start || !seg_end)) ||
      !jump || n_max < 0 || (n_max > 0 && (!word_segment || !word_text_end || !word_start || !word_end || !word_prob)) || !n_words || !text || !n_bytes)
    return -1;
  *text = nullptr;
  *n_words = *n_bytes = 0;
  return guarded_host([&] {
    const std::vector<std::string> table = axw::load_token_table(tokens_path);
    const std::vector<axw::WordOut> words = axw::words_from_alignment(table, ids, n, eot, language, seg_tokens, seg_start, seg_end, n_seg, jump,
                                                                      token_logprob, last_speech_timestamp, time_offset);
    if ((int)words.size() > n_max) throw std::runtime_error("words_from_alignment: more words than n_max");
    for (size_t w = 0; w < words.size(); ++w) {
      word_segment[w] = words[w].segment; word_start[w] = words[w].start; word_end[w] = words[w].end; word_prob[w] = (float)words[w].probability;
    }
    *n_words = (int)words.size();
    std::vector<const std::string*> texts;
    for (const axw::WordOut& w : words) texts.push_back(&w.text);
    return emit_word_text(texts, word_text_end, text, n_bytes);
  });
}

// ---- word timestamps in long-form (DESIGN.md "Word-level timestamps": words in the seek loop)
AX_WHISPER_API int AX_WHISPER_LongWordAdvance(const int32_t* ids, int n, int timestamp_begin, int seek, int window_frames, int split_advance,
                                              int has_word, double last_word_end, int* advance, int* by_word_end) {
  if (n < 0 || (n > 0 && !ids) || seek < 0 || window_frames < 0 || !advance) return -1;
  bool by = false;
  *advance = axw::long_word_advance(ids, n, timestamp_begin, seek, window_frames, split_advance, has_word != 0, last_word_end, &by);
  if (by_word_end) *by_word_end = by ? 1 : 0;
  return 0;
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsWords(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                     int max_new, int max_passes, const AX_WHISPER_LONG_OPTIONS* o, int win_cap, int* win_info,
                                                     int32_t* ids, float* win_score, int* win_prompt, int* n_windows, int* lang_out,
                                                     AX_WHISPER_LONG_WORD_LOG* words) {
  return long_windows(handle, "RunPCMLongWindowsWords", pcm, num_samples, n_files, max_new, max_passes, axw::long_call_options(o, false),
                      {win_cap, win_info, ids, win_score, win_prompt, n_windows, lang_out, words});
}

// one file's log -> its segments and words; the arrays are malloc'ed into out
static void long_words_result(Engine& e, const std::vector<axw::LongWindow>& log, int lang_index, AX_WHISPER_LONG_WORDS* out) {
  const int T = (int)e.config().ints.at("timestamp_begin"), E = e.config().eot;
  std::vector<double> ss, se, ws, we;
  std::vector<int> s_end, w_seg, w_end;
  std::vector<float> wp;
  std::string s_text, w_text;
  std::vector<axw::WindowSegment> segs;
  for (const axw::LongWindow& w : log) {
    if (w.skipped || !w.kept) continue;
    axw::split_window(w.ids.data(), (int)w.ids.size(), T, E, w.window_frames, segs);
    const int base = (int)ss.size();
    for (size_t k = 0; k < segs.size(); ++k) {
      ss.push_back(k < w.seg_start.size() ? w.seg_start[k] : (double)w.seek / 100.0 + segs[k].start);
      se.push_back(k < w.seg_end.size() ? w.seg_end[k] : (double)w.seek / 100.0 + segs[k].end);
      s_text += e.transcript_lang(w.ids.data() + segs[k].tok_begin, segs[k].tok_end - segs[k].tok_begin, lang_index);
      s_end.push_back((int)s_text.size());
    }
    for (const axw::LongWord& x : w.words) {
      w_seg.push_back(base + x.segment); ws.push_back(x.start); we.push_back(x.end); wp.push_back(x.probability);
      w_text += x.text;
      w_end.push_back((int)w_text.size());
    }
  }
  auto dup = [](const auto& v) {
    using V = typename std::decay<decltype(v[0])>::type;
    V* p = static_cast<V*>(malloc(std::max<size_t>(v.size(), 1) * sizeof(V)));
    if (!p) throw std::runtime_error("long words: out of memory");
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(V));
    return p;
  };
  out->n_segments = (int)ss.size(); out->n_words = (int)ws.size();
  out->seg_start = dup(ss); out->seg_end = dup(se); out->seg_text_end = dup(s_end); out->seg_text = strdup(s_text.c_str());
  out->word_segment = dup(w_seg); out->word_start = dup(ws); out->word_end = dup(we); out->word_prob = dup(wp); out->word_text_end = dup(w_end);
  out->word_text = static_cast<char*>(malloc(w_text.size() + 1));
  if (!out->seg_text || !out->word_text) throw std::runtime_error("long words: out of memory");
  memcpy(out->word_text, w_text.data(), w_text.size());
  out->word_text[w_text.size()] = 0;
}

AX_WHISPER_API void AX_WHISPER_FreeLongWords(AX_WHISPER_LONG_WORDS* out) {
  if (!out) return;
  free(out->seg_start); free(out->seg_end); free(out->seg_text_end); free(out->seg_text);
  free(out->word_segment); free(out->word_start); free(out->word_end); free(out->word_prob); free(out->word_text_end); free(out->word_text);
  *out = AX_WHISPER_LONG_WORDS{};
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongWords(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, const AX_WHISPER_LONG_OPTIONS* o,
                                              int* lang_out, AX_WHISPER_LONG_WORDS* out) {
  if (!handle || !pcm_data || num_samples < 1 || !out) return -1;
  *out = AX_WHISPER_LONG_WORDS{};
  axw::LongRun run;
  if (!axw::long_run_options(axw::long_call_options(o, true), 1, nullptr, run)) return -1;
  const int rc = guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    std::vector<axw::LongWindow> log;
    const float* files[1] = {pcm_data};
    g.run_long_windows(files, &num_samples, 1, 0, 0, run.get(), log);
    long_words_result(g.primary(), log, run.lang[0], out);
  });
  if (rc != 0) AX_WHISPER_FreeLongWords(out);
  if (rc == 0 && lang_out) *lang_out = run.lang[0];
  return rc;
}

AX_WHISPER_API int AX_WHISPER_RunFileLongWords(AX_WHISPER_HANDLE handle, const char* wav_file, const AX_WHISPER_LONG_OPTIONS* o, int* lang_out,
                                               AX_WHISPER_LONG_WORDS* out) {
  return run_wav(handle, wav_file, out, [&](float* pcm, int n) { return AX_WHISPER_RunPCMLongWords(handle, pcm, n, o, lang_out, out); });
}

// Host only: the alignment heads a handle constructed from this config file starts with
AX_WHISPER_API int AX_WHISPER_ConfigAlignmentHeads(const char* config_path, int n_max, int* pairs, int* n) {
  if (!config_path || !n || n_max < 0 || (n_max > 0 && !pairs)) return -1;
  *n = 0;
  return guarded_host([&] {
    const axw::JsonValue j = axw::JsonParser(axw::read_text_file(config_path)).parse();
    const int n_layer = (int)j.at("n_text_layer").as_int();
    const int n_head = j.has("n_text_head") ? (int)j.at("n_text_head").as_int() : (int)j.at("n_text_state").as_int() / 64;
    std::vector<std::pair<int, int>> v = axw::config_alignment_heads(j, n_layer, n_head);
    if (v.empty()) v = axw::default_alignment_heads(n_layer, n_head);
    if ((int)v.size() > n_max) throw std::runtime_error("config_alignment_heads: more heads than n_max");
    for (size_t i = 0; i < v.size(); ++i) { pairs[2 * i] = v[i].first; pairs[2 * i + 1] = v[i].second; }
    *n = (int)v.size();
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_SetAlignmentHeads(AX_WHISPER_HANDLE handle, const int* pairs, int n) {
  if (!handle || n < 0 || (n > 0 && !pairs)) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    for (int i = 0; i < g.size(); ++i) {
      Engine& e = g.at(i);
      std::lock_guard<std::mutex> lock(e.mutex());
      e.set_alignment_heads(pairs, n);
    }
  });
}

// ---- token suppression (DESIGN.md "Token suppression"; suppress.hpp)
static int copy_ids_out(const std::vector<int>& v, int n_max, int* ids, int* n, const char* what) {
  if ((int)v.size() > n_max) throw std::runtime_error(std::string(what) + ": more ids than n_max");
  for (size_t i = 0; i < v.size(); ++i) ids[i] = v[i];
  *n = (int)v.size();
  return 0;
}

AX_WHISPER_API int AX_WHISPER_SetSuppressTokens(AX_WHISPER_HANDLE handle, const int* ids, int n) {
  if (!handle || n < 0 || (n > 0 && !ids)) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    // every engine gets the set or none does: all of them held, the list checked once and every refusal asked for before the first install
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < g.size(); ++i) locks.emplace_back(g.at(i).mutex());
    const axw::ModelConfig& c = g.primary().config();
    if (n > 0) (void)axw::checked_suppress_tokens(ids, n, c.n_vocab, c.eot, c.no_timestamps + 1, "set_suppress_tokens");
    for (int i = 0; i < g.size(); ++i) {
      const auto it = g.at(i).config().ints.find("stream_slots");
      if (it != g.at(i).config().ints.end() && it->second > 0)
        throw std::runtime_error("set_suppress_tokens: not while a stream is open (engine " + std::to_string(i) + "); the stream's captured step has made its choice");
    }
    for (int i = 0; i < g.size(); ++i) g.at(i).set_suppress_tokens(ids, n);
  });
}

AX_WHISPER_API int AX_WHISPER_GetSuppressTokens(AX_WHISPER_HANDLE handle, int n_max, int* ids, int* n) {
  if (!handle || !n || n_max < 0 || (n_max > 0 && !ids)) return -1;
  *n = 0;
  return guarded(handle, [&](Engine& e) { copy_ids_out(e.suppress_tokens(), n_max, ids, n, "get_suppress_tokens"); });
}

// Host only: the list that suppress_tokens = -1 stands for, derived from a tokens file
AX_WHISPER_API int AX_WHISPER_NonSpeechTokens(const char* tokens_path, int n_max, int* ids, int* n) {
  if (!tokens_path || !n || n_max < 0 || (n_max > 0 && !ids)) return -1;
  *n = 0;
  return guarded_host([&] { return copy_ids_out(axw::non_speech_tokens(axw::load_token_table(tokens_path)), n_max, ids, n, "non_speech_tokens"); });
}

// Host only: the suppress set a handle constructed from this config file starts with (tokens_path: read only for a -1 entry)
AX_WHISPER_API int AX_WHISPER_ConfigSuppressTokens(const char* config_path, const char* tokens_path, int n_max, int* ids, int* n) {
  if (!config_path || !n || n_max < 0 || (n_max > 0 && !ids)) return -1;
  *n = 0;
  return guarded_host([&] {
    const axw::JsonValue j = axw::JsonParser(axw::read_text_file(config_path)).parse();
    const int no_ts = (int)j.at("no_timestamps").as_int();
    const std::vector<int> v = axw::config_suppress_tokens(j, (int)j.at("n_vocab").as_int(), (int)j.at("eot").as_int(), no_ts + 1, [&] {
      if (!tokens_path) throw std::runtime_error("config_suppress_tokens: the list holds -1 and no tokens file was given");
      return axw::load_token_table(tokens_path);
    });
    return copy_ids_out(v, n_max, ids, n, "config_suppress_tokens");
  });
}

AX_WHISPER_API int AX_WHISPER_AlignTokens(AX_WHISPER_HANDLE handle, int batch, const int32_t* ids, int stride, const int* n_ids,
                                          const int* num_frames, const int* lang, const int* task, int* jump, float* token_logprob,
                                          float* matrix, int m_rows, int m_ld) {
  if (!handle || !ids || !n_ids || !num_frames || !jump || !token_logprob || batch < 1 || stride < 1) return -1;
  return guarded(handle, [&](Engine& e) {
    e.align_tokens(Engine::AlignRequest{batch, ids, stride, n_ids, num_frames, lang, task, jump, token_logprob, matrix, m_rows, m_ld});
  });
}

AX_WHISPER_API int AX_WHISPER_VocabLogProbRows(AX_WHISPER_HANDLE handle, const float* x, int n_rows, const int32_t* ids, float* out, int route) {
  if (!handle || !x || !ids || !out || n_rows < 1 || (route != 0 && route != 1)) return -1;
  return guarded(handle, [&](Engine& e) { e.vocab_logprob_rows(x, n_rows, ids, out, route); });
}

AX_WHISPER_API int AX_WHISPER_VocabLogProbPlan(int d_model, int n_rows, int eot, int* plan3) {
  if (!plan3) return -1;
  return axw::vocab_logprob_plan(d_model, n_rows, eot, plan3, plan3 + 1, plan3 + 2) ? 0 : -1;
}

AX_WHISPER_API int AX_WHISPER_AlignQKSoftmax(AX_WHISPER_HANDLE handle, int n_clips, const int* len, const int* n_keys, const float* q, int rows,
                                             int n_head, const int* row0, const float* k, int n_slots, int keys_pad, const int* slot,
                                             const int* heads, int n_align, float* P, int rows_pad, int f_pad) {
  if (!handle || !len || !n_keys || !q || !row0 || !k || !slot || !heads || !P) return -1;
  return guarded(handle, [&](Engine& e) {
    Engine::AlignKernelIO io{};
    io.n_clips = n_clips; io.len = len; io.n_keys = n_keys; io.q = q; io.rows = rows; io.n_head = n_head; io.row0 = row0;
    io.k = k; io.n_slots = n_slots; io.keys_pad = keys_pad; io.slot = slot; io.heads = heads; io.n_align = n_align;
    io.P = P; io.rows_pad = rows_pad; io.f_pad = f_pad;
    e.align_kernel(0, io);
  });
}

AX_WHISPER_API int AX_WHISPER_AlignNormalize(AX_WHISPER_HANDLE handle, int n_clips, const int* len, const int* n_keys, const float* P, int n_align,
                                             int rows_pad, int f_pad, float inv_heads, float* matrix, int m_rows, int m_ld) {
  if (!handle || !len || !n_keys || !P || !matrix) return -1;
  return guarded(handle, [&](Engine& e) {
    Engine::AlignKernelIO io{};
    io.n_clips = n_clips; io.len = len; io.n_keys = n_keys; io.n_align = n_align;
    io.P = const_cast<float*>(P); io.rows_pad = rows_pad; io.f_pad = f_pad; io.matrix = matrix; io.m_rows = m_rows; io.m_ld = m_ld; io.inv_heads = inv_heads;
    e.align_kernel(1, io);
  });
}

AX_WHISPER_API int AX_WHISPER_AlignDTW(AX_WHISPER_HANDLE handle, int n_clips, const int* len, const int* n_keys, const float* matrix, int m_rows,
                                       int m_ld, int* jump, int jump_ld) {
  if (!handle || !len || !n_keys || !matrix || !jump) return -1;
  return guarded(handle, [&](Engine& e) {
    Engine::AlignKernelIO io{};
    io.n_clips = n_clips; io.len = len; io.n_keys = n_keys;
    io.matrix = const_cast<float*>(matrix); io.m_rows = m_rows; io.m_ld = m_ld; io.jump = jump; io.jump_ld = jump_ld;
    e.align_kernel(2, io);
  });
}

// Clips in: the greedy timestamp decode of every clip (under its own language and task when given), the alignment of its text ids on
// the engine that decoded it, and the host rule (words.hpp) on the result.
AX_WHISPER_API int AX_WHISPER_RunPCMBatchWordTimestamps(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                                        int max_new, const int* lang, const int* task, int32_t* ids, int* n_ids, int* lang_out,
                                                        int n_max, int* n_segments, double* seg_start, double* seg_end, int* n_words,
                                                        int* word_segment, int* word_text_end, double* word_start, double* word_end,
                                                        float* word_prob, char** text, int* jump, float* token_logprob) {
  if (!handle || !pcm || !num_samples || !ids || !n_ids || batch < 1 || n_max < 1 || !n_segments || !seg_start || !seg_end || !n_words ||
      !word_segment || !word_text_end || !word_start || !word_end || !word_prob || !text)
    return -1;
  for (int b = 0; b < batch; ++b) {
    if (!pcm[b] || num_samples[b] < 1) return -1;
    text[b] = nullptr;
  }
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    const auto& cfg = g.primary().config();
    const int Tc = cfg.n_text_ctx, T = cfg.no_timestamps + 1, eot = cfg.eot;
    const bool per_lang = lang || task;
    std::vector<int> detected(batch, -1);
    Engine::DecodeRequest rq = timestamp_request(Engine::kDecodeTimestamps, max_new, nullptr, nullptr);
    if (per_lang) rq.ctx = clip_contexts(nullptr, 0, nullptr, Engine::LangSpec{lang, task}, {detected.data(), nullptr, nullptr});
    struct ClipText { std::vector<int32_t> text; std::vector<int> seg_tokens; std::vector<double> st, en; std::vector<int> jump; std::vector<float> lp; };
    std::vector<ClipText> clip(batch);
    g.run_tokens_then(rq, pcm, num_samples, batch, Tc, (int)cfg.lang_tokens.size(), ids, n_ids, [&](Engine& e, int lo, int hi) {
      const int nb = hi - lo;
      std::vector<int32_t> tids((size_t)nb * Tc, 0);
      std::vector<int> tn(nb, 0), frames(nb), jmp((size_t)nb * (Tc + 1), 0);
      std::vector<float> lp((size_t)nb * Tc, 0.f);
      for (int b = lo; b < hi; ++b) {
        ClipText& c = clip[b];
        const int n = n_ids[b], cap = n / 2 + 1;
        const int32_t* row = ids + (size_t)b * Tc;
        std::vector<float> st(cap), en(cap);
        std::vector<int> tb(cap), te(cap);
        int n_seg = 0;
        const float clip_s = num_samples[b] / 16000.f < 30.f ? num_samples[b] / 16000.f : 30.f;
        if (AX_WHISPER_SplitSegments(row, n, T, eot, clip_s, cap, st.data(), en.data(), tb.data(), te.data(), &n_seg) != 0)
          throw std::runtime_error("word timestamps: the segment split failed");
        for (int k = 0; k < n_seg; ++k) {
          int count = 0;
          for (int i = tb[k]; i < te[k]; ++i)
            if (row[i] < eot) { c.text.push_back(row[i]); ++count; }
          c.seg_tokens.push_back(count); c.st.push_back(st[k]); c.en.push_back(en[k]);
        }
        if ((int)c.text.size() + 5 > Tc) c.text.resize(Tc - 5);  // (a decode never keeps that many ids; the alignment's bound)
        tn[b - lo] = (int)c.text.size();
        std::copy(c.text.begin(), c.text.end(), tids.begin() + (size_t)(b - lo) * Tc);
        frames[b - lo] = std::min(num_samples[b] / 160, 3000);
      }
      std::vector<int> lg(nb, -1);
      for (int b = lo; per_lang && b < hi; ++b) lg[b - lo] = detected[b];
      e.align_tokens(Engine::AlignRequest{nb, tids.data(), Tc, tn.data(), frames.data(), lg.data(), task ? task + lo : nullptr, jmp.data(), lp.data(),
                                          nullptr, 0, 0});
      for (int b = lo; b < hi; ++b) {
        clip[b].jump.assign(jmp.begin() + (size_t)(b - lo) * (Tc + 1), jmp.begin() + (size_t)(b - lo) * (Tc + 1) + tn[b - lo] + 1);
        clip[b].lp.assign(lp.begin() + (size_t)(b - lo) * Tc, lp.begin() + (size_t)(b - lo) * Tc + tn[b - lo]);
      }
    });
    const std::vector<std::string>& table = g.primary().token_table();
    for (int b = 0; b < batch; ++b) {
      ClipText& c = clip[b];
      const int li = per_lang ? detected[b] : (int)cfg.ints.at("lang_index");
      const std::string code = li >= 0 && li < (int)cfg.lang_codes.size() ? cfg.lang_codes[(size_t)li] : std::string();
      const int n = (int)c.text.size(), n_seg = (int)c.seg_tokens.size();
      int total = 0;
      for (int& t : c.seg_tokens) { t = std::min(t, n - total); total += t; }
      const std::vector<axw::WordOut> words = axw::words_from_alignment(table, c.text.data(), n, eot, code, c.seg_tokens.data(), c.st.data(), c.en.data(),
                                                                        n_seg, c.jump.data(), c.lp.data(), 0.0);
      if ((int)words.size() > n_max || n_seg > n_max) throw std::runtime_error("word timestamps: more words or segments than n_max");
      n_segments[b] = n_seg;
      for (int k = 0; k < n_seg; ++k) { seg_start[(size_t)b * n_max + k] = c.st[k]; seg_end[(size_t)b * n_max + k] = c.en[k]; }
      const size_t o = (size_t)b * n_max;
      for (size_t w = 0; w < words.size(); ++w) {
        word_segment[o + w] = words[w].segment; word_start[o + w] = words[w].start; word_end[o + w] = words[w].end; word_prob[o + w] = (float)words[w].probability;
      }
      n_words[b] = (int)words.size();
      int n_bytes = 0;
      std::vector<const std::string*> texts;
      for (const axw::WordOut& w : words) texts.push_back(&w.text);
      if (emit_word_text(texts, word_text_end + o, text + b, &n_bytes) != 0)
        throw std::runtime_error("word timestamps: out of memory");
      if (lang_out) lang_out[b] = li;
      if (jump) std::copy(c.jump.begin(), c.jump.end(), jump + (size_t)b * Tc);
      if (token_logprob) std::copy(c.lp.begin(), c.lp.end(), token_logprob + (size_t)b * Tc);
    }
  });
}

// ---- audio at any sample rate (DESIGN.md "Sample rates")
AX_WHISPER_API long long AX_WHISPER_ResampledLength(long long n, int rate) {
  std::string err;
  const long long r = axw::resample::resampled_length(n, rate, err);
  if (r < 0) g_init_error = err;
  return r;
}

AX_WHISPER_API int AX_WHISPER_ResampleFilter(int rate, int* L, int* M, int* K, float* table, int cap) {
  if (!L || !M || !K) return -1;
  return guarded_host([&] {
    axw::resample::Filter f;
    std::string err;
    if (!axw::resample::plan(rate, f, err)) { g_init_error = err; return -1; }
    *L = f.L; *M = f.M; *K = f.K;
    if (!table) return 0;
    if ((long long)cap < f.entries()) { g_init_error = "ResampleFilter: the table has " + std::to_string(f.entries()) + " entries"; return -1; }
    axw::resample::build_table(f, table);
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_ResampleBatch(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, const int* rates,
                                            int batch, float* const* out, const int* out_cap, int* n_out) {
  if (!handle || !pcm || !num_samples || !rates || !out || !out_cap || !n_out || batch < 1) return -1;
  for (int b = 0; b < batch; ++b) if (!pcm[b] || !out[b]) return -1;
  return guarded(handle, [&](Engine& e) { e.resample(pcm, num_samples, rates, batch, out, out_cap, n_out); });
}

AX_WHISPER_API int AX_WHISPER_ComputeMelRate(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, int rate, float* mel_out) {
  if (!handle || !pcm || !mel_out || num_samples < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.compute_mel(pcm, num_samples, mel_out, rate); });
}

AX_WHISPER_API int AX_WHISPER_RunPCMBatchRate(AX_WHISPER_HANDLE handle, int mode, const float* const* pcm, const int* num_samples,
                                              const int* rates, int batch, int max_new, int32_t* ids, int* n_ids) {
  if (!handle || !pcm || !num_samples || !rates || !ids || !n_ids || batch < 1 || (mode != 0 && mode != 1)) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    // refused rates and lengths fail here for the whole batch, before any device starts on its block
    for (int b = 0; b < batch; ++b) {
      std::string err;
      if (axw::resample::resampled_length(num_samples[b], rates[b], err) < 0) throw std::runtime_error("clip " + std::to_string(b) + ": " + err);
    }
    Engine::DecodeRequest rq;
    rq.mode = mode ? Engine::kDecodeTimestamps : Engine::kDecodePlain;
    rq.max_new = max_new; rq.sample_rate = rates;
    run_request(g, rq, pcm, num_samples, batch, ids, n_ids);
  });
}

AX_WHISPER_API int AX_WHISPER_StreamAdmitBatchRate(AX_WHISPER_HANDLE handle, const int* slots, const float* const* pcm,
                                                   const int* num_samples, const int* rates, const int* max_new, int count) {
  if (!handle || !slots || !pcm || !num_samples || count < 1) return -1;
  for (int i = 0; i < count; ++i) if (!pcm[i] || num_samples[i] < 1) return -1;
  return guarded(handle, [&](Engine& e) { e.stream_admit(slots, pcm, num_samples, max_new, count, rates); });
}

// file decode + the stage-level resample call on the primary engine: the file's samples at 16 kHz (its own at 16000 Hz)
static int load_file_16k(AX_WHISPER_HANDLE handle, const char* path, std::vector<float>& pcm16, axw::WavData& wav) {
  std::string err;
  if (!axw::load_audio_file(path, wav, err)) {
    H(handle)->set_error("load wav failed: " + err);
    fprintf(stderr, "[ax_whisper] load wav failed: %s\n", err.c_str());
    return -1;
  }
  if (wav.mono.empty()) { H(handle)->set_error("wav file holds no samples"); return -1; }
  if (wav.sample_rate == axw::resample::kTargetRate) { pcm16 = wav.mono; return 0; }
  const long long n16 = AX_WHISPER_ResampledLength((long long)wav.mono.size(), wav.sample_rate);
  if (n16 < 0) { H(handle)->set_error(std::string(path) + ": " + g_init_error); return -1; }
  pcm16.resize((size_t)n16);
  const float* in = wav.mono.data();
  float* out = pcm16.data();
  const int n = (int)wav.mono.size(), cap = (int)n16;
  int n_out = 0;
  return AX_WHISPER_ResampleBatch(handle, &in, &n, &wav.sample_rate, 1, &out, &cap, &n_out);
}

AX_WHISPER_API int AX_WHISPER_RunFileResampled(AX_WHISPER_HANDLE handle, const char* wav_file, char** result) {
  if (!handle || !wav_file || !result) return -1;
  *result = nullptr;
  std::vector<float> pcm16;
  axw::WavData wav;
  if (load_file_16k(handle, wav_file, pcm16, wav) != 0) return -1;
  return AX_WHISPER_RunPCM(handle, pcm16.data(), (int)pcm16.size(), result);
}

AX_WHISPER_API int AX_WHISPER_LoadAudioFile16k(AX_WHISPER_HANDLE handle, const char* path, float** samples, int* n_samples, int* info) {
  if (!handle || !path || !samples || !n_samples) return -1;
  *samples = nullptr;
  *n_samples = 0;
  std::vector<float> pcm16;
  axw::WavData wav;
  if (load_file_16k(handle, path, pcm16, wav) != 0) return -1;
  *samples = static_cast<float*>(malloc(std::max<size_t>(pcm16.size(), 1) * sizeof(float)));
  if (!*samples) return -1;
  memcpy(*samples, pcm16.data(), pcm16.size() * sizeof(float));
  *n_samples = (int)pcm16.size();
  if (info) { info[0] = wav.sample_rate; info[1] = wav.channels; info[2] = (int)wav.mono.size(); }
  return 0;
}

// ---- chunked long-form (DESIGN.md "Chunked long-form"; long_cuts.hpp)
AX_WHISPER_API int AX_WHISPER_LongCutPlanHost(const float* s, int content, int min_frames, int max_frames, int win_cap, int* seek, int* len,
                                              int* n_windows) {
  if (!n_windows || content < 0 || (content > 0 && !s) || win_cap < 0 || (win_cap > 0 && (!seek || !len))) return -1;
  *n_windows = 0;
  return guarded_host([&] {
    const std::vector<axw::CutWindow> plan = axw::cut_plan(s, content, min_frames, max_frames);
    if ((long)plan.size() > win_cap) throw std::runtime_error(std::to_string(plan.size()) + " windows were planned, win_cap is " + std::to_string(win_cap));
    for (size_t k = 0; k < plan.size(); ++k) { seek[k] = plan[k].seek; len[k] = plan[k].len; }
    *n_windows = (int)plan.size();
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_ChunkedSegments(const int32_t* ids, int n, int timestamp_begin, int eot, int seek, int len, int n_max, double* start,
                                              double* end, int* tok_begin, int* tok_end, int* n_seg) {
  if ((n > 0 && !ids) || n < 0 || !n_seg || seek < 0 || len < 0 || len > axw::kCutMaxFrames || n_max < 0 ||
      (n_max > 0 && (!start || !end || !tok_begin || !tok_end)))
    return -1;
  *n_seg = 0;
  return guarded_host([&] {
    const std::vector<axw::ChunkSegment> segs = axw::chunked_segments(ids, n, timestamp_begin, eot, seek, len);
    const int count = (int)std::min<size_t>(segs.size(), (size_t)n_max);
    for (int k = 0; k < count; ++k) { start[k] = segs[k].start; end[k] = segs[k].end; tok_begin[k] = segs[k].tok_begin; tok_end[k] = segs[k].tok_end; }
    *n_seg = count;
    return 0;
  });
}

AX_WHISPER_API int AX_WHISPER_LongFrameLevels(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                              int smooth_frames, float* const* e, float* const* s) {
  if (!handle || !axw::long_files_ok(pcm, num_samples, n_files)) return -1;
  return guarded(handle, [&](Engine& en) { en.long_frame_levels(pcm, num_samples, n_files, smooth_frames, e, s); });
}

AX_WHISPER_API int AX_WHISPER_LongCutPlanFromLevels(AX_WHISPER_HANDLE handle, const float* s, int content, int min_frames, int max_frames,
                                                    int win_cap, int* seek, int* len, int* n_windows) {
  if (!handle || !s || content < 1 || !n_windows || win_cap < 0 || (win_cap > 0 && (!seek || !len))) return -1;
  *n_windows = 0;
  return guarded(handle, [&](Engine& e) {
    std::vector<axw::CutWindow> plan;
    e.long_cut_plan_from_levels(s, content, min_frames, max_frames, plan);
    if ((long)plan.size() > win_cap) throw std::runtime_error(std::to_string(plan.size()) + " windows were planned, win_cap is " + std::to_string(win_cap));
    for (size_t k = 0; k < plan.size(); ++k) { seek[k] = plan[k].seek; len[k] = plan[k].len; }
    *n_windows = (int)plan.size();
  });
}

static axw::CutParams cut_params(const AX_WHISPER_CHUNK_OPTIONS* c) {
  axw::CutParams p;
  if (c) { p.w_max = c->max_frames; p.w_min = c->min_frames; p.smooth = c->smooth_frames; }
  return p;
}

AX_WHISPER_API int AX_WHISPER_LongCutPlan(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                          const AX_WHISPER_CHUNK_OPTIONS* chunk, int win_cap, int* n_windows, int* win_file, int* win_seek,
                                          int* win_len, float* const* s) {
  if (!handle || !axw::long_files_ok(pcm, num_samples, n_files) || !n_windows || win_cap < 0 || (win_cap > 0 && (!win_file || !win_seek || !win_len))) return -1;
  return guarded(handle, [&](Engine& e) {
    std::vector<int> n, wf, ws, wl;
    e.long_cut_plan(pcm, num_samples, n_files, cut_params(chunk), n, wf, ws, wl, s);
    if ((long)wf.size() > win_cap) throw std::runtime_error(std::to_string(wf.size()) + " windows were planned, win_cap is " + std::to_string(win_cap));
    std::copy(n.begin(), n.end(), n_windows);
    std::copy(wf.begin(), wf.end(), win_file);
    std::copy(ws.begin(), ws.end(), win_seek);
    std::copy(wl.begin(), wl.end(), win_len);
  });
}

AX_WHISPER_API int AX_WHISPER_ComputeMelWindowCut(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, int seek, int len, float* mel_out) {
  if (!handle || !pcm || !mel_out || num_samples < 1 || seek < 0) return -1;
  return guarded(handle, [&](Engine& e) { e.compute_mel_window_cut(pcm, num_samples, seek, len, mel_out); });
}

// AX_WHISPER_CHUNK_OPTIONS + AX_WHISPER_LONG_OPTIONS -> ChunkedOptions; what the mode does not cover travels along and is refused by the
// engine with its text (longform.hpp: chunked_options_error)
static axw::ChunkedOptions chunked_options(const AX_WHISPER_CHUNK_OPTIONS* chunk, const AX_WHISPER_LONG_OPTIONS* o, int n_files, bool want_scores) {
  axw::ChunkedOptions c;
  c.cut = cut_params(chunk);
  c.beam_size = chunk ? chunk->beam_size : 1;
  c.scored = want_scores;
  if (!o) return c;
  c.no_speech_threshold = o->no_speech_threshold; c.logprob_threshold = o->logprob_threshold;
  if (!std::isnan(o->no_speech_threshold) || !std::isnan(o->logprob_threshold)) c.scored = true;
  if (o->lang) c.file_lang.assign(o->lang, o->lang + n_files);
  if (o->task) c.file_task.assign(o->task, o->task + n_files);
  c.n_temperatures = o->temperatures ? std::max(o->n_temperatures, 0) : 0;
  c.compression_ratio_threshold = !std::isnan(o->compression_ratio_threshold);
  for (int f = 0; o->initial_prompt_ids && o->n_initial && f < n_files; ++f)
    if (o->n_initial[f] > 0) c.initial_prompt = true;
  c.condition_on_previous_text = o->condition_on_previous_text != 0;
  c.word_timestamps = o->word_timestamps != 0;
  return c;
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongChunkedWindows(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                       int max_new, int max_passes, const AX_WHISPER_CHUNK_OPTIONS* chunk,
                                                       const AX_WHISPER_LONG_OPTIONS* o, int win_cap, int* win_info, int32_t* ids,
                                                       float* win_score, int* n_windows) {
  if (!handle || !axw::long_files_ok(pcm, num_samples, n_files) || win_cap < 0 || !n_windows || (win_cap > 0 && (!win_info || !ids))) return -1;
  *n_windows = 0;
  const axw::ChunkedOptions opts = chunked_options(chunk, o, n_files, win_score != nullptr);
  if (opts.scored && win_cap > 0 && !win_score) return -1;
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    std::vector<axw::LongWindow> log;
    g.run_long_chunked(pcm, num_samples, n_files, max_new, max_passes, opts, log);
    require_win_cap("RunPCMLongChunkedWindows", log.size(), win_cap);
    write_window_rows(log, g.primary().config().n_text_ctx, opts.scored ? 3 : 0, {win_cap, win_info, ids, win_score, nullptr, n_windows, nullptr, nullptr});
  });
}

AX_WHISPER_API int AX_WHISPER_RunPCMLongChunked(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, const AX_WHISPER_CHUNK_OPTIONS* chunk,
                                                const AX_WHISPER_LONG_OPTIONS* o, char** result) {
  if (!handle || !pcm_data || !result || num_samples < 1) return -1;
  *result = nullptr;
  const axw::ChunkedOptions opts = chunked_options(chunk, o, 1, false);
  return guarded_group(handle, [&](axw::DeviceGroup<Engine>& g) {
    Engine& e = g.primary();
    std::vector<axw::LongWindow> log;
    const float* files[1] = {pcm_data};
    g.run_long_chunked(files, &num_samples, 1, 0, 0, opts, log);
    const int T = (int)e.config().ints.at("timestamp_begin"), E = e.config().eot;
    const bool lang = !opts.file_lang.empty() && opts.file_lang[0] >= 0;
    *result = strdup(join_segment_texts(e, log, lang ? &opts.file_lang[0] : nullptr, [&](const axw::LongWindow& w) {
      return axw::chunked_segments(w.ids.data(), (int)w.ids.size(), T, E, w.seek, w.window_frames);
    }).c_str());
  });
}

AX_WHISPER_API int AX_WHISPER_RunFileLongChunked(AX_WHISPER_HANDLE handle, const char* wav_file, const AX_WHISPER_CHUNK_OPTIONS* chunk,
                                                 const AX_WHISPER_LONG_OPTIONS* o, char** result) {
  return run_wav(handle, wav_file, result, [&](float* pcm, int n) { return AX_WHISPER_RunPCMLongChunked(handle, pcm, n, chunk, o, result); });
}

AX_WHISPER_API int AX_WHISPER_GetTimings(AX_WHISPER_HANDLE handle, float* out5) {
  if (!handle || !out5) return -1;
  return guarded(handle, [&](Engine& e) { memcpy(out5, e.timings, sizeof(float) * 5); });
}

AX_WHISPER_API int AX_WHISPER_Bench(AX_WHISPER_HANDLE handle, const char* what, int batch, int arg, int iters, float* ms_total) {
  if (!handle || !what || !ms_total || batch < 1 || iters < 1) return -1;
  return guarded(handle, [&](Engine& e) { *ms_total = e.bench(what, batch, arg, iters); });
}

}  // extern "C"
