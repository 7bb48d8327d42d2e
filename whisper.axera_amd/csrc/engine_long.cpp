// engine_long.cpp — long-form transcription (DESIGN.md "Long-form"): the log-mel of whole files kept in HBM, and the seek loop
// that decodes one 30 s window of every unfinished file per pass through the batched encoder and the timestamp-mode step graph.
#include "engine_impl.hpp"
#include "words.hpp"

namespace axw {
inline namespace AXW_NS {

// bytes the PCM and the log-mel rows of one call may take (AX_WHISPER_LONG_MAX_BYTES; default 4 GiB = about 9 hours of audio
// at 80 mels): a call beyond it is refused with this text instead of failing somewhere in hipMalloc
static size_t long_max_bytes() {
  const char* e = getenv("AX_WHISPER_LONG_MAX_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? (size_t)v : (size_t)4 << 30;
}
static constexpr size_t kLongKeepBytes = (size_t)256 << 20;  // an arena up to this size stays allocated for the next call

void Engine::long_release() {
  if (long_.bytes <= kLongKeepBytes) return;
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipStreamSynchronize(stream()));
  long_ = LongArena{};
}

// pcm == nullptr: n_files files of silence (bench)
void Engine::long_prepare(const float* const* pcm, const int* n_samples, int n_files, int n_windows, const CutParams* cut, bool want_e) {
  if (feature_openai_)
    throw std::runtime_error("long-form needs the default front-end: AX_WHISPER_FEATURE_MODE=openai trims the input to 30 s before the STFT");
  if (cfg_.n_mels % 8 != 0) throw std::runtime_error("long-form needs n_mels to be a multiple of 8");
  const int nm = cfg_.n_mels;
  std::vector<long long> pcm_off(n_files), frame_off(n_files);
  std::vector<int> nf(n_files);
  size_t samples = 0, frames = 0;
  int max_frames = 1;
  for (int b = 0; b < n_files; ++b) {
    if (n_samples[b] < 1) throw std::runtime_error("file " + std::to_string(b) + ": empty audio");
    if (n_samples[b] > (1 << 29)) throw std::runtime_error("file " + std::to_string(b) + ": more than 2^29 samples");
    if (pcm) {
      unsigned bad = 0;
      for (int i = 0; i < n_samples[b]; ++i) bad |= !std::isfinite(pcm[b][i]);
      if (bad) throw std::runtime_error("file " + std::to_string(b) + ": non-finite PCM sample (NaN or Inf)");
    }
    pcm_off[b] = (long long)samples;
    frame_off[b] = (long long)frames;
    nf[b] = 1 + n_samples[b] / kHop;
    samples += ((size_t)n_samples[b] + 3) & ~(size_t)3;  // every file starts on a 16-byte boundary
    frames += (size_t)nf[b];
    max_frames = std::max(max_frames, nf[b]);
  }
  // chunked calls: every file's room in the window lists (long_cuts.hpp: at most ceil(content / W_min) + 1 windows)
  std::vector<int> seg_off(cut ? n_files + 1 : 0, 0);
  for (int b = 0; cut && b < n_files; ++b) {
    const long room = (long)seg_off[b] + std::max(1, cut_plan_capacity(n_samples[b] / kHop, cut->w_min));  // (at least one: the stage-level window call)
    if (room > (1L << 28)) throw std::runtime_error("chunked long-form: more than 2^28 windows");
    seg_off[b + 1] = (int)room;
  }
  const size_t plan_cap = cut ? (size_t)seg_off[n_files] : 0;
  // arena: [pcm | store | pcm_off | frame_off | n_samples | n_frames | gmax | win_file | win_seek], pieces 256-byte aligned;
  // chunked calls add [levels | frame levels | seg_off | seg_seek | seg_len | plan block]
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t o = 0;
  const size_t o_pcm = o; o += up(samples * 4);
  const size_t o_store = o; o += up(frames * nm * 4);
  const size_t o_poff = o; o += up((size_t)n_files * 8);
  const size_t o_foff = o; o += up((size_t)n_files * 8);
  const size_t o_ns = o; o += up((size_t)n_files * 4);
  const size_t o_nf = o; o += up((size_t)n_files * 4);
  const size_t o_gmax = o; o += up((size_t)n_files * 4);
  const size_t o_wf = o; o += up((size_t)n_windows * 4);
  const size_t o_ws = o; o += up((size_t)n_windows * 4);
  const size_t o_lev = o; o += cut ? up(frames * 4) : 0;
  const size_t o_leve = o; o += cut && want_e ? up(frames * 4) : 0;
  const size_t o_so = o; o += cut ? up((size_t)(n_files + 1) * 4) : 0;
  const size_t o_ss = o; o += up(plan_cap * 4);
  const size_t o_sl = o; o += up(plan_cap * 4);
  const size_t o_plan = o; o += cut ? up(((size_t)n_files + 3 * plan_cap) * 4) : 0;
  if (o > long_max_bytes())
    throw std::runtime_error("long-form: the PCM and log-mel stores of this call need " + std::to_string(o) + " bytes, the cap is " +
                             std::to_string(long_max_bytes()) + " (AX_WHISPER_LONG_MAX_BYTES)");
  // allocation and synchronous copies: not beside another handle's stream capture (iengine.hpp)
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipStreamSynchronize(stream()));  // an earlier call on this stream may still read the arena
  if (o > long_.bytes) {
    long_ = LongArena{};  // (first: the old and the new arena need not fit side by side)
    long_.base = device_array<char>(o);
    long_.bytes = o;
  }
  if (n_windows > h_long_win_cap_) {
    h_long_win_cap_ = 0;
    h_long_win_ = pinned_array<int>((size_t)2 * n_windows);
    h_long_win_cap_ = n_windows;
  }
  char* a = long_.base;
  long_.pcm = (float*)(a + o_pcm); long_.store = (float*)(a + o_store);
  long_.pcm_off = (long long*)(a + o_poff); long_.frame_off = (long long*)(a + o_foff);
  long_.n_samples = (int*)(a + o_ns); long_.n_frames = (int*)(a + o_nf); long_.gmax = (unsigned*)(a + o_gmax);
  long_.win_file = (int*)(a + o_wf); long_.win_seek = (int*)(a + o_ws);
  long_.n_files = n_files; long_.n_windows = n_windows;
  long_.levels = cut ? (float*)(a + o_lev) : nullptr; long_.levels_e = cut && want_e ? (float*)(a + o_leve) : nullptr;
  long_.seg_off = cut ? (int*)(a + o_so) : nullptr; long_.seg_seek = cut ? (int*)(a + o_ss) : nullptr; long_.seg_len = cut ? (int*)(a + o_sl) : nullptr;
  long_.plan = cut ? (int*)(a + o_plan) : nullptr; long_.plan_cap = (int)plan_cap; long_.max_frames = max_frames;
  if (cut) HIP_CHECK(hipMemcpy(long_.seg_off, seg_off.data(), (size_t)(n_files + 1) * 4, hipMemcpyHostToDevice));
  for (int b = 0; b < n_files; ++b) {
    if (pcm) HIP_CHECK(hipMemcpy(long_.pcm + pcm_off[b], pcm[b], (size_t)n_samples[b] * 4, hipMemcpyHostToDevice));
    else HIP_CHECK(hipMemset(long_.pcm + pcm_off[b], 0, (size_t)n_samples[b] * 4));
  }
  HIP_CHECK(hipMemcpy(long_.pcm_off, pcm_off.data(), (size_t)n_files * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(long_.frame_off, frame_off.data(), (size_t)n_files * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(long_.n_samples, n_samples, (size_t)n_files * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(long_.n_frames, nf.data(), (size_t)n_files * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipDeviceSynchronize());  // (the engine's streams are not ordered against the null stream)
  FrontendParams p{};
  p.pcm = long_.pcm; p.n_samples = long_.n_samples; p.batch = n_files; p.n_mels = nm;
  p.twiddle = twiddle_; p.window = window_; p.mel_basis = mel_basis_t_;
  p.gmax = long_.gmax; p.max_frames = max_frames;
  LongStoreParams ls{long_.pcm_off, long_.frame_off, long_.store};
  launch_frontend_long(p, ls, stream());
}

// window i of this pass = file files[i] at seeks[i] -> encoder slot i. The caller waits for the stream before the next pass
// (fetch_ids), so one pinned staging buffer serves every pass.
void Engine::long_windows_to_slots(const int* files, const int* seeks, int count, bool want_ref_layout) {
  if (count < 1 || count > long_.n_windows || count > cap_) throw std::runtime_error("long-form: bad window count");
  for (int i = 0; i < count; ++i)
    if (files[i] < 0 || files[i] >= long_.n_files || seeks[i] < 0) throw std::runtime_error("long-form: bad window");
  memcpy(h_long_win_, files, (size_t)count * 4);
  memcpy(h_long_win_ + count, seeks, (size_t)count * 4);
  hipStream_t s = stream();
  HIP_CHECK(hipMemcpyAsync(long_.win_file, h_long_win_, (size_t)count * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(long_.win_seek, h_long_win_ + count, (size_t)count * 4, hipMemcpyHostToDevice, s));
  MelWindowParams w{};
  w.store = long_.store; w.frame_off = long_.frame_off; w.n_frames = long_.n_frames; w.gmax = long_.gmax;
  w.win_file = long_.win_file; w.win_seek = long_.win_seek;
  w.mel_tm = d_mel_tm_; w.mel_ref = want_ref_layout ? d_mel_ref_ : nullptr;
  w.mel_rows = mel_rows_; w.n_mels = cfg_.n_mels; w.n_windows = count;
  launch_mel_window(w, s);
}

void Engine::compute_mel_window(const float* pcm, int n_samples, int seek, float* mel_out) {
  require_no_stream("compute_mel_window");
  if (seek < 0) throw std::runtime_error("compute_mel_window: negative seek");
  HIP_CHECK(hipSetDevice(device_));
  ensure_capacity(1);
  const float* arr[1] = {pcm};
  long_prepare(arr, &n_samples, 1, 1);
  const int file = 0;
  long_windows_to_slots(&file, &seek, 1, true);
  HIP_CHECK(hipMemcpyAsync(mel_out, d_mel_ref_, (size_t)cfg_.n_mels * kFramesOut * 4, hipMemcpyDeviceToHost, stream()));
  HIP_CHECK(hipStreamSynchronize(stream()));
  long_release();
}

// opts != nullptr: the windows are decoded in scored mode, every log entry carries its two numbers, and a window the silent-window
// rule drops emits nothing and advances by its whole length (DESIGN.md "Confidence")
// opts->temperatures non-empty: temperature fallback (DESIGN.md "Temperature fallback"). Sampled mode throughout; a pass entry is
// (file, seek, attempt); a window that needs fallback and has attempts left does not advance, it is encoded and decoded again in
// the next pass at the next temperature (one more log entry, kept = false on the one that failed).
// opts->prompted(): prompt conditioning (DESIGN.md "Prompt conditioning"). Every file carries (all_ids, reset_since); a window's
// prompt, the same for each of its attempts, goes to greedy_loop in the pass's contexts, and carry_prompt runs after every kept window.
// opts->per_file_language(): a language and task per file (DESIGN.md "Language and task per clip"). Every window of a pass carries
// its file's language and task to greedy_loop in the same contexts; a detecting file asks for -2 on its first window (seek 0,
// attempt 0) and for the index that came back on every window after it.
void Engine::run_long_windows(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes,
                              const LongScoreOptions* opts, std::vector<LongWindow>& log) {
  if (n_files < 1) throw std::runtime_error("n_files must be >= 1");
  require_no_stream("run_long_windows");
  require_timestamp_vocab();
  if (opts) require_scored_vocab();
  const bool fallback = opts && !opts->temperatures.empty();
  const bool prompted = opts && opts->prompted();
  const bool per_lang = opts && opts->per_file_language();
  if (prompted && !opts->initial_prompt_ids.empty() && (long)opts->initial_prompt_ids.size() < (long)opts->file_base + n_files)
    throw std::runtime_error("long-form: fewer initial prompts than files");
  const int n_attempts = fallback ? (int)opts->temperatures.size() : 1;
  if (n_attempts > 16) throw std::runtime_error("long-form: at most 16 temperatures");
  if (fallback && !opts->file_ids.empty() && (long)opts->file_ids.size() < (long)opts->file_base + n_files)
    throw std::runtime_error("long-form: fewer file ids than files");
  for (int a = 0; a < n_attempts && fallback; ++a)
    if (!(opts->temperatures[a] >= 0.f) || std::isinf(opts->temperatures[a]) || (opts->temperatures[a] > 0.f && opts->temperatures[a] < 1e-6f))
      throw std::runtime_error("long-form: temperatures must be 0, or finite and >= 1e-6");
  const StepSpec spec = step_spec(fallback ? kDecodeSampled : opts ? kDecodeScored : kDecodeTimestamps);
  // the language every file decodes under (-2: still to be detected) and its task
  std::vector<int> file_lang(per_lang ? n_files : 0, -1), file_task(per_lang ? n_files : 0, 0);
  if (per_lang) {
    for (const std::vector<int>* v : {&opts->file_lang, &opts->file_task})
      if (!v->empty() && (long)v->size() < (long)opts->file_base + n_files) throw std::runtime_error("long-form: fewer languages or tasks than files");
    for (int f = 0; f < n_files; ++f) {
      if (!opts->file_lang.empty()) file_lang[f] = opts->file_lang[(size_t)(opts->file_base + f)];
      if (!opts->file_task.empty()) file_task[f] = opts->file_task[(size_t)(opts->file_base + f)];
    }
    // a bad request fails before any GPU work
    check_contexts(spec.mode, ClipContexts{std::nullopt, LangSpec{file_lang.data(), file_task.data()}}, n_files, false, "run_long_windows");
    for (int f = 0; f < n_files; ++f) {
      if (file_lang[f] == -1) file_lang[f] = handle_lang_;
      // (a file without a window keeps this: the index it asked for, the handle's where it asked for detection)
      if (opts->file_lang_out) opts->file_lang_out[opts->file_base + f] = file_lang[f] == -2 ? handle_lang_ : file_lang[f];
    }
  }
  HIP_CHECK(hipSetDevice(device_));
  auto t0 = std::chrono::steady_clock::now();
  // windows per pass: the engine's capacity (AX_WHISPER_MAX_BATCH / max_batch of Init, or what earlier calls grew it to);
  // more files than that wait for a place
  const int S = std::min(n_files, std::max(cap_, 1));
  ensure_capacity(S);
  hipStream_t s = stream();
  HIP_CHECK(hipEventRecord(ev_[0], s));
  long_prepare(pcm, n_samples, n_files, S);
  HIP_CHECK(hipEventRecord(ev_[1], s));
  const int T = cfg_.no_timestamps + 1, E = cfg_.eot, Tc = cfg_.n_text_ctx;
  std::vector<int> seek(n_files, 0), attempt(n_files, 0), active, files(S), seeks(S), n_ids(S);
  std::vector<float> temps(S);
  std::vector<uint64_t> streams(S);
  std::vector<int32_t> ids((size_t)S * Tc);
  std::vector<float> avg(S), nsp(S);
  std::vector<WindowSegment> segs;
  // prompt conditioning: the carried text of every file; a window's prompt is the same for all of its attempts
  const int keep = Tc / 2 - 1;
  std::vector<PromptCarry> carry(prompted ? n_files : 0);
  for (int f = 0; prompted && f < n_files && !opts->initial_prompt_ids.empty(); ++f) carry[f].all_ids = opts->initial_prompt_ids[(size_t)(opts->file_base + f)];
  std::vector<int32_t> prompt_ids(prompted ? (size_t)S * keep : 0);
  std::vector<int> n_prompt(prompted ? S : 0, 0);
  std::vector<int> win_lang(per_lang ? S : 0), win_task(per_lang ? S : 0), win_lang_got(per_lang ? S : 0);
  // what every pass decodes behind: the arrays above, filled per pass
  ClipContexts ctx;
  if (prompted) ctx.prompts = PromptSpec{prompt_ids.data(), keep, n_prompt.data()};
  if (per_lang) { ctx.lang = LangSpec{win_lang.data(), win_task.data()}; ctx.lang_out.detected = win_lang_got.data(); }
  // word timestamps: the tables of the pass's one alignment call, the log entry a slot's window went to, every file's last word end
  const bool words = opts && opts->word_timestamps;
  std::vector<int32_t> al_ids(words ? (size_t)S * Tc : 0);
  std::vector<int> al_n(words ? S : 0), al_frames(words ? S : 0), al_lang(words ? S : 0), al_task(words ? S : 0), al_jump(words ? (size_t)S * (Tc + 1) : 0);
  std::vector<float> al_lp(words ? (size_t)S * Tc : 0);
  std::vector<long> win_log(words ? S : 0, -1);
  std::vector<double> last_speech(words ? n_files : 0, 0.0);
  int next_file = 0, steps = 0;
  for (int pass = 0; max_passes <= 0 || pass < max_passes; ++pass) {
    // finished files leave, the others move up, waiting files take the free places
    int k = 0;
    for (int f : active)
      if (seek[f] < n_samples[f] / kHop) active[k++] = f;
    active.resize(k);
    while ((int)active.size() < S && next_file < n_files) {
      if (n_samples[next_file] / kHop > 0) active.push_back(next_file);  // (a file below one frame has no window)
      ++next_file;
    }
    const int A = (int)active.size();
    if (A == 0) break;
    for (int i = 0; i < A; ++i) { files[i] = active[i]; seeks[i] = seek[active[i]]; }
    if (fallback) {  // the clip's stream is (seek, file id * 16 + attempt): a file's draws do not depend on its neighbours
      for (int i = 0; i < A; ++i) {
        temps[i] = opts->temperatures[attempt[files[i]]];
        streams[i] = (uint64_t)(uint32_t)seeks[i] | (uint64_t)(uint32_t)(opts->file_id(files[i]) * 16 + attempt[files[i]]) << 32;
      }
      // (waits for the stream, which the last pass's fetch left idle)
      upload_sample(SampleSpec{temps.data(), streams.data(), opts->seed}, A);
    }
    long_windows_to_slots(files.data(), seeks.data(), A, false);
    run_encoder(A);
    if (prompted) {
      for (int i = 0; i < A; ++i) {
        const PromptCarry& c = carry[files[i]];
        const int n = std::min((int)c.all_ids.size() - c.reset_since, keep);
        n_prompt[i] = n;
        std::copy(c.all_ids.end() - n, c.all_ids.end(), prompt_ids.begin() + (size_t)i * keep);
      }
    }
    for (int i = 0; per_lang && i < A; ++i) { win_lang[i] = file_lang[files[i]]; win_task[i] = file_task[files[i]]; }
    steps += greedy_loop(spec, A, max_new, nullptr, ctx);
    for (int i = 0; per_lang && i < A; ++i) {
      const int f = files[i];
      if (file_lang[f] != -2) continue;
      file_lang[f] = win_lang_got[i];  // detected once, on the window at seek 0; every later window of the file uses it
      if (opts->file_lang_out) opts->file_lang_out[opts->file_base + f] = file_lang[f];
    }
    fetch_ids(A, ids.data(), n_ids.data());
    if (opts) fetch_scores(A, n_ids.data(), nullptr, avg.data(), nsp.data(), nullptr);
    for (int i = 0; i < A; ++i) {
      const int f = files[i];
      LongWindow w;
      w.file = f; w.seek = seeks[i]; w.pass = pass; w.slot = i;
      w.window_frames = std::min(kFramesOut, n_samples[f] / kHop - seeks[i]);
      const int n = std::max(0, std::min(n_ids[i], Tc));
      w.ids.assign(ids.begin() + (size_t)i * Tc, ids.begin() + (size_t)i * Tc + n);
      if (prompted) w.n_prompt = n_prompt[i];
      if (opts) { w.no_speech_logprob = nsp[i]; w.avg_logprob = avg[i]; }
      if (fallback) {
        // the window's text: the raw bytes of its ids below eot, before the zh post-pass
        std::vector<int32_t> text_ids;
        for (int32_t id : w.ids)
          if (id < E) text_ids.push_back(id);
        const std::string text = strip_ascii_space(detokenize(text_ids.data(), (int)text_ids.size()));
        w.attempt = attempt[f]; w.temperature = temps[i];
        w.compression_ratio = compression_ratio(reinterpret_cast<const unsigned char*>(text.data()), text.size());
        const bool need = window_needs_fallback(w.compression_ratio, avg[i], nsp[i], opts->compression_ratio_threshold, opts->logprob_threshold,
                                                opts->no_speech_threshold);
        if (getenv("AX_WHISPER_LONG_LOG"))
          fprintf(stderr, "[ax_whisper] long: file %d seek %d attempt %d (t %.2f): compression_ratio %.3f avg_logprob %.4f%s\n", f, seeks[i],
                  w.attempt, w.temperature, w.compression_ratio, avg[i], need ? " (needs fallback)" : "");
        if (need && attempt[f] + 1 < n_attempts) {  // decoded again in the next pass; the file stays where it is
          w.kept = false; w.advance = 0;
          ++attempt[f];
          log.push_back(std::move(w));
          continue;
        }
        attempt[f] = 0;  // kept (the last attempt even if it fails too)
      }
      if (opts) {
        w.skipped = long_window_is_silent(nsp[i], avg[i], opts->no_speech_threshold, opts->logprob_threshold);
        if (getenv("AX_WHISPER_LONG_LOG"))
          fprintf(stderr, "[ax_whisper] long: file %d seek %d: no_speech_logprob %.4f avg_logprob %.4f%s\n", f, seeks[i], nsp[i], avg[i],
                  w.skipped ? " (skipped)" : "");
      }
      w.advance = w.skipped ? w.window_frames : split_window(w.ids.data(), n, T, E, w.window_frames, segs);
      seek[f] += w.advance;
      if (prompted) carry_prompt(carry[f], w.ids.data(), n, T, E, w.window_frames, w.skipped, opts->condition_on_previous_text, fallback ? temps[i] : 0.f);
      if (words && !w.skipped) win_log[i] = (long)log.size();
      log.push_back(std::move(w));
    }
    if (!words) continue;
    // Word timestamps: the decisions of the pass stand; its kept, non-skipped windows are aligned in ONE call over the pass's slots
    // (their cross K/V is still there; the alignment overwrites self-attention caches, which the next pass rewrites), then the word
    // rule runs per window in file time and long_word_advance may move the file's seek to the last word's end.
    bool any = false;
    for (int i = 0; i < A; ++i) {
      al_n[i] = 0; al_frames[i] = 2; al_lang[i] = -1; al_task[i] = 0;
      if (win_log[i] < 0) continue;
      LongWindow& w = log[(size_t)win_log[i]];
      split_window(w.ids.data(), (int)w.ids.size(), T, E, w.window_frames, segs);
      const double time_offset = (double)w.seek / 100.0;
      for (const WindowSegment& sg : segs) {
        int count = 0;
        for (int k = sg.tok_begin; k < sg.tok_end; ++k)
          if (w.ids[k] < E && (int)w.text_ids.size() + 5 < Tc) { w.text_ids.push_back(w.ids[k]); ++count; }  // (the alignment's bound)
        w.seg_tokens.push_back(count);
        w.seg_start.push_back(time_offset + (double)sg.start);
        w.seg_end.push_back(time_offset + (double)sg.end);
      }
      if (w.window_frames < 2 || w.text_ids.empty()) continue;  // (no encoder frame to align against, or no text: no words)
      al_n[i] = (int)w.text_ids.size();
      std::copy(w.text_ids.begin(), w.text_ids.end(), al_ids.begin() + (size_t)i * Tc);
      al_frames[i] = w.window_frames;
      if (per_lang) { al_lang[i] = file_lang[files[i]]; al_task[i] = file_task[files[i]]; }
      any = true;
    }
    if (any)
      align_tokens(AlignRequest{A, al_ids.data(), Tc, al_n.data(), al_frames.data(), al_lang.data(), al_task.data(), al_jump.data(), al_lp.data(), nullptr,
                                0, 0, opts->word_logprob_route});
    for (int i = 0; i < A; ++i) {
      if (win_log[i] < 0) continue;
      LongWindow& w = log[(size_t)win_log[i]];
      win_log[i] = -1;
      const int f = files[i], nt = al_n[i], li = per_lang ? file_lang[f] : handle_lang_;
      if (nt > 0) {
        w.jump.assign(al_jump.begin() + (size_t)i * (Tc + 1), al_jump.begin() + (size_t)i * (Tc + 1) + nt + 1);
        w.word_logprob.assign(al_lp.begin() + (size_t)i * Tc, al_lp.begin() + (size_t)i * Tc + nt);
        const std::string code = li >= 0 && li < (int)cfg_.lang_codes.size() ? cfg_.lang_codes[(size_t)li] : std::string();
        for (const WordOut& o : words_from_alignment(token_table(), w.text_ids.data(), nt, E, code, w.seg_tokens.data(), w.seg_start.data(), w.seg_end.data(),
                                                     (int)w.seg_tokens.size(), w.jump.data(), w.word_logprob.data(), last_speech[f], (double)w.seek / 100.0))
          w.words.push_back(LongWord{o.segment, o.text, o.start, o.end, (float)o.probability});
      } else {
        w.text_ids.clear();  // (nothing was aligned)
        for (int& t : w.seg_tokens) t = 0;
      }
      const bool has_word = !w.words.empty();
      const double last_word_end = has_word ? w.words.back().end : 0.0;
      bool by_word_end = false;
      const int adv = long_word_advance(w.ids.data(), (int)w.ids.size(), T, w.seek, w.window_frames, w.advance, has_word, last_word_end, &by_word_end);
      seek[f] += adv - w.advance;
      w.advance = adv;
      w.by_word_end = by_word_end;
      if (has_word) last_speech[f] = last_word_end;
    }
  }
  HIP_CHECK(hipEventRecord(ev_[3], s));
  HIP_CHECK(hipEventSynchronize(ev_[3]));
  (void)hipEventElapsedTime(&timings[0], ev_[0], ev_[1]);  // upload + whole-file front-end
  timings[1] = 0.f;                                        // (encoder and decode loop alternate: both are in [2])
  (void)hipEventElapsedTime(&timings[2], ev_[1], ev_[3]);
  timings[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  timings[4] = (float)steps;
  long_release();
}

// ------------------------------------------------------------------------------ chunked long-form (DESIGN.md "Chunked long-form")
// levels kernel + plan kernels over the files long_prepare left in the arena (prepared with cut parameters)
void Engine::long_plan(const CutParams& cut) {
  LongLevelsParams lv{};
  lv.store = long_.store; lv.frame_off = long_.frame_off; lv.n_frames = long_.n_frames; lv.gmax = long_.gmax;
  lv.s = long_.levels; lv.e = long_.levels_e;
  lv.n_mels = cfg_.n_mels; lv.n_files = long_.n_files; lv.smooth = cut.smooth; lv.max_frames = long_.max_frames;
  launch_long_levels(lv, stream());
  LongCutPlanParams pl{};
  pl.s = long_.levels; pl.frame_off = long_.frame_off; pl.n_samples = long_.n_samples; pl.seg_off = long_.seg_off;
  pl.seg_seek = long_.seg_seek; pl.seg_len = long_.seg_len;
  pl.n_windows = long_.plan_n(); pl.win_file = long_.plan_file(); pl.win_seek = long_.plan_seek(); pl.win_len = long_.plan_len();
  pl.n_files = long_.n_files; pl.w_min = cut.w_min; pl.w_max = cut.w_max;
  launch_long_cut_plan(pl, stream());
}

int Engine::long_fetch_plan(std::vector<int>& n_windows, std::vector<int>& win_file, std::vector<int>& win_seek, std::vector<int>& win_len) {
  const size_t nf = (size_t)long_.n_files, cap = (size_t)long_.plan_cap;
  std::vector<int> block(nf + 3 * cap);
  HIP_CHECK(hipMemcpyAsync(block.data(), long_.plan, block.size() * 4, hipMemcpyDeviceToHost, stream()));
  HIP_CHECK(hipStreamSynchronize(stream()));
  n_windows.assign(block.begin(), block.begin() + nf);
  long total = 0;
  for (int n : n_windows) {
    if (n < 0) throw std::runtime_error("chunked long-form: bad plan");
    total += n;
  }
  if (total > (long)cap) throw std::runtime_error("chunked long-form: bad plan");
  win_file.assign(block.begin() + nf, block.begin() + nf + total);
  win_seek.assign(block.begin() + nf + cap, block.begin() + nf + cap + total);
  win_len.assign(block.begin() + nf + 2 * cap, block.begin() + nf + 2 * cap + total);
  return (int)total;
}

// windows [first, first + count) of the plan -> encoder slots 0 .. count - 1: the kernel reads the plan's own lists
void Engine::long_cut_windows_to_slots(int first, int count, bool want_ref_layout) {
  if (count < 1 || count > cap_ || first < 0 || first + count > long_.plan_cap) throw std::runtime_error("chunked long-form: bad window range");
  MelWindowParams w{};
  w.store = long_.store; w.frame_off = long_.frame_off; w.n_frames = long_.n_frames; w.gmax = long_.gmax;
  w.win_file = long_.plan_file() + first; w.win_seek = long_.plan_seek() + first;
  w.mel_tm = d_mel_tm_; w.mel_ref = want_ref_layout ? d_mel_ref_ : nullptr;
  w.mel_rows = mel_rows_; w.n_mels = cfg_.n_mels; w.n_windows = count;
  launch_mel_window_cut(w, long_.plan_len() + first, stream());
}

static void check_cut(const CutParams& cut) {
  const std::string bad = cut_params_error(cut.w_min, cut.w_max, cut.smooth);
  if (!bad.empty()) throw std::runtime_error(bad);
}

void Engine::long_frame_levels(const float* const* pcm, const int* n_samples, int n_files, int smooth, float* const* e, float* const* s) {
  require_no_stream("long_frame_levels");
  if (n_files < 1) throw std::runtime_error("n_files must be >= 1");
  CutParams cut;
  cut.smooth = smooth;
  check_cut(cut);
  HIP_CHECK(hipSetDevice(device_));
  long_prepare(pcm, n_samples, n_files, 1, &cut, true);
  long_plan(cut);
  size_t off = 0;
  for (int b = 0; b < n_files; ++b) {
    const size_t nf = 1 + (size_t)n_samples[b] / kHop;
    if (e && e[b]) HIP_CHECK(hipMemcpyAsync(e[b], long_.levels_e + off, nf * 4, hipMemcpyDeviceToHost, stream()));
    if (s && s[b]) HIP_CHECK(hipMemcpyAsync(s[b], long_.levels + off, nf * 4, hipMemcpyDeviceToHost, stream()));
    off += nf;
  }
  HIP_CHECK(hipStreamSynchronize(stream()));
  long_release();
}

void Engine::long_cut_plan(const float* const* pcm, const int* n_samples, int n_files, const CutParams& cut, std::vector<int>& n_windows,
                           std::vector<int>& win_file, std::vector<int>& win_seek, std::vector<int>& win_len, float* const* s_out) {
  require_no_stream("long_cut_plan");
  if (n_files < 1) throw std::runtime_error("n_files must be >= 1");
  check_cut(cut);
  HIP_CHECK(hipSetDevice(device_));
  long_prepare(pcm, n_samples, n_files, 1, &cut, false);
  long_plan(cut);
  size_t off = 0;
  for (int b = 0; b < n_files; ++b) {
    const size_t nf = 1 + (size_t)n_samples[b] / kHop;
    if (s_out && s_out[b]) HIP_CHECK(hipMemcpyAsync(s_out[b], long_.levels + off, nf * 4, hipMemcpyDeviceToHost, stream()));
    off += nf;
  }
  long_fetch_plan(n_windows, win_file, win_seek, win_len);
  long_release();
}

// the plan kernels alone: the caller's levels take the place of a one-file arena
void Engine::long_cut_plan_from_levels(const float* s, int content, int w_min, int w_max, std::vector<CutWindow>& plan) {
  require_no_stream("long_cut_plan_from_levels");
  CutParams cut;
  cut.w_min = w_min; cut.w_max = w_max; cut.smooth = 0;
  check_cut(cut);
  if (content < 1 || content > (1 << 29) / kHop) throw std::runtime_error("long_cut_plan_from_levels: content must be 1 .. 2^29 / 160 frames");
  for (int f = 0; f < content; ++f)
    if (!std::isfinite(s[f])) throw std::runtime_error("chunked long-form: level " + std::to_string(f) + " is not finite");
  HIP_CHECK(hipSetDevice(device_));
  const int cap = cut_plan_capacity(content, w_min);
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  // [levels | frame_off (8) | n_samples | seg_off (2) | seg_seek | seg_len | plan block (1 + 3 cap)]
  size_t o = 0;
  const size_t o_lev = o; o += up((size_t)content * 4);
  const size_t o_foff = o; o += up(8);
  const size_t o_ns = o; o += up(4);
  const size_t o_so = o; o += up(8);
  const size_t o_ss = o; o += up((size_t)cap * 4);
  const size_t o_sl = o; o += up((size_t)cap * 4);
  const size_t o_plan = o; o += up(((size_t)1 + 3 * (size_t)cap) * 4);
  std::vector<int> block((size_t)1 + 3 * (size_t)cap);
  {
    std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
    HIP_CHECK(hipStreamSynchronize(stream()));
    DeviceArray<char> mem = device_array<char>(o);
    char* a = mem;
    const long long zero = 0;
    const int ns = content * kHop, so[2] = {0, cap};
    HIP_CHECK(hipMemcpy(a + o_lev, s, (size_t)content * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(a + o_foff, &zero, 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(a + o_ns, &ns, 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(a + o_so, so, 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipDeviceSynchronize());  // (the engine's streams are not ordered against the null stream)
    LongCutPlanParams pl{};
    pl.s = (const float*)(a + o_lev); pl.frame_off = (const long long*)(a + o_foff); pl.n_samples = (const int*)(a + o_ns);
    pl.seg_off = (const int*)(a + o_so); pl.seg_seek = (int*)(a + o_ss); pl.seg_len = (int*)(a + o_sl);
    int* plan_dev = (int*)(a + o_plan);
    pl.n_windows = plan_dev; pl.win_file = plan_dev + 1; pl.win_seek = plan_dev + 1 + cap; pl.win_len = plan_dev + 1 + 2 * (size_t)cap;
    pl.n_files = 1; pl.w_min = w_min; pl.w_max = w_max;
    launch_long_cut_plan(pl, stream());
    HIP_CHECK(hipMemcpyAsync(block.data(), plan_dev, block.size() * 4, hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
  }
  const int n = block[0];
  if (n < 0 || n > cap) throw std::runtime_error("chunked long-form: bad plan");
  plan.clear();
  for (int k = 0; k < n; ++k) plan.push_back({block[(size_t)1 + cap + k], block[(size_t)1 + 2 * (size_t)cap + k]});
}

void Engine::compute_mel_window_cut(const float* pcm, int n_samples, int seek, int len, float* mel_out) {
  require_no_stream("compute_mel_window_cut");
  if (seek < 0) throw std::runtime_error("compute_mel_window_cut: negative seek");
  if (len < 0 || len > kFramesOut) throw std::runtime_error("compute_mel_window_cut: len must be 0 .. 3000");
  HIP_CHECK(hipSetDevice(device_));
  ensure_capacity(1);
  const float* arr[1] = {pcm};
  // a one-window plan written by the host where the plan kernels would write it: the arena of a chunked call with the fewest
  // windows of room a file can have (W_min = W_max = 3000; long_prepare gives every file at least one)
  CutParams cut;
  cut.w_min = cut.w_max = kCutMaxFrames;
  long_prepare(arr, &n_samples, 1, 1, &cut, false);
  if (long_.plan_cap < 1) throw std::runtime_error("compute_mel_window_cut: the file holds no frame of audio");
  const int file = 0;
  hipStream_t s = stream();
  HIP_CHECK(hipMemcpyAsync(long_.plan_file(), &file, 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(long_.plan_seek(), &seek, 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(long_.plan_len(), &len, 4, hipMemcpyHostToDevice, s));
  long_cut_windows_to_slots(0, 1, true);
  HIP_CHECK(hipMemcpyAsync(mel_out, d_mel_ref_, (size_t)cfg_.n_mels * kFramesOut * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  long_release();
}

// The passes: windows [base, base + A) of the flat plan -> slots 0 .. A - 1 -> encoder -> timestamp-mode decode -> ids to the host.
// No window waits for another one's result, so a pass is full whenever enough windows are left, whichever files they belong to.
void Engine::run_long_chunked(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes, const ChunkedOptions& opts,
                              std::vector<LongWindow>& log) {
  if (n_files < 1) throw std::runtime_error("n_files must be >= 1");
  require_no_stream("run_long_chunked");
  if (feature_openai_)
    throw std::runtime_error("chunked long-form needs the default front-end: AX_WHISPER_FEATURE_MODE=openai trims the input to 30 s before the STFT");
  {
    const std::string bad = chunked_options_error(opts, opts.file_base + n_files);
    if (!bad.empty()) throw std::runtime_error(bad);
  }
  require_timestamp_vocab();
  if (opts.scored) require_scored_vocab();
  const bool per_lang = !opts.file_lang.empty() || !opts.file_task.empty();
  const StepSpec spec = step_spec(opts.scored ? kDecodeScored : kDecodeTimestamps);
  std::vector<int> file_lang(per_lang ? n_files : 0, -1), file_task(per_lang ? n_files : 0, 0);
  if (per_lang) {
    for (int f = 0; f < n_files; ++f) {
      if (!opts.file_lang.empty()) file_lang[f] = opts.file_lang[(size_t)(opts.file_base + f)];
      if (!opts.file_task.empty()) file_task[f] = opts.file_task[(size_t)(opts.file_base + f)];
    }
    check_contexts(spec.mode, ClipContexts{std::nullopt, LangSpec{file_lang.data(), file_task.data()}}, n_files, false, "run_long_chunked");
    for (int f = 0; f < n_files; ++f)
      if (file_lang[f] == -1) file_lang[f] = handle_lang_;
  }
  HIP_CHECK(hipSetDevice(device_));
  auto t0 = std::chrono::steady_clock::now();
  hipStream_t s = stream();
  HIP_CHECK(hipEventRecord(ev_[0], s));
  long_prepare(pcm, n_samples, n_files, 1, &opts.cut, false);
  long_plan(opts.cut);
  std::vector<int> n_windows, win_file, win_seek, win_len;
  const int total = long_fetch_plan(n_windows, win_file, win_seek, win_len);  // the one copy of the plan: counts and times
  HIP_CHECK(hipEventRecord(ev_[1], s));
  // windows per pass: the engine's capacity, as in the seek loop
  const int S = std::max(1, std::min(total, std::max(cap_, 1)));
  ensure_capacity(S);
  const int Tc = cfg_.n_text_ctx;
  std::vector<int> n_ids(S), win_lang(per_lang ? S : 0), win_task(per_lang ? S : 0);
  std::vector<int32_t> ids((size_t)S * Tc);
  std::vector<float> avg(S), nsp(S);
  ClipContexts ctx;
  if (per_lang) ctx.lang = LangSpec{win_lang.data(), win_task.data()};
  int steps = 0, pass = 0;
  for (int base = 0; base < total && (max_passes <= 0 || pass < max_passes); ++pass) {
    const int A = std::min(S, total - base);
    long_cut_windows_to_slots(base, A, false);
    run_encoder(A);
    for (int i = 0; per_lang && i < A; ++i) { win_lang[i] = file_lang[win_file[base + i]]; win_task[i] = file_task[win_file[base + i]]; }
    steps += greedy_loop(spec, A, max_new, nullptr, ctx);
    fetch_ids(A, ids.data(), n_ids.data());
    if (opts.scored) fetch_scores(A, n_ids.data(), nullptr, avg.data(), nsp.data(), nullptr);
    for (int i = 0; i < A; ++i) {
      LongWindow w;
      w.file = win_file[base + i]; w.seek = win_seek[base + i]; w.window_frames = w.advance = win_len[base + i];
      w.pass = pass; w.slot = i;
      const int n = std::max(0, std::min(n_ids[i], Tc));
      w.ids.assign(ids.begin() + (size_t)i * Tc, ids.begin() + (size_t)i * Tc + n);
      if (opts.scored) {
        w.no_speech_logprob = nsp[i]; w.avg_logprob = avg[i];
        w.skipped = long_window_is_silent(nsp[i], avg[i], opts.no_speech_threshold, opts.logprob_threshold);
      }
      log.push_back(std::move(w));
    }
    base += A;
  }
  HIP_CHECK(hipEventRecord(ev_[3], s));
  HIP_CHECK(hipEventSynchronize(ev_[3]));
  (void)hipEventElapsedTime(&timings[0], ev_[0], ev_[1]);  // upload + whole-file front-end + levels + plan
  timings[1] = 0.f;
  (void)hipEventElapsedTime(&timings[2], ev_[1], ev_[3]);
  timings[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  timings[4] = (float)steps;
  long_release();
}

}  // inline namespace AXW_NS
}  // namespace axw
