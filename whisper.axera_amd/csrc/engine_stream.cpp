// engine_stream.cpp — axw::Engine: utterance slots refilled while the others decode (AX_WHISPER_Stream*), and the probe that
// tells which of the engine's streams share a hardware queue (step_graph places a fresh multi-branch graph with it).
#include "engine_impl.hpp"

namespace axw {
inline namespace AXW_NS {

// ------------------------------------------------------------------------------ slot refill (continuous batching)
// The reference stops every utterance at its own eot (Whisper.cpp:219-222) and serves requests one by one
// (WhisperHTTPServer.hpp:37-100). With per-slot offsets (common.hpp: DecState) a slot whose clip has finished takes the
// next clip while the other slots decode on; the step graph is the one the batched loop replays.
void Engine::require_no_stream(const char* what) const {
  if (stream_slots_ > 0) throw std::runtime_error(std::string(what) + ": a slot stream is open on this handle (AX_WHISPER_StreamClose first)");
}

__global__ static void slot_reset_kernel(int slot, int max_new, const int* sot, int* off, int* tok, int* done, int* n_out, int* max_new_clip,
                                         const h16* tok_emb, const float* pos, float* x, int d) {
  const int t = sot[0];
  if (threadIdx.x == 0) { off[slot] = 0; tok[slot] = t; n_out[slot] = 0; max_new_clip[slot] = max_new; done[slot] = 0; }
  for (int c = threadIdx.x; c < d; c += blockDim.x) x[(long)slot * d + c] = (float)tok_emb[(long)t * d + c] + pos[c];  // position 0
}

// The timestamp twin of slot_reset_kernel (stream mode 1): the slot's own prefix [sot, language id, task id, unused], its detect flag
// and language index, and a zeroed lang_logprob row, so that nothing of the clip that sat here before is left: the language and
// the detect flag are rewritten here, the no-speech value by the rules kernel at offset 0 (every clip passes it), the score entries
// [0 .. n_ids] by the sampled steps.
__global__ static void slot_reset_ts_kernel(int slot, int max_new, int sot, int lang_tok, int task_tok, int lang_index, int detect, int n_lang,
                                            int* slot_ctx, int* slot_detect, int* slot_lang, float* slot_lang_lp, int* off, int* tok, int* done,
                                            int* n_out, int* max_new_clip, const h16* tok_emb, const float* pos, float* x, int d) {
  if (threadIdx.x == 0) {
    off[slot] = 0; tok[slot] = sot; n_out[slot] = 0; max_new_clip[slot] = max_new; done[slot] = 0;
    slot_ctx[4 * slot] = sot; slot_ctx[4 * slot + 1] = lang_tok; slot_ctx[4 * slot + 2] = task_tok; slot_ctx[4 * slot + 3] = 0;
    slot_detect[slot] = detect; slot_lang[slot] = lang_index;
  }
  for (int j = threadIdx.x; j < n_lang; j += blockDim.x) slot_lang_lp[(long)slot * n_lang + j] = 0.f;
  for (int c = threadIdx.x; c < d; c += blockDim.x) x[(long)slot * d + c] = (float)tok_emb[(long)sot * d + c] + pos[c];  // position 0
}

void Engine::ensure_stream_ts() {
  ensure_lang_buffers();
  if (d_slot_ctx_) return;
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  d_slot_ctx_ = pooled<int>(slot_allocs_, (size_t)cap_ * 4, true);  // (freed and re-made with the slot buffers)
  d_slot_detect_ = pooled<int>(slot_allocs_, cap_, true);
  d_slot_lang_ = pooled<int>(slot_allocs_, cap_, true);
  d_slot_lang_lp_ = pooled<float>(slot_allocs_, (size_t)cap_ * cfg_.lang_tokens.size(), true);
}

StreamRulesParams Engine::stream_rules_params() const {
  StreamRulesParams t{};
  t.detect = d_slot_detect_; t.slot_ctx = d_slot_ctx_; t.lang_tokens = prefill_.lang_tok; t.n_lang = (int)cfg_.lang_tokens.size();
  t.fallback_index = handle_lang_; t.lang_out = d_slot_lang_; t.lang_logprob = d_slot_lang_lp_;
  return t;
}

void Engine::stream_open(int n_slots, int mode) {
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  if (n_slots < 1) throw std::runtime_error("stream_open: n_slots must be >= 1");
  if (mode != 0 && mode != 1) throw std::runtime_error("stream_open: unknown mode " + std::to_string(mode) + " (0 plain, 1 scored timestamps)");
  if (user_stream_) throw std::runtime_error("stream_open: not with a caller-supplied stream (AX_WHISPER_SetStream)");
  if (mode == 1) {
    require_scored_vocab();
    if (cfg_.lang_tokens.empty()) throw std::runtime_error("stream_open: the timestamp mode needs the config's language list");
  }
  stream_close();
  ensure_capacity(std::max(n_slots, 3));
  const int n = std::max(n_slots, 3);  // the step sequence of 3+ slots handles any mix of idle and active slots
  hipStream_t s = stream();
  stream_mode_ = mode;
  if (mode == 1) ensure_stream_ts();
  // every launch of the mode's step. Captured here, outside the serving loop (and probed with replays: before the state is set)
  (void)step_graph(stream_spec(), n, cfg_.n_text_ctx - stream_n_prefix());
  reset_decode_state(n);
  std::vector<int> ones(n, 1);         // every slot idle: its attention launches return at once
  HIP_CHECK(hipMemcpy(d_done_, ones.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  h_admit_ring_ = pinned_array<int>((size_t)kAdmitRing * 2 * cap_);
  admit_seq_ = 0;
  while ((int)ev_admit_.size() < n) ev_admit_.push_back(make_event(hipEventDisableTiming));
  HIP_CHECK(hipStreamSynchronize(s));
  slot_state_.assign(n, kIdle);
  slot_max_new_.assign(n, 0);
  slot_lang_.assign(n, handle_lang_);
  slot_task_.assign(n, sot_seq_[2]);
  slot_detect_.assign(n, 0);
  memset(h_done_live_, 0, (size_t)cap_ * 4);
  step_seq_ = 0;
  stream_slots_ = n;
  stream_user_slots_ = n_slots;
  cfg_.ints["stream_slots"] = n_slots;
  cfg_.ints["stream_mode"] = mode;
}

void Engine::stream_close() {
  if (stream_slots_ == 0) return;
  (void)hipStreamSynchronize(admit_stream_);
  (void)hipStreamSynchronize(stream());
  stream_slots_ = 0;
  stream_user_slots_ = 0;
  stream_mode_ = 0;
  slot_state_.clear();
  cfg_.ints["stream_slots"] = 0;
  cfg_.ints["stream_mode"] = 0;
}

void Engine::stream_admit(const int* slots, const float* const* pcm, const int* n_samples, const int* max_new, int count, const int* rates,
                          const int* lang, const int* task) {
  HIP_CHECK(hipSetDevice(device_));
  if (stream_slots_ == 0) throw std::runtime_error("stream_admit: no stream open");
  if (count < 1 || count > stream_user_slots_) throw std::runtime_error("stream_admit: count out of range");
  // a language or task per clip: refused before anything is enqueued, so the stream and its running slots are left as they were
  if ((lang || task) && stream_mode_ != 1) throw std::runtime_error("stream_admit: a language or task per clip needs a stream opened in timestamp mode (AX_WHISPER_StreamOpenMode, mode 1)");
  const int n_lang = (int)cfg_.lang_tokens.size();
  int translate = -1;  // (as plan_contexts reads it: an id inside the vocabulary, or none)
  if (const auto tr = cfg_.ints.find("translate"); tr != cfg_.ints.end() && tr->second >= 0 && tr->second < cfg_.n_vocab) translate = (int)tr->second;
  for (int i = 0; i < count; ++i) {
    if (lang && (lang[i] < -2 || lang[i] >= n_lang)) throw std::runtime_error("stream_admit: language index " + std::to_string(lang[i]) + " of clip " + std::to_string(i) + " outside [-2, " + std::to_string(n_lang) + ")");
    if (lang && lang[i] == -2 && n_lang < 2) throw std::runtime_error("stream_admit: language detection needs a config that lists more than one language");
    if (task && task[i] != 0 && task[i] != 1) throw std::runtime_error("stream_admit: task " + std::to_string(task[i]) + " of clip " + std::to_string(i) + " (0 transcribe, 1 translate)");
    if (task && task[i] == 1 && translate < 0) throw std::runtime_error("stream_admit: translate: the config has no translate id inside the vocabulary");
  }
  for (int i = 0; i < count; ++i) {
    // the slots the caller opened, not the 3 the step graph is rounded up to: finished_slots of StreamStep is [n_slots]
    if (slots[i] < 0 || slots[i] >= stream_user_slots_) throw std::runtime_error("stream_admit: slot out of range");
    if (slot_state_[slots[i]] != kIdle) throw std::runtime_error("stream_admit: slot " + std::to_string(slots[i]) + " is busy");
    for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) throw std::runtime_error("stream_admit: a slot is listed twice");
    if (n_samples[i] < 1) throw std::runtime_error("empty audio clip");
  }
  const int Tc = cfg_.n_text_ctx;
  // front-end + encoder of these clips as ONE batched pass on the admission stream (encoder scratch of clip indices
  // 0..count-1; the decode step touches none of it), cross K/V scattered straight into the slots, which stay idle — their
  // attention launches skip them — until stream_step has seen the event
  struct StreamSwap {  // run_frontend / run_encoder enqueue on stream(): point it at the admission stream for this call
    hipStream_t& u; hipStream_t keep;
    StreamSwap(hipStream_t& us, hipStream_t to) : u(us), keep(us) { u = to; }
    ~StreamSwap() { u = keep; }
  } swap(user_stream_, admit_stream_);
  // Nothing below waits for an earlier pass's ENCODER: the ring entry of this pass was last used kAdmitRing passes ago, the
  // PCM staging rows by the pass before (its uploads are the first thing it enqueued). With sample rates the pass's resample kernel
  // reads the raw staging behind those uploads, so ev_upload_ is recorded behind that kernel: one wait covers both stagings
  const int ring = (int)(admit_seq_ % kAdmitRing);
  if (admit_seq_ >= kAdmitRing) HIP_CHECK(hipEventSynchronize(ev_ring_[ring]));
  if (admit_seq_ > 0) HIP_CHECK(hipEventSynchronize(ev_upload_));
  int* h_ns = h_admit_ring_ + (size_t)ring * 2 * cap_;
  int* h_map = h_ns + cap_;
  memcpy(h_map, slots, (size_t)count * 4);
  HIP_CHECK(hipMemcpyAsync(d_slot_map_, h_map, (size_t)count * 4, hipMemcpyHostToDevice, admit_stream_));
  std::vector<int> n16(count);  // the clips' lengths at 16 kHz: their own without rates
  upload_pcm(pcm, n_samples, count, rates, n16.data());  // (with rates: uploads, then the resample kernel)
  HIP_CHECK(hipEventRecord(ev_upload_, admit_stream_));
  run_frontend(d_pcm_, (int)pcm_stride_, n16.data(), count, false, true, h_ns);
  run_encoder(count, d_slot_map_);
  HIP_CHECK(hipEventRecord(ev_ring_[ring], admit_stream_));
  ++admit_seq_;
  for (int i = 0; i < count; ++i) {
    HIP_CHECK(hipEventRecord(ev_admit_[slots[i]], admit_stream_));
    h_done_live_[slots[i]] = 0;
    slot_state_[slots[i]] = kEncoding;
    const int mn = max_new ? max_new[i] : 0, room = Tc - stream_n_prefix();
    slot_max_new_[slots[i]] = (mn > 0 && mn < room) ? mn : room;
    const int lg = lang ? lang[i] : -1;
    slot_lang_[slots[i]] = lg >= 0 ? lg : handle_lang_;
    slot_detect_[slots[i]] = lg == -2 ? 1 : 0;
    slot_task_[slots[i]] = (task && task[i] == 1) ? translate : sot_seq_[2];  // the task id itself
  }
}

// Up to n decoder steps. Between two steps the host looks at the host-mapped done flags (advance_kernel raises a clip's flag,
// behind a system-scope fence, the moment its ids are final): a finished slot is seen without a copy or a wait, and a slot
// whose encoder has finished joins before the next step. (Measured and not kept: extra slots holding already-encoded clips
// that take over the moment a decoding slot frees — the step then runs its linear layers over more rows and its attention
// launches over more workgroups, and that costs more than the refill latency it removes: 32 + 8 slots 224 -> 202 clips/s.)
int Engine::stream_step(int n_steps, int* finished_slots) {
  HIP_CHECK(hipSetDevice(device_));
  if (stream_slots_ == 0) throw std::runtime_error("stream_step: no stream open");
  hipStream_t s = stream();
  const int n = stream_slots_;
  auto n_in = [&](int st) { int c = 0; for (int i = 0; i < n; ++i) c += slot_state_[i] == st; return c; };
  auto harvest = [&] {
    for (int i = 0; i < n; ++i)
      if (slot_state_[i] == kActive && __atomic_load_n(&h_done_live_[i], __ATOMIC_ACQUIRE)) slot_state_[i] = kFinished;
  };
  // slots whose encoder has finished join; if nothing decodes the loop waits for the first encoder
  auto activate_ready = [&] {
    int active = n_in(kActive);
    for (int i = 0; i < n; ++i) {
      if (slot_state_[i] != kEncoding) continue;
      hipError_t q = hipEventQuery(ev_admit_[i]);
      if (q == hipErrorNotReady && active == 0) { HIP_CHECK(hipEventSynchronize(ev_admit_[i])); q = hipSuccess; }
      if (q == hipErrorNotReady) continue;
      HIP_CHECK(q);
      if (stream_mode_ == 1)
        hipLaunchKernelGGL(slot_reset_ts_kernel, dim3(1), dim3(256), 0, s, i, slot_max_new_[i], sot_seq_[0], cfg_.lang_tokens[slot_lang_[i]],
                           slot_task_[i], slot_lang_[i], slot_detect_[i], (int)cfg_.lang_tokens.size(),
                           d_slot_ctx_, d_slot_detect_, d_slot_lang_, d_slot_lang_lp_, d_off_, d_tok_, d_done_, d_nout_, d_max_new_clip_, tok_emb_,
                           dec_pos_, d_xdec_, cfg_.n_text_state);
      else
        hipLaunchKernelGGL(slot_reset_kernel, dim3(1), dim3(256), 0, s, i, slot_max_new_[i], d_sot_, d_off_, d_tok_, d_done_, d_nout_,
                           d_max_new_clip_, tok_emb_, dec_pos_, d_xdec_, cfg_.n_text_state);
      slot_state_[i] = kActive;
      ++active;
    }
  };
  const StepGraphRef g = step_graph(stream_spec(), n, cfg_.n_text_ctx - stream_n_prefix());  // the graph stream_open captured
  // The host runs two steps ahead of the device (it waits for step k-2 before it enqueues step k): the queue never runs dry,
  // and what the host sees in the flags is at most two steps old, so a waiting clip takes a freed slot within two steps.
  for (int st = 0; st < std::max(1, n_steps); ++st) {
    if (step_seq_ >= 2) HIP_CHECK(hipEventSynchronize(ev_step_[(step_seq_ - 2) % 3]));
    harvest();
    activate_ready();
    if (n_in(kActive) == 0) break;  // nothing decodes and nothing is ready: a step would be the GEMM chain for nobody
    launch_step_graph(g, s);
    HIP_CHECK(hipEventRecord(ev_step_[step_seq_ % 3], s));
    ++step_seq_;
  }
  harvest();
  int n_fin = 0;
  for (int i = 0; i < n; ++i)
    if (slot_state_[i] == kFinished) finished_slots[n_fin++] = i;
  return n_fin;
}

void Engine::stream_collect(int slot, int32_t* ids, int* n_ids) {
  HIP_CHECK(hipSetDevice(device_));
  if (stream_slots_ == 0) throw std::runtime_error("stream_collect: no stream open");
  if (slot < 0 || slot >= stream_user_slots_ || slot_state_[slot] != kFinished) throw std::runtime_error("stream_collect: slot has not finished");
  // on its own stream: the slot's ids are final (its done flag was seen), the decoder steps queued meanwhile do not touch them
  HIP_CHECK(hipMemcpyAsync(ids, d_out_ids_ + (size_t)slot * cfg_.n_text_ctx, (size_t)cfg_.n_text_ctx * 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(n_ids, d_nout_ + slot, 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipStreamSynchronize(copy_stream_));
  slot_state_[slot] = kIdle;
}

// Mode 1: the ids (timestamp tokens included) and the slot's scores and language, on copy_stream_ like the ids: the slot's score
// entries, no-speech value and language were final before its done flag was raised (the rules launch of a step runs in front of its
// advance launch), and a slot whose flag is set is written by nobody until it is refilled.
void Engine::stream_collect_scored(int slot, int32_t* ids, int* n_ids, const SlotScores& out) {
  HIP_CHECK(hipSetDevice(device_));
  if (stream_slots_ == 0) throw std::runtime_error("stream_collect_scored: no stream open");
  if (stream_mode_ != 1) throw std::runtime_error("stream_collect_scored: the stream was not opened in timestamp mode (AX_WHISPER_StreamOpenMode, mode 1)");
  if (slot < 0 || slot >= stream_user_slots_ || slot_state_[slot] != kFinished) throw std::runtime_error("stream_collect_scored: slot has not finished");
  const int Tc = cfg_.n_text_ctx, n_lang = (int)cfg_.lang_tokens.size();
  std::vector<float> lp(Tc), llp(n_lang);
  std::vector<int> dec(Tc);
  float nsp = 0.f;
  int lang = 0;
  HIP_CHECK(hipMemcpyAsync(ids, d_out_ids_ + (size_t)slot * Tc, (size_t)Tc * 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(n_ids, d_nout_ + slot, 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(lp.data(), d_tok_lp_ + (size_t)slot * Tc, (size_t)Tc * 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(dec.data(), d_dec_id_ + (size_t)slot * Tc, (size_t)Tc * 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(&nsp, d_nospeech_ + slot, 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(&lang, d_slot_lang_ + slot, 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipMemcpyAsync(llp.data(), d_slot_lang_lp_ + (size_t)slot * n_lang, (size_t)n_lang * 4, hipMemcpyDeviceToHost, copy_stream_));
  HIP_CHECK(hipStreamSynchronize(copy_stream_));
  clip_score_summary(lp.data(), dec.data(), *n_ids, out.token_logprob, out.avg_logprob, out.ended_eot);
  if (out.no_speech_logprob) *out.no_speech_logprob = nsp;
  if (out.lang) *out.lang = lang;
  if (out.lang_logprob) std::copy(llp.begin(), llp.end(), out.lang_logprob);
  slot_state_[slot] = kIdle;
}

// The stream's rules kernel alone on host data (tests). `chosen` / `logprob` come from a one-partial argmax row and a score row of
// n_text_ctx + 1 entries per slot, as Engine::timestamp_rules has them; every output starts from the caller's values.
void Engine::stream_rules_stage(const StreamRulesIO& io) {
  require_no_stream("stream_rules_stage");
  require_scored_vocab();
  const int n = io.n, Tc = cfg_.n_text_ctx, n_lang = (int)cfg_.lang_tokens.size();
  if (n < 1 || !io.rows || !io.off || !io.done || !io.detect || !io.hist || !io.n_hist || !io.slot_ctx || !io.chosen || !io.logprob ||
      !io.no_speech || !io.lang_out || !io.lang_logprob)
    throw std::runtime_error("stream_rules_stage: bad arguments");
  if (n_lang < 1) throw std::runtime_error("stream_rules_stage: the config lists no languages");
  for (int b = 0; b < n; ++b)
    if (io.off[b] < 0 || io.off[b] >= Tc) throw std::runtime_error("stream_rules_stage: offset out of range");
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  ensure_lang_buffers();
  hipStream_t s = stream();
  const StagedRows in = stage_rows("stream_rules_stage", io.rows, io.hist, io.n_hist, n, s);
  DeviceArray<int> b_off = device_array<int>(n), b_done = device_array<int>(n), b_det = device_array<int>(n), b_ctx = device_array<int>((size_t)n * 4),
                   b_idx = device_array<int>(n), b_dec = device_array<int>((size_t)n * (Tc + 1)), b_lang = device_array<int>(n);
  DeviceArray<float> b_val = device_array<float>(n), b_lp = device_array<float>((size_t)n * (Tc + 1)), b_nsp = device_array<float>(n),
                     b_llp = device_array<float>((size_t)n * n_lang);
  HIP_CHECK(hipMemcpyAsync(b_off, io.off, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_done, io.done, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_det, io.detect, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_ctx, io.slot_ctx, (size_t)n * 16, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_idx, io.chosen, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_nsp, io.no_speech, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_lang, io.lang_out, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b_llp, io.lang_logprob, (size_t)n * n_lang * 4, hipMemcpyHostToDevice, s));
  for (int b = 0; b < n; ++b)  // the entry the kernel would write: the caller's sentinel
    HIP_CHECK(hipMemcpyAsync(b_lp + (size_t)b * (Tc + 1) + io.n_hist[b], io.logprob + b, 4, hipMemcpyHostToDevice, s));
  TsRulesParams r{};
  r.logits = in.logits; r.stride = in.stride; r.batch = n;
  r.n_vocab = cfg_.n_vocab; r.eot = cfg_.eot; r.ts_begin = cfg_.no_timestamps + 1;
  r.off = b_off; r.n_prefix = 3; r.done = b_done;
  r.out_ids = in.hist; r.n_out = in.n_hist; r.n_ctx = Tc;
  r.amax_val = b_val; r.amax_idx = b_idx; r.amax_stride = 1;
  r.suppress = suppress_mask();
  StreamRulesParams t{};
  t.detect = b_det; t.slot_ctx = b_ctx; t.lang_tokens = prefill_.lang_tok; t.n_lang = n_lang; t.fallback_index = handle_lang_;
  t.lang_out = b_lang; t.lang_logprob = b_llp;
  launch_stream_rules(r, TsScoreParams{b_lp, b_dec, (long)Tc + 1, b_nsp, (int)cfg_.ints.at("no_speech")}, t, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(io.chosen, b_idx, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(io.slot_ctx, b_ctx, (size_t)n * 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(io.no_speech, b_nsp, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(io.lang_out, b_lang, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(io.lang_logprob, b_llp, (size_t)n * n_lang * 4, hipMemcpyDeviceToHost, s));
  for (int b = 0; b < n; ++b)
    HIP_CHECK(hipMemcpyAsync(io.logprob + b, b_lp + (size_t)b * (Tc + 1) + io.n_hist[b], 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------ which of the engine's streams run side by side?
// The runtime multiplexes a process's HIP streams onto a few hardware queues (four by default); two streams on one queue
// execute one after the other. A spinner kernel on stream A and a time stamp on stream B, issued right behind it: if the stamp is
// taken before the spinner ends, A and B are on different queues.
__global__ static void queue_probe_spin(unsigned long long* out, long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
  out[0] = (unsigned long long)t0;
  out[1] = (unsigned long long)wall_clock64();
}
__global__ static void queue_probe_mark(unsigned long long* out) { out[0] = (unsigned long long)wall_clock64(); }

static bool streams_concurrent(hipStream_t a, hipStream_t b, unsigned long long* d_buf /*[4]*/) {
  unsigned long long h[4] = {0, 0, 0, 0};
  HIP_CHECK(hipStreamSynchronize(a));
  HIP_CHECK(hipStreamSynchronize(b));
  HIP_CHECK(hipMemset(d_buf, 0, 32));
  queue_probe_spin<<<1, 64, 0, a>>>(d_buf, 30000);  // 300 us on the 100 MHz wall clock
  queue_probe_mark<<<1, 64, 0, b>>>(d_buf + 2);
  HIP_CHECK(hipStreamSynchronize(a));
  HIP_CHECK(hipStreamSynchronize(b));
  HIP_CHECK(hipMemcpy(h, d_buf, 32, hipMemcpyDeviceToHost));
  return h[2] != 0 && h[2] + 5000 < h[1];  // stamped at least 50 us before the spinner ended
}

// hipGraphInstantiate gives every parallel branch of a captured step a stream of its own, and the runtime deals a process's
// streams onto its hardware queues (four by default) round-robin: which queue the branch lands on depends on how many streams the
// process has created before. Measured with 0..5 unused pad streams created ahead (profiles/r05_stream_queue_root_cause.txt,
// stream64, period 4): 335 / 367 / 341 / 345 clips/s — the "bimodality" of rounds 3-4 was this draw (plain step replays do not care:
// 1.130-1.142 ms; the slot stream does, because admission passes and result copies run beside the steps).
// The one good place is the queue of branch_stream_[0], which only ever carries the capture and never a replay. So a freshly
// instantiated multi-branch step is PROBED — a 3 ms spinner on branch_stream_[0], then one replay: if a branch shares that queue the
// replay takes > 3 ms instead of ~1 — and re-instantiated behind one more pad stream until it does (at most 4 times, ~5 ms each, once
// per captured graph). The replays run on whatever the decode state holds: callers reset the state AFTER they have the graph.
bool Engine::graph_branch_shares_queue(hipGraphExec_t exec, hipStream_t other) {
  hipStream_t s = stream();
  const DeviceArray<unsigned long long> d_buf = device_array<unsigned long long>(4);
  const Event e0 = make_event(), e1 = make_event();
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipStreamSynchronize(other));
  HIP_CHECK(hipGraphLaunch(exec, s));  // first launch of a fresh exec: paid here, not inside the measurement
  HIP_CHECK(hipStreamSynchronize(s));
  auto replay_ms = [&](bool with_spinner) {
    if (with_spinner) queue_probe_spin<<<1, 64, 0, other>>>(d_buf, 300000);  // 3 ms
    HIP_CHECK(hipEventRecord(e0, s));
    HIP_CHECK(hipGraphLaunch(exec, s));
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    HIP_CHECK(hipStreamSynchronize(other));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  };
  // a replay of many clips (or on a device another handle keeps busy) takes milliseconds by itself: the spinner shows as
  // ~3 ms ON TOP of the unloaded replay when a branch waits behind it, and as nothing when it does not
  const float base = replay_ms(false);
  const float loaded = replay_ms(true);
  return loaded > base + 2.0f;
}

// bench "queue_probe". Bit i set: pair i runs side by side. Pairs: 0 main-admission, 1 main-branch0, 2 main-copies,
// 3 admission-branch0, 4 admission-copies, 5 branch0-copies (diagnostic of the slot stream's process-to-process bimodality)
int Engine::queue_probe_mask() {
  HIP_CHECK(hipSetDevice(device_));
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  const DeviceArray<unsigned long long> d_buf = device_array<unsigned long long>(4);
  hipStream_t st[4] = {own_stream_, admit_stream_, branch_stream_[0], copy_stream_};
  const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
  int mask = 0;
  for (int i = 0; i < 6; ++i)
    if (streams_concurrent(st[pa[i]], st[pb[i]], d_buf)) mask |= 1 << i;
  return mask;
}

}  // inline namespace AXW_NS
}  // namespace axw
