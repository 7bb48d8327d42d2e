// engine_beam.cpp — axw::Engine: beam search (DESIGN.md "Beam search"). A hypothesis is a slot of the launch-per-phase step: clip c
// owns slots [c * K, c * K + K). Per step the captured step graph runs up to the logits dump (StepSpec::mask 11: no rules kernel, no
// advance), the three kernels of decode_beam.hip choose the next hypotheses, and advance_kernel feeds the chosen ids in its
// teacher-forcing mode with the beam histories as its `forced` array.
#include "engine_impl.hpp"

namespace axw {
inline namespace AXW_NS {

static void check_beam_size(int K, const char* who) {
  if (K < 1 || K > kBeamMax) throw std::runtime_error(std::string(who) + ": beam_size " + std::to_string(K) + " (need 1 .. " + std::to_string(kBeamMax) + ")");
}

void Engine::ensure_beam_buffers() {
  if (beam_.hist) return;
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  const size_t B = cap_, Tc = cfg_.n_text_ctx;
  // (freed, and re-made at the new capacity, with the other slot buffers)
  beam_.hist = pooled<int>(slot_allocs_, B * Tc, true);
  beam_.pool_ids = pooled<int>(slot_allocs_, B * Tc, true);
  beam_.cand_id = pooled<int>(slot_allocs_, B * kBeamMaxCand, true);
  beam_.cand_lp = pooled<float>(slot_allocs_, B * kBeamMaxCand, true);
  beam_.n_cand = pooled<int>(slot_allocs_, B, true);
  beam_.S = pooled<float>(slot_allocs_, B, true);
  beam_.slot_score = pooled<float>(slot_allocs_, B, true);
  beam_.slot = pooled<int>(slot_allocs_, B, true);
  beam_.src = pooled<int>(slot_allocs_, B, true);
  beam_.pool_len = pooled<int>(slot_allocs_, B, true);
  beam_.pool_score = pooled<float>(slot_allocs_, B, true);
  beam_.pool_n = pooled<int>(slot_allocs_, B, true);
  beam_.complete = pooled<int>(slot_allocs_, B, true);
  beam_.n_complete = pooled<int>(slot_allocs_, 1, true);
}

// Start: rank j in slot c * K + j, S_0 = 0 and the other ranks dead, an empty pool; histories hold valid ids (eot) everywhere, since
// advance_kernel feeds a frozen clip whatever is there
void Engine::beam_begin(int clips, int K) {
  hipStream_t s = stream();
  const int slots = clips * K, Tc = cfg_.n_text_ctx;
  std::vector<int> hist((size_t)slots * Tc, cfg_.eot), ident(slots);
  std::vector<float> S(slots, -INFINITY);
  for (int i = 0; i < slots; ++i) ident[i] = i;
  for (int c = 0; c < clips; ++c) S[(size_t)c * K] = 0.f;
  HIP_CHECK(hipMemcpyAsync(beam_.hist, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(beam_.S, S.data(), (size_t)slots * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(beam_.slot_score, S.data(), (size_t)slots * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(beam_.slot, ident.data(), (size_t)slots * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(beam_.src, ident.data(), (size_t)slots * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(beam_.pool_n, 0, (size_t)clips * 4, s));
  HIP_CHECK(hipMemsetAsync(beam_.pool_len, 0, (size_t)slots * 4, s));
  HIP_CHECK(hipMemsetAsync(beam_.complete, 0, (size_t)clips * 4, s));
  HIP_CHECK(hipMemsetAsync(beam_.n_complete, 0, 4, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (stack vectors)
}

// What follows the logits dump of the step at decode offset `off` (every slot is at the same offset: the loop is lock-step)
void Engine::enqueue_beam_tail(int clips, int K, int off, int max_new, hipStream_t s) {
  const int slots = clips * K, Tc = cfg_.n_text_ctx, H = cfg_.n_text_head;
  const int n = off - 2;  // history length: the step that fed `transcribe` samples the first id
  if (n >= 0) {
    BeamCandParams c{};
    c.logits = d_ts_logits_; c.stride = ts_stride_; c.n_slots = slots;
    c.n_vocab = cfg_.n_vocab; c.eot = cfg_.eot; c.ts_begin = cfg_.no_timestamps + 1;
    c.hist = beam_.hist; c.hist_stride = Tc; c.n_hist = nullptr; c.n = n;
    c.slot_score = beam_.slot_score; c.complete = beam_.complete; c.beam = K; c.n_cand_max = K + 1;
    c.cand_id = beam_.cand_id; c.cand_logprob = beam_.cand_lp; c.n_cand = beam_.n_cand;
    c.suppress = suppress_mask();
    launch_beam_candidates(c, s);
    BeamSelectParams q{};
    q.n_clips = clips; q.beam = K; q.eot = cfg_.eot; q.n = n;
    q.cand_id = beam_.cand_id; q.cand_logprob = beam_.cand_lp; q.n_cand = beam_.n_cand;
    q.S = beam_.S; q.slot = beam_.slot; q.slot_score = beam_.slot_score;
    q.hist = beam_.hist; q.hist_stride = Tc; q.src = beam_.src;
    q.pool_n = beam_.pool_n; q.pool_ids = beam_.pool_ids; q.pool_len = beam_.pool_len; q.pool_score = beam_.pool_score;
    q.complete = beam_.complete; q.n_complete = beam_.n_complete;
    launch_beam_select(q, s);
    if (K > 1) {  // (one hypothesis per clip never moves)
      BeamReorderParams r{};
      r.src = beam_.src; r.n_slots = slots; r.hist = beam_.hist; r.hist_stride = Tc; r.n = n;
      r.k = d_self_k_; r.v = d_self_v_; r.kv_batch_stride = H * layout::kv_head_elems(Tc); r.cap = cap_;
      r.n_layer = cfg_.n_text_layer; r.n_head = H; r.n_ctx_pad = Tc; r.off = off;
      launch_beam_reorder(r, s);
    }
  }
  // advance_kernel in teacher-forcing mode: feeds hist[slot][off - 2] (the prefix before that), never stops a slot
  AdvanceParams a{};
  a.amax_val = d_amax_val_; a.amax_idx = d_amax_idx_; a.n_part = 0; a.amax_stride = n_amax_part_;
  a.n_prefix = 3;
  a.state = d_state_; a.off = d_off_; a.tok = d_tok_; a.done = d_done_; a.n_out = d_nout_; a.out_ids = d_out_ids_; a.batch = slots;
  a.n_ctx = Tc; a.eot = cfg_.eot; a.max_new = max_new; a.n_vocab = cfg_.n_vocab; a.max_new_clip = d_max_new_clip_; a.sot = d_sot_;
  a.forced = beam_.hist; a.n_forced = Tc; a.argmax_dump = nullptr;
  a.tok_emb = tok_emb_; a.pos = dec_pos_; a.x = d_xdec_; a.d_model = cfg_.n_text_state;
  a.done_host = nullptr;
  launch_advance(a, s);
}

// cross K/V of clip c (slot c, where the encoder put it) -> slots [c * K, c * K + K), clips in descending order (common.hpp)
void Engine::beam_spread_cross(int clips, int K) {
  if (K == 1) return;
  const long slot_elems = cfg_.n_text_head * layout::kv_head_elems(t_pad_);
  for (int c = clips - 1; c >= 0; --c)
    launch_beam_spread_cross(d_cross_k_, d_cross_v_, (long)cap_ * slot_elems, slot_elems, cfg_.n_text_layer, c, c * K, K, stream());
}

// The loop over the encoded clips in slots 0 .. clips - 1. Returns the decoder steps run.
int Engine::beam_loop(int clips, int K, int max_new, const BeamResult& out, float* no_speech_logprob, BeamTrace* trace) {
  const int Tc = cfg_.n_text_ctx, nv = cfg_.n_vocab, slots = clips * K;
  if (max_new <= 0 || max_new > Tc - 3) max_new = Tc - 3;
  hipStream_t s = stream();
  // layers + the logits dump from offset 0 on; asked for BEFORE the decode state is set up (step_graph)
  hipGraphExec_t g = step_graph(StepSpec{kDecodeScored, 11}, slots, max_new);
  ensure_beam_buffers();
  beam_spread_cross(clips, K);
  reset_decode_state(slots);
  beam_begin(clips, K);
  const int total = 2 + max_new;
  const int kPoll = 8;  // steps between polls of the completion counter, two deep (greedy_loop)
  hipEvent_t pe[2] = {ev_[3], ev_[4]};
  int steps = 0, polls = 0;
  for (int st = 0; st < total; ++st) {
    HIP_CHECK(hipGraphLaunch(g, s));
    ++steps;
    if (st == 0) launch_row_logprob(d_ts_logits_, ts_stride_, nv, (int)cfg_.ints.at("no_speech"), slots, d_nospeech_, s);
    const int n = st - 2;
    const bool tr = trace && n >= 0 && n < trace->cap;
    if (tr && trace->rows)
      HIP_CHECK(hipMemcpy2DAsync(trace->rows + (size_t)n * slots * nv, (size_t)nv * 4, d_ts_logits_, (size_t)ts_stride_ * 4, (size_t)nv * 4, slots,
                                 hipMemcpyDeviceToHost, s));
    enqueue_beam_tail(clips, K, st, max_new, s);
    if (tr) {
      const int M = K + 1;
      auto get = [&](auto* dst, const auto* src_dev, size_t count) {
        if (dst) HIP_CHECK(hipMemcpyAsync(dst, src_dev, count * 4, hipMemcpyDeviceToHost, s));
      };
      get(trace->cand_id ? trace->cand_id + (size_t)n * slots * M : nullptr, beam_.cand_id, (size_t)slots * M);
      get(trace->cand_logprob ? trace->cand_logprob + (size_t)n * slots * M : nullptr, beam_.cand_lp, (size_t)slots * M);
      get(trace->n_cand ? trace->n_cand + (size_t)n * slots : nullptr, beam_.n_cand, slots);
      get(trace->S ? trace->S + (size_t)n * slots : nullptr, beam_.S, slots);
      get(trace->slot ? trace->slot + (size_t)n * slots : nullptr, beam_.slot, slots);
      get(trace->src ? trace->src + (size_t)n * slots : nullptr, beam_.src, slots);
      get(trace->pool_n ? trace->pool_n + (size_t)n * clips : nullptr, beam_.pool_n, clips);
      if (trace->tok)
        HIP_CHECK(hipMemcpy2DAsync(trace->tok + (size_t)n * slots, 4, beam_.hist + n, (size_t)Tc * 4, 4, slots, hipMemcpyDeviceToHost, s));
    }
    if ((st + 1) % kPoll == 0 && st >= 4) {
      if (polls >= 1) {  // look at the poll issued kPoll steps ago (keeps the queue full)
        HIP_CHECK(hipEventSynchronize(pe[(polls - 1) & 1]));
        if (h_poll_[(polls - 1) & 1] >= clips) break;
      }
      HIP_CHECK(hipMemcpyAsync(&h_poll_[polls & 1], beam_.n_complete, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipEventRecord(pe[polls & 1], s));
      ++polls;
    }
  }
  HIP_CHECK(hipGetLastError());
  const int n_final = std::max(steps - 2, 0);
  if (trace) trace->n_steps = n_final;
  // ---- the state comes back; fill and ranking on the host (beam.hpp)
  std::vector<int32_t> hist((size_t)slots * Tc), pool_ids((size_t)slots * Tc);
  std::vector<int> slot(slots), pool_n(clips), pool_len(slots);
  std::vector<float> S(slots), pool_score(slots), nsp(slots);
  static_assert(sizeof(int) == sizeof(int32_t), "int32_t");
  HIP_CHECK(hipMemcpyAsync(hist.data(), beam_.hist, hist.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(pool_ids.data(), beam_.pool_ids, pool_ids.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(slot.data(), beam_.slot, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(S.data(), beam_.S, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(pool_n.data(), beam_.pool_n, (size_t)clips * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(pool_len.data(), beam_.pool_len, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(pool_score.data(), beam_.pool_score, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(nsp.data(), d_nospeech_, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (int i = 0; i < slots; ++i)
    if (slot[i] < 0 || slot[i] >= slots) throw std::runtime_error("beam search: the rank -> slot map came back out of range");
  const BeamState state{clips, K, n_final, Tc, hist.data(), S.data(), slot.data(), pool_n.data(), pool_ids.data(), pool_len.data(), pool_score.data()};
  beam_finalize(state, out);
  for (int c = 0; no_speech_logprob && c < clips; ++c) no_speech_logprob[c] = nsp[(size_t)c * K];  // the clip's rank-0 slot at offset 0
  return steps;
}

static void check_beam_call(const char* who, int clips, int K, int cap) {
  if (clips < 1) throw std::runtime_error(std::string(who) + ": batch must be >= 1");
  if ((long)clips * K > cap)
    throw std::runtime_error(std::string(who) + ": beam search needs " + std::to_string((long)clips * K) + " slots (" + std::to_string(clips) +
                             " clips x beam_size " + std::to_string(K) + "), the engine holds " + std::to_string(cap) + " (max_batch)");
}

void Engine::run_beam(const float* const* pcm, const int* n_samples, int clips, int beam_size, int max_new, const BeamResult& out,
                      float* no_speech_logprob) {
  require_no_stream("run_beam");
  check_beam_size(beam_size, "run_beam");
  if (clips < 1 || !pcm || !n_samples) throw std::runtime_error("run_beam: bad arguments");
  require_scored_vocab();
  HIP_CHECK(hipSetDevice(device_));
  auto t0 = std::chrono::steady_clock::now();
  ensure_capacity(clips);
  check_beam_call("run_beam", clips, beam_size, cap_);
  hipStream_t s = stream();
  HIP_CHECK(hipEventRecord(ev_[0], s));
  upload_pcm(pcm, n_samples, clips);
  run_frontend(d_pcm_, (int)pcm_stride_, n_samples, clips, false, true);
  HIP_CHECK(hipEventRecord(ev_[1], s));
  run_encoder(clips);
  HIP_CHECK(hipEventRecord(ev_[2], s));
  const int steps = beam_loop(clips, beam_size, max_new, out, no_speech_logprob, nullptr);
  HIP_CHECK(hipEventRecord(ev_[3], s));
  HIP_CHECK(hipEventSynchronize(ev_[3]));
  (void)hipEventElapsedTime(&timings[0], ev_[0], ev_[1]);
  (void)hipEventElapsedTime(&timings[1], ev_[1], ev_[2]);
  (void)hipEventElapsedTime(&timings[2], ev_[2], ev_[3]);
  timings[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  timings[4] = (float)steps;
}

void Engine::decode_beam(int clips, int beam_size, int max_new, const BeamResult& out, float* no_speech_logprob, BeamTrace* trace) {
  require_no_stream("decode_beam");
  check_beam_size(beam_size, "decode_beam");
  require_scored_vocab();
  HIP_CHECK(hipSetDevice(device_));
  check_beam_call("decode_beam", clips, beam_size, cap_);
  if (trace && trace->cap < 0) throw std::runtime_error("decode_beam: trace capacity below 0");
  hipStream_t s = stream();
  HIP_CHECK(hipEventRecord(ev_[2], s));
  const int steps = beam_loop(clips, beam_size, max_new, out, no_speech_logprob, trace);
  HIP_CHECK(hipEventRecord(ev_[3], s));
  HIP_CHECK(hipEventSynchronize(ev_[3]));
  timings[0] = timings[1] = 0.f;
  (void)hipEventElapsedTime(&timings[2], ev_[2], ev_[3]);
  timings[3] = timings[2];
  timings[4] = (float)steps;
}

// The candidates kernel alone, on host rows and histories (tests; callers with logits of their own)
void Engine::beam_candidates(const float* logits, const int32_t* hist, const int* n_hist, int rows, int n_cand_max, int32_t* cand_id,
                             float* cand_logprob, int* n_cand) {
  require_no_stream("beam_candidates");
  require_timestamp_vocab();
  if (rows < 1 || !logits || !hist || !n_hist || !cand_id || !cand_logprob || !n_cand || n_cand_max < 1 || n_cand_max > kBeamMaxCand)
    throw std::runtime_error("beam_candidates: bad arguments (1 .. " + std::to_string(kBeamMaxCand) + " candidates per row)");
  const int M = n_cand_max;
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = stream();
  const StagedRows in = stage_rows("beam_candidates", logits, hist, n_hist, rows, s);
  DeviceArray<float> b_lp = device_array<float>((size_t)rows * M);
  DeviceArray<int> b_id = device_array<int>((size_t)rows * M), b_nc = device_array<int>(rows);
  BeamCandParams c{};
  c.logits = in.logits; c.stride = in.stride; c.n_slots = rows; c.n_vocab = cfg_.n_vocab; c.eot = cfg_.eot; c.ts_begin = cfg_.no_timestamps + 1;
  c.hist = in.hist; c.hist_stride = cfg_.n_text_ctx; c.n_hist = in.n_hist; c.beam = 1; c.n_cand_max = M;
  c.cand_id = b_id; c.cand_logprob = b_lp; c.n_cand = b_nc;
  c.suppress = suppress_mask();
  launch_beam_candidates(c, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(cand_id, b_id, (size_t)rows * M * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cand_logprob, b_lp, (size_t)rows * M * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(n_cand, b_nc, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// The selection kernel alone, on host state (tests). Needs the engine only for its device.
int Engine::beam_select(const BeamSelectIO& io) {
  require_no_stream("beam_select");
  check_beam_size(io.beam, "beam_select");
  const int K = io.beam, M = K + 1, clips = io.clips, slots = clips * K;
  if (clips < 1 || io.n < 0 || io.n >= io.stride || !io.cand_id || !io.cand_logprob || !io.n_cand || !io.hist || !io.S || !io.slot || !io.pool_n ||
      !io.pool_ids || !io.pool_len || !io.pool_score || !io.complete || !io.tok || !io.src || !io.slot_score)
    throw std::runtime_error("beam_select: bad arguments");
  for (int c = 0; c < clips; ++c) {  // the kernel indexes with these
    if (io.pool_n[c] < 0 || io.pool_n[c] > K) throw std::runtime_error("beam_select: pool size out of range");
    unsigned seen = 0;
    for (int r = 0; r < K; ++r) {
      const int t = io.slot[c * K + r] - c * K;
      if (t < 0 || t >= K || (seen >> t & 1)) throw std::runtime_error("beam_select: the ranks of a clip must hold each of its slots once");
      seen |= 1u << t;
    }
  }
  for (int i = 0; i < slots; ++i)
    if (io.n_cand[i] < 0 || io.n_cand[i] > M) throw std::runtime_error("beam_select: candidate count out of range");
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = stream();
  const size_t hs = (size_t)slots * io.stride;
  DeviceArray<int> b_cid = device_array<int>((size_t)slots * M), b_nc = device_array<int>(slots), b_hist = device_array<int>(hs),
                   b_slot = device_array<int>(slots), b_src = device_array<int>(slots), b_pn = device_array<int>(clips),
                   b_pids = device_array<int>(hs), b_plen = device_array<int>(slots), b_comp = device_array<int>(clips),
                   b_ncomp = device_array<int>(1, true);
  DeviceArray<float> b_clp = device_array<float>((size_t)slots * M), b_S = device_array<float>(slots), b_ss = device_array<float>(slots, true),
                     b_ps = device_array<float>(slots);
  auto up = [&](void* dst, const void* src, size_t count) { HIP_CHECK(hipMemcpyAsync(dst, src, count * 4, hipMemcpyHostToDevice, s)); };
  up(b_cid, io.cand_id, (size_t)slots * M); up(b_clp, io.cand_logprob, (size_t)slots * M); up(b_nc, io.n_cand, slots);
  up(b_hist, io.hist, hs); up(b_S, io.S, slots); up(b_slot, io.slot, slots); up(b_pn, io.pool_n, clips);
  up(b_pids, io.pool_ids, hs); up(b_plen, io.pool_len, slots); up(b_ps, io.pool_score, slots); up(b_comp, io.complete, clips);
  BeamSelectParams q{};
  q.n_clips = clips; q.beam = K; q.eot = io.eot; q.n = io.n;
  q.cand_id = b_cid; q.cand_logprob = b_clp; q.n_cand = b_nc;
  q.S = b_S; q.slot = b_slot; q.slot_score = b_ss; q.hist = b_hist; q.hist_stride = io.stride; q.src = b_src;
  q.pool_n = b_pn; q.pool_ids = b_pids; q.pool_len = b_plen; q.pool_score = b_ps; q.complete = b_comp; q.n_complete = b_ncomp;
  launch_beam_select(q, s);
  HIP_CHECK(hipGetLastError());
  int n_complete = 0;
  auto down = [&](void* dst, const void* src, size_t count) { HIP_CHECK(hipMemcpyAsync(dst, src, count * 4, hipMemcpyDeviceToHost, s)); };
  down(io.S, b_S, slots); down(io.slot, b_slot, slots); down(io.pool_n, b_pn, clips); down(io.pool_ids, b_pids, hs);
  down(io.pool_len, b_plen, slots); down(io.pool_score, b_ps, slots); down(io.complete, b_comp, clips); down(io.src, b_src, slots);
  down(io.slot_score, b_ss, slots); down(&n_complete, b_ncomp, 1);
  HIP_CHECK(hipMemcpy2DAsync(io.tok, 4, b_hist + io.n, (size_t)io.stride * 4, 4, slots, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return n_complete;
}

}  // inline namespace AXW_NS
}  // namespace axw
