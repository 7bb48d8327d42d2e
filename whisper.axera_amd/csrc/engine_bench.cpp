// engine_bench.cpp — axw::Engine: the hooks that are not the product. AX_WHISPER_Bench times one stage of the pipeline in
// isolation (one private function per target), AX_WHISPER_ScanStored16 looks for non-finite values in what the engine stores.
#include "engine_impl.hpp"

#include "resample.hpp"

namespace axw {
inline namespace AXW_NS {

// ------------------------------------------------------------------------------ stored 16-bit tensors: non-finite scan
// (parity battery under trained-model statistics: outlier channels, FFN hidden values in the thousands — a half tensor
// that overflowed would show here even where the logits still look plausible)
__global__ static void scan16_kernel(const h16* __restrict__ p, size_t n, unsigned long long* bad, unsigned* maxbits) {
  unsigned long long nb = 0;
  float mx = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = (float)p[i];
    if (v != v || fabsf(v) > 3.0e38f) ++nb; else mx = fmaxf(mx, fabsf(v));
  }
  if (nb) atomicAdd(bad, nb);
  atomicMax(maxbits, __float_as_uint(mx));  // non-negative floats order like their bit patterns
}

int Engine::scan_stored16(int batch, int n_max, char (*names)[32], long long* nonfinite, float* maxabs) {
  require_no_stream("scan_stored16");
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  if (batch < 1 || batch > cap_) throw std::runtime_error("scan_stored16: batch outside the allocated slots");
  const size_t B = batch, d = cfg_.n_text_state, T = cfg_.n_audio_ctx, L = cfg_.n_text_layer, H = cfg_.n_text_head, Tc = cfg_.n_text_ctx;
  struct Buf { const char* name; const h16* p; size_t n; };
  std::vector<Buf> bufs = {
      {"enc.mel", d_mel_tm_, B * mel_rows_ * cfg_.n_mels}, {"enc.conv1", d_h1_, B * h1_rows_ * d}, {"enc.ln", d_ln_, B * T * d},
      {"enc.q", d_q_, B * T * d}, {"enc.k", d_k_, B * T * d}, {"enc.vt", d_vt_, B * d * t_pad_}, {"enc.attn", d_attn_, B * T * d},
      {"enc.ffn_hidden", d_ffn_, B * T * 4 * d},
      {"cross_k", d_cross_k_, L * (size_t)cap_ * H * layout::kv_head_elems(t_pad_)}, {"cross_v", d_cross_v_, L * (size_t)cap_ * H * layout::kv_head_elems(t_pad_)},
      {"self_k", d_self_k_, L * (size_t)cap_ * H * layout::kv_head_elems(Tc)}, {"self_v", d_self_v_, L * (size_t)cap_ * H * layout::kv_head_elems(Tc)},
      {"dec.act_hi", d_act_[0], (size_t)layout::pair_elems(d / 32, nbs_)}, {"dec.act_lo", d_act_[1], (size_t)layout::pair_elems(d / 32, nbs_)},
      {"dec.att_hi", d_att_[0], (size_t)layout::pair_elems(d / 32, nbs_)}, {"dec.att_lo", d_att_[1], (size_t)layout::pair_elems(d / 32, nbs_)},
      {"dec.hid_hi", d_hidp_[0], (size_t)layout::pair_elems(4 * d / 32, nbs_)}, {"dec.hid_lo", d_hidp_[1], (size_t)layout::pair_elems(4 * d / 32, nbs_)},
  };
  if (d_self_k1_) {
    bufs.push_back({"persist.self_k1", d_self_k1_, self1_bytes_ / 2 * (size_t)std::max(persist_max_clips_ - 1, 1)});
    bufs.push_back({"persist.self_v1", d_self_v1_, self1_bytes_ / 2 * (size_t)std::max(persist_max_clips_ - 1, 1)});
  }
  const int n = std::min<int>(n_max, (int)bufs.size());
  const DeviceArray<unsigned long long> d_res = device_array<unsigned long long>((size_t)n * 2, true);
  hipStream_t s = stream();
  for (int i = 0; i < n; ++i)
    scan16_kernel<<<1024, 256, 0, s>>>(bufs[i].p, bufs[i].n, d_res + 2 * i, reinterpret_cast<unsigned*>(d_res + 2 * i + 1));
  std::vector<unsigned long long> h((size_t)n * 2);
  HIP_CHECK(hipMemcpyAsync(h.data(), d_res, (size_t)n * 16, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) {
    snprintf(names[i], 32, "%s", bufs[i].name);
    nonfinite[i] = (long long)h[2 * i];
    const unsigned bits = (unsigned)(h[2 * i + 1] & 0xffffffffu);
    memcpy(&maxabs[i], &bits, 4);
  }
  return n;
}

// ------------------------------------------------------------------------------ the later clips' caches of a multi-clip launch
// back to [n_text_layer][512][d] fp32 from the blocked K / transposed V of clip `clip` (1, 2) of the last two- or three-clip
// persistent launch (decode_persistent2.hip: [layer * n_head + head][8 blocks][4096] per clip); GetSelfKV's twin. Every block is
// returned, so a test sees the rows no step wrote, too.
void Engine::get_persistent_self_kv(int clip, float* k_out, float* v_out) {
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  if (clip < 1 || clip > 2) throw std::runtime_error("get_persistent_self_kv: clip is 1 or 2 (clip 0's cache is on-chip)");
  if (persist_max_clips_ <= clip || !d_self_k1_ || !d_self_v1_)
    throw std::runtime_error("get_persistent_self_kv: this handle runs " + std::to_string(persist_max_clips_) + " clip(s) per persistent launch, there is no cache of clip " +
                             std::to_string(clip));
  const int d = cfg_.n_text_state, H = cfg_.n_text_head, L = cfg_.n_text_layer;
  constexpr int kBlocks = 8, kRows = kBlocks * layout::kKvBlockKeys;
  const size_t unit = (size_t)kBlocks * layout::kKvBlockElems, per = (size_t)L * H * unit;
  if (per * 2 != self1_bytes_) throw std::runtime_error("get_persistent_self_kv: cache size mismatch");
  std::vector<uint16_t> hk(per), hv(per);
  HIP_CHECK(hipStreamSynchronize(stream()));
  HIP_CHECK(hipMemcpy(hk.data(), d_self_k1_ + (size_t)(clip - 1) * per, per * 2, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hv.data(), d_self_v1_ + (size_t)(clip - 1) * per, per * 2, hipMemcpyDeviceToHost));
  for (int l = 0; l < L; ++l)
    for (int h = 0; h < H; ++h) {
      const size_t u = ((size_t)l * H + h) * unit;
      for (int t = 0; t < kRows; ++t)
        for (int c = 0; c < layout::kKvDim; ++c) {
          k_out[((size_t)l * kRows + t) * d + h * 64 + c] = h16_bits_to_float(hk[u + layout::k_index(t, c)]);
          v_out[((size_t)l * kRows + t) * d + h * 64 + c] = h16_bits_to_float(hv[u + layout::vt_index(t, c)]);
        }
    }
}

// ------------------------------------------------------------------------------ bench
float Engine::bench(const std::string& what, int batch, int arg, int iters) {
  require_no_stream("bench");
  if (what == "queue_probe") return (float)queue_probe_mask();
  HIP_CHECK(hipSetDevice(device_));
  ensure_capacity(batch);
  if (what == "decode_step" || what == "decode_gemv" || what == "decode_attn" || what == "decode_step_ts" || what == "decode_step_ts_scored" ||
      what == "decode_step_ts_sampled" || what == "stream_step_ts")
    return bench_decode_step(what, batch, arg, iters);
  if (what == "decode_step_beam") return bench_decode_step_beam(batch, arg, iters);
  if (what == "attn_stamp") return bench_attn_stamp(batch, arg, iters);
  if (what == "encoder") return bench_encoder(batch, iters);
  if (what == "cross_kv_quant") return bench_cross_kv_quant(batch, iters);
  if (what == "frontend") return bench_frontend(batch, iters);
  if (what == "resample") return bench_resample(batch, arg, iters);
  if (what == "frontend_long") return bench_frontend_long(batch, arg, iters);
  if (what == "long_cut_plan") return bench_long_cut_plan(batch, arg, iters);
  if (what == "prefill" || what == "prefill_pass" || what == "prefill_step") return bench_prefill(what, batch, arg, iters);
  if (what == "detect_language") return bench_detect_language(batch, arg, iters);
  if (what == "word_align" || what == "word_align_host") return bench_word_align(what, batch, arg, iters);
  if (what == "word_logprob" || what == "word_logprob_rows") return bench_word_logprob(what, batch, arg, iters);
  throw std::runtime_error("bench: unknown target '" + what + "'");
}

// what run() enqueues on s, between two events of this call
template <class Fn>
static float timed_ms(hipStream_t s, Fn&& run) {
  const Event a = make_event(), b = make_event();
  HIP_CHECK(hipEventRecord(a, s));
  run();
  HIP_CHECK(hipEventRecord(b, s));
  HIP_CHECK(hipEventSynchronize(b));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  return ms;
}

// prefill: reset + prefill_prompts (tables, route, no-speech row, hand-over) of `batch` slots, every one with a context of L = arg
// positions, by the handle's route; prefill_pass / prefill_step: by that route whatever the handle's is (A/B on one handle).
// The slots' cross K/V is whatever the last encoder pass left (zeros on a fresh handle): the work does not depend on it.
float Engine::bench_prefill(const std::string& what, int batch, int arg, int iters) {
  require_scored_vocab();
  const int keep = cfg_.n_text_ctx / 2 - 1, P = std::max(1, std::min(arg - 3, keep));
  std::vector<int32_t> ids((size_t)batch * P);
  unsigned x = 12345u;
  for (auto& v : ids) { x = x * 1664525u + 1013904223u; v = (int32_t)((x >> 8) % (unsigned)cfg_.eot); }
  const std::vector<int> n_prompt(batch, P);
  const ClipContexts ctx{PromptSpec{ids.data(), P, n_prompt.data()}};
  const ScopedSet<int> scope(prefill_force_, what == "prefill_pass" ? 0 : what == "prefill_step" ? 1 : -1);
  hipStream_t s = stream();
  reset_decode_state(batch);
  prefill_prompts(batch, ctx, false, true);  // warm: scratch, score arrays
  return timed_ms(s, [&] {
    for (int i = 0; i < iters; ++i) {
      reset_decode_state(batch);
      prefill_prompts(batch, ctx, false, true);
    }
  });
}

// detect_language: detection of `batch` slots as AX_WHISPER_DetectLanguageStage runs it (reset, the [sot] position, the pick, the
// results on the host); arg 0: the prefill route (one step's layers + the detection kernel), 1: the step-fed route (one decoder step with
// the logits dump, the pick on the host), anything else: the handle's route. Cross K/V as bench "prefill" finds it.
float Engine::bench_detect_language(int batch, int arg, int iters) {
  require_timestamp_vocab();
  const ScopedSet<int> scope(prefill_force_, arg == 0 ? 0 : arg == 1 ? 1 : -1);
  std::vector<int> idx(batch);
  const LangResult out{idx.data(), nullptr, nullptr};
  detect_language_stage(batch, out);  // warm: scratch, the language id list
  return timed_ms(stream(), [&] {
    for (int i = 0; i < iters; ++i) detect_language_stage(batch, out);
  });
}

// word_align / word_align_host: align_tokens of `batch` slots, every one with arg text ids against all n_audio_ctx frames, by the
// kernels / by the host route whatever the handle's is (A/B on one handle). Host time included: both routes end on the host.
// Cross K/V as bench "prefill" finds it.
float Engine::bench_word_align(const std::string& what, int batch, int arg, int iters) {
  require_timestamp_vocab();
  const int n = std::max(1, std::min(arg, cfg_.n_text_ctx - 5));
  std::vector<int32_t> ids((size_t)batch * n);
  unsigned x = 12345u;
  for (auto& v : ids) { x = x * 1664525u + 1013904223u; v = (int32_t)((x >> 8) % (unsigned)cfg_.eot); }
  const std::vector<int> n_ids(batch, n), frames(batch, 2 * cfg_.n_audio_ctx);
  std::vector<int> jump((size_t)batch * (n + 1));
  std::vector<float> lp((size_t)batch * n);
  const AlignRequest rq{batch, ids.data(), n, n_ids.data(), frames.data(), nullptr, nullptr, jump.data(), lp.data(), nullptr, 0, 0};
  const ScopedSet<int> scope(align_force_, what == "word_align" ? 0 : 1);
  align_tokens(rq);  // warm: the prefill scratch
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) align_tokens(rq);
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// word_logprob / word_logprob_rows: the token probabilities of `batch` clips x arg ids alone (batch * arg final residual rows, seeded,
// already on the device), by the fused kernel / by the logits launch four rows at a time (A/B on one handle). Scratch allocation and
// the closing synchronisation are inside, as align_tokens pays them.
float Engine::bench_word_logprob(const std::string& what, int batch, int arg, int iters) {
  require_timestamp_vocab();
  const int n = batch * std::max(1, std::min(arg, cfg_.n_text_ctx - 5)), d = cfg_.n_text_state;
  std::vector<float> hx((size_t)n * d);
  std::vector<int> hid(n);
  unsigned x = 12345u;
  for (auto& v : hx) { x = x * 1664525u + 1013904223u; v = (float)(int)((x >> 8) & 0xffff) / 16384.f - 2.f; }
  for (auto& v : hid) { x = x * 1664525u + 1013904223u; v = (int)((x >> 8) % (unsigned)cfg_.eot); }
  hipStream_t s = stream();
  DeviceArray<float> dx = device_array<float>(hx.size()), lp = device_array<float>(n);
  DeviceArray<int> did = device_array<int>(n);
  HIP_CHECK(hipMemcpy(dx, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(did, hid.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  const bool fused = what == "word_logprob";
  auto run = [&] { fused ? token_logprob_fused(dx, nullptr, did, n, lp, s) : token_logprob_rows(dx, nullptr, did, n, lp, s); };
  run();  // warm
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) run();
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// decode_gemv / decode_attn: the same captured step with only the GEMV / only the attention launches;
// decode_step_ts: the whole step in timestamp mode (logits dump + rules kernel); decode_step_ts_scored: with the scored rules kernel;
// decode_step_ts_sampled: with the sampled rules kernel, every clip at temperature AX_WHISPER_BENCH_TEMPERATURE (default 1);
// stream_step_ts: the scored step of the slot stream in timestamp mode (stream_rules_kernel, a prefix per slot), the same placement
float Engine::bench_decode_step(const std::string& what, int batch, int arg, int iters) {
  const bool sampled = what == "decode_step_ts_sampled";
  const bool slots = what == "stream_step_ts";
  const bool whole = what == "decode_step" || what == "decode_step_ts" || what == "decode_step_ts_scored" || sampled || slots;
  if (what == "decode_step_ts") require_timestamp_vocab();
  if (what == "decode_step_ts_scored" || sampled || slots) require_scored_vocab();
  StepSpec spec = step_spec(what == "decode_step_ts" ? kDecodeTimestamps : (what == "decode_step_ts_scored" || slots) ? kDecodeScored : sampled ? kDecodeSampled : kDecodePlain);
  if (slots) {
    if (cfg_.lang_tokens.empty()) throw std::runtime_error("bench stream_step_ts: the config lists no languages");
    ensure_stream_ts();
    spec.slots = true;
  }
  if (sampled) {
    const char* e = getenv("AX_WHISPER_BENCH_TEMPERATURE");
    const std::vector<float> temps(batch, e ? (float)atof(e) : 1.f);
    std::vector<uint64_t> streams(batch);
    for (int b = 0; b < batch; ++b) streams[b] = (uint64_t)b;
    upload_sample(SampleSpec{temps.data(), streams.data(), 1}, batch);
  }
  spec.mask = whole ? 15 : (what == "decode_gemv" ? 1 : 2);
  hipStream_t s = stream();
  const int Tc = cfg_.n_text_ctx;
  reset_decode_state(batch);
  const StepGraphRef g = step_graph(spec, batch, Tc - 4);
  arg = std::max(0, std::min(arg, Tc - 1 - iters));
  DecState st{arg, 0, 0, 0};
  std::vector<int> offs(batch, arg);  // every slot at position `arg`
  HIP_CHECK(hipMemcpy(d_state_, &st, sizeof(st), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_off_, offs.data(), (size_t)batch * 4, hipMemcpyHostToDevice));
  launch_step_graph(g, s);  // warm
  st.step = arg;
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipMemcpy(d_state_, &st, sizeof(st), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_off_, offs.data(), (size_t)batch * 4, hipMemcpyHostToDevice));
  return timed_ms(s, [&] { for (int i = 0; i < iters; ++i) launch_step_graph(g, s); });
}

// bench "decode_step_beam": the beam step (graph up to the logits dump + the four launches behind it) of `slots` slots in groups of
// beam_size, from decode offset 224 (or what the context allows) on, one offset further per iteration. The pass runs twice from the
// same state (zeroed self-attention caches, the start state of a decode placed at that offset): once timed, once more with the
// reorder's source map read back after every iteration, so that the figure has a known meaning — GetConfigInt
// "beam_bench_moved_slots": slots the reorder launch copied, summed over the iterations; "beam_bench_iters": iterations run;
// "beam_bench_complete_clips": clips complete at the end (their kernels return at once).
float Engine::bench_decode_step_beam(int slots, int beam_size, int iters) {
  if (beam_size < 1 || beam_size > kBeamMax) throw std::runtime_error("bench decode_step_beam: arg is the beam size, 1 .. " + std::to_string(kBeamMax));
  require_scored_vocab();
  if (slots < beam_size || slots % beam_size != 0) throw std::runtime_error("bench decode_step_beam: batch must be a multiple of the beam size");
  const int clips = slots / beam_size, Tc = cfg_.n_text_ctx;
  hipStream_t s = stream();
  hipGraphExec_t g = step_graph(StepSpec{kDecodeScored, 11}, slots, Tc - 3);
  ensure_beam_buffers();
  const int off0 = std::max(2, std::min(224, Tc - 2 - iters));
  DecState st{off0, 0, 0, 0};
  std::vector<int> offs(slots, off0), src(slots);
  const size_t self_bytes = (size_t)cfg_.n_text_layer * cap_ * cfg_.n_text_head * layout::kv_head_elems(Tc) * sizeof(h16);
  auto place = [&] {
    HIP_CHECK(hipMemcpyAsync(d_state_, &st, sizeof(st), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_off_, offs.data(), (size_t)slots * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  };
  long moved = 0;
  int ran = 0;
  auto pass = [&](bool count) {
    HIP_CHECK(hipMemsetAsync(d_self_k_, 0, self_bytes, s));
    HIP_CHECK(hipMemsetAsync(d_self_v_, 0, self_bytes, s));
    reset_decode_state(slots);
    beam_begin(clips, beam_size);
    place();
    HIP_CHECK(hipGraphLaunch(g, s));  // warm
    enqueue_beam_tail(clips, beam_size, off0, Tc - 3, s);
    HIP_CHECK(hipStreamSynchronize(s));
    place();
    const Event a = make_event(), b = make_event();
    HIP_CHECK(hipEventRecord(a, s));
    for (int i = 0; i < iters && off0 + i < Tc - 1; ++i) {
      HIP_CHECK(hipGraphLaunch(g, s));
      enqueue_beam_tail(clips, beam_size, off0 + i, Tc - 3, s);
      if (count) {
        HIP_CHECK(hipMemcpyAsync(src.data(), beam_.src, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (int k = 0; k < slots; ++k) moved += src[k] != k;
        ++ran;
      }
    }
    HIP_CHECK(hipEventRecord(b, s));
    HIP_CHECK(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
  };
  const float ms = pass(false);
  (void)pass(true);
  int n_complete = 0;
  HIP_CHECK(hipMemcpyAsync(&n_complete, beam_.n_complete, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  cfg_.ints["beam_bench_moved_slots"] = moved;
  cfg_.ints["beam_bench_iters"] = ran;
  cfg_.ints["beam_bench_complete_clips"] = n_complete;
  return ms;
}

// One replay of the production step graph (all launches, every branch) at decode offset `arg` whose decode_attention
// launches stamp their own {first workgroup start, last workgroup end}; the table goes to $AX_WHISPER_ATTN_STAMP
// (default attn_stamps.csv). Returns the length of the UNION of the attention intervals in ms: K/V bytes of the step
// over that time is the rate the attention launches achieve while the other branch's launches run beside them.
float Engine::bench_attn_stamp(int batch, int arg, int iters) {
  if (batch <= gemv_max_) throw std::runtime_error("bench attn_stamp: the batched decode sequences only (3+ clips)");
  // (a launch has batch * heads workgroups, or up to 640 when few (clip, head) pairs are split along the keys)
  if (std::max<long>((long)batch * cfg_.n_text_head, 640) > (long)kStampWgs) throw std::runtime_error("bench attn_stamp: too many workgroups per launch");
  const size_t n_words = (size_t)2 * kStampWgs * kStampLaunches;
  if (!d_stamp_) {
    std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));  // an allocation (iengine.hpp)
    d_stamp_ = device_array<unsigned long long>(n_words, true);
  }
  StepSpec spec = step_spec();
  spec.mask = 15 | 16;
  hipStream_t s = stream();
  const int Tc = cfg_.n_text_ctx;
  reset_decode_state(batch);
  drop_step_graph(spec, batch, Tc - 4);  // captured anew: the capture fills stamp_meta_
  stamp_meta_.clear();
  hipGraphExec_t g = step_graph(spec, batch, Tc - 4);
  const int warm_replays = iters >= 100 ? iters - 100 : 0;
  arg = std::max(0, std::min(arg, Tc - 4 - warm_replays));  // every replay advances the clips by one position
  DecState st{arg, 0, 0, 0};
  std::vector<int> offs(batch, arg);
  std::vector<unsigned long long> raw(n_words), got(2 * kStampLaunches);
  std::vector<std::pair<double, double>> iv;
  double best_union = 0.0;
  std::string table;
  float step_ms = 0.f;
  for (int rep = 0; rep < 3; ++rep) {  // the first repetitions warm the caches; the last one is reported
    HIP_CHECK(hipMemcpy(d_state_, &st, sizeof(st), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_off_, offs.data(), (size_t)batch * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d_stamp_, 0, n_words * 8));
    HIP_CHECK(hipDeviceSynchronize());
    // arg2 (iters >= 100): `iters - 100` replays back to back BEFORE the stamped one, so that the stamped step starts the way
    // a step of the loop does — behind its predecessor, both branches already queued (a lone replay's second branch starts
    // ~250 us late: the host is still enqueuing its nodes)
    step_ms = timed_ms(s, [&] { for (int k = 0; k < warm_replays + 1; ++k) HIP_CHECK(hipGraphLaunch(g, s)); });
    HIP_CHECK(hipMemcpy(raw.data(), d_stamp_, n_words * 8, hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < stamp_meta_.size(); ++i) {  // a launch = the earliest start and the latest end of its workgroups
    unsigned long long lo = ~0ull, hi = 0ull;
    for (size_t w = 0; w < kStampWgs; ++w) {
      const unsigned long long bg = raw[(i * kStampWgs + w) * 2], en = raw[(i * kStampWgs + w) * 2 + 1];
      if (bg) lo = std::min(lo, bg);
      hi = std::max(hi, en);
    }
    got[2 * i] = lo;
    got[2 * i + 1] = hi;
  }
  unsigned long long t0 = ~0ull;
  for (size_t i = 0; i < stamp_meta_.size(); ++i) t0 = std::min(t0, got[2 * i]);
  const double keys_self = arg + 1, d_ = cfg_.n_text_state;
  char line[256];
  snprintf(line, sizeof line, "# batch %d, decode offset %d, %zu attention launches, %d replays back to back before the stamped one (all %d: %.3f us, hipEvents); times in us from the stamped step's first attention start (100 MHz wall clock)\n",
           batch, arg, stamp_meta_.size(), warm_replays, warm_replays + 1, step_ms * 1e3);
  table += line;
  table += "launch,kind,layer,first_clip,clips,begin_us,end_us,duration_us,kv_bytes,GBs\n";
  for (size_t i = 0; i < stamp_meta_.size(); ++i) {
    const StampMeta& m = stamp_meta_[i];
    const double bg = (double)(got[2 * i] - t0) * 0.01, en = (double)(got[2 * i + 1] - t0) * 0.01;
    static const char* const kinds[] = {"self", "cross", "qkv", "o", "co", "fc1", "fc2", "cq"};
    const bool is_attn = m.cross <= 1;
    const double bytes = is_attn ? (double)m.nb * 2.0 * 2.0 * d_ * (m.cross ? (double)cfg_.n_audio_ctx : keys_self) : 0.0;
    if (is_attn) iv.push_back({bg, en});
    snprintf(line, sizeof line, "%zu,%s,%d,%d,%d,%.2f,%.2f,%.2f,%.0f,%.1f\n", i, kinds[m.cross & 7], m.layer, m.b0, m.nb, bg, en, en - bg, bytes,
             en > bg ? bytes / ((en - bg) * 1e-6) / 1e9 : 0.0);
    table += line;
  }
  std::sort(iv.begin(), iv.end());
  double cur_b = -1, cur_e = -1;
  for (auto& x : iv) {
    if (x.first > cur_e) { best_union += cur_e - cur_b; cur_b = x.first; cur_e = x.second; }
    else cur_e = std::max(cur_e, x.second);
  }
  best_union += cur_e - cur_b;
  snprintf(line, sizeof line, "# union of the attention intervals: %.2f us\n", best_union);
  table += line;
  const char* path = getenv("AX_WHISPER_ATTN_STAMP");
  if (FILE* f = fopen(path ? path : "attn_stamps.csv", "w")) { fputs(table.c_str(), f); fclose(f); }
  drop_step_graph(spec, batch, Tc - 4);
  return (float)(best_union * 1e-3);
}

float Engine::bench_encoder(int batch, int iters) {
  run_encoder(batch);
  return timed_ms(stream(), [&] { for (int i = 0; i < iters; ++i) run_encoder(batch); });
}

// the quantise kernel alone over `batch` slots' h16 cross K/V as it stands (an fp8 handle only)
float Engine::bench_cross_kv_quant(int batch, int iters) {
  if (!cross_fp8_) throw std::runtime_error("bench cross_kv_quant: the handle was not made under AX_WHISPER_CROSS_KV=fp8");
  enqueue_cross_kv_quantize(batch, nullptr, stream());
  return timed_ms(stream(), [&] { for (int i = 0; i < iters; ++i) enqueue_cross_kv_quantize(batch, nullptr, stream()); });
}

float Engine::bench_frontend(int batch, int iters) {
  std::vector<int> ns(batch, 480000);
  run_frontend(d_pcm_, (int)pcm_stride_, ns.data(), batch, false);
  return timed_ms(stream(), [&] { for (int i = 0; i < iters; ++i) run_frontend(d_pcm_, (int)pcm_stride_, ns.data(), batch, false); });
}

// the resample kernel over `batch` clips of 30 s (silence) at `rate` Hz into the staging rows, as upload_pcm launches it
float Engine::bench_resample(int batch, int rate, int iters) {
  if (rate == resample::kTargetRate) throw std::runtime_error("bench resample: arg = the clips' sample rate, other than 16000");
  const RateTable& t = rate_table(rate);
  const int n = 30 * rate;
  std::string err;
  const int n_out = (int)resample::resampled_length(n, rate, err);
  ensure_resample_staging((size_t)batch * n, batch);
  for (int b = 0; b < batch; ++b) h_rs_clips_[b] = ResampleClip{(long long)b * n, 0, t.tab_off, n, n_out, t.L, t.M, t.K, b};
  hipStream_t s = stream();
  HIP_CHECK(hipMemsetAsync(d_raw_, 0, (size_t)batch * n * 4, s));
  HIP_CHECK(hipMemcpyAsync(d_rs_clips_, h_rs_clips_, (size_t)batch * sizeof(ResampleClip), hipMemcpyHostToDevice, s));
  ResampleParams p{};
  p.in = d_raw_; p.tables = d_rs_tables_; p.clips = d_rs_clips_; p.batch = batch;
  p.out = d_pcm_; p.stride = (int)pcm_stride_; p.max_out = n_out;
  launch_resample(p, s);
  return timed_ms(s, [&] { for (int i = 0; i < iters; ++i) launch_resample(p, s); });
}

// whole-file front-end of `batch` files of `arg` seconds (silence) + one window kernel over all of them
float Engine::bench_frontend_long(int batch, int arg, int iters) {
  if (arg < 1 || arg > 33554) throw std::runtime_error("bench frontend_long: arg = seconds of audio per file, 1 .. 33554");
  std::vector<int> ns(batch, arg * 16000), files(batch), seeks(batch, 0);
  for (int i = 0; i < batch; ++i) files[i] = i;
  long_prepare(nullptr, ns.data(), batch, batch);  // allocates, fills, and runs the front-end once (warm)
  long_windows_to_slots(files.data(), seeks.data(), batch, false);
  FrontendParams p{};
  p.pcm = long_.pcm; p.n_samples = long_.n_samples; p.batch = batch; p.n_mels = cfg_.n_mels;
  p.twiddle = twiddle_; p.window = window_; p.mel_basis = mel_basis_t_;
  p.gmax = long_.gmax; p.max_frames = 1 + ns[0] / kHop;
  const LongStoreParams ls{long_.pcm_off, long_.frame_off, long_.store};
  const float ms = timed_ms(stream(), [&] {
    for (int i = 0; i < iters; ++i) {
      launch_frontend_long(p, ls, stream());
      long_windows_to_slots(files.data(), seeks.data(), batch, false);
    }
  });
  long_release();
  return ms;
}

// chunked long-form: levels kernel + plan kernels over `batch` resident files of `arg` seconds, default parameters. The files are a
// ramp (silence would make every level equal), so the scans meet distinct values; what is timed does not depend on them.
float Engine::bench_long_cut_plan(int batch, int arg, int iters) {
  if (arg < 1 || arg > 33554) throw std::runtime_error("bench long_cut_plan: arg = seconds of audio per file, 1 .. 33554");
  std::vector<int> ns(batch, arg * 16000);
  std::vector<float> ramp((size_t)arg * 16000);
  for (size_t i = 0; i < ramp.size(); ++i) ramp[i] = 0.5f * std::sin(0.05f * (float)(i % 40000)) * (float)(1 + i % 7919) / 7919.f;
  std::vector<const float*> files(batch, ramp.data());
  const CutParams cut;
  long_prepare(files.data(), ns.data(), batch, 1, &cut, false);
  long_plan(cut);  // warm
  const float ms = timed_ms(stream(), [&] { for (int i = 0; i < iters; ++i) long_plan(cut); });
  long_release();
  return ms;
}

}  // inline namespace AXW_NS
}  // namespace axw
