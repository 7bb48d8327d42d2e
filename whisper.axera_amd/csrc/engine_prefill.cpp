// engine_prefill.cpp — axw::Engine: prompt conditioning (DESIGN.md "Prompt conditioning"). prefill_prompts() is the ONE place a
// prompt enters the engine: between reset_decode_state and the first decoder step it brings every prompted slot to the state
// "context [sot_prev, prompt, sot, language] cached, `transcribe` about to be fed at offset L = P + 3", after which the existing
// steps (logits, rules, advance) run unchanged. Slots without a prompt are not touched.
// Two routes lead to that state: the prefill pass (decode_prefill.hip + the encoder's GEMM / LayerNorm, all rows at once) and the
// step-fed route (AX_WHISPER_PREFILL=step: one existing decoder step per position; the yardstick for error and time).
// Out of scope: prompts under beam search, in the Stream* slots and in the persistent launches; best_of above 1.
#include "engine_impl.hpp"

#include <climits>

namespace axw {
inline namespace AXW_NS {

namespace {
// the prompted clips of one call, as the kernels' tables want them
struct PromptPlan {
  std::vector<int> ctx, row_pos, row_slot;             // per row
  std::vector<int> row0, len, slot, sot_row, n_kept;   // per prompted clip
  int rows = 0, max_len = 0;
  int clips() const { return (int)slot.size(); }
};
}  // namespace

// prompts.n_prompt[b] ids of clip b at prompts.ids + b * prompts.stride; truncated to their last n_text_ctx / 2 - 1 (openai-whisper)
static PromptPlan plan_prompts(const ModelConfig& cfg, const int* sot_seq, int batch, const IEngine::PromptSpec& pr) {
  if (!pr.n_prompt) throw std::runtime_error("prefill_prompts: no prompt lengths");
  const auto it = cfg.ints.find("sot_prev");
  if (it == cfg.ints.end() || it->second < 0 || it->second >= cfg.n_vocab) throw std::runtime_error("prompted decode needs a sot_prev id inside the vocabulary");
  const int sot_prev = (int)it->second, keep = cfg.n_text_ctx / 2 - 1, ts_begin = cfg.no_timestamps + 1;
  PromptPlan pl;
  for (int b = 0; b < batch; ++b) {
    const int n = pr.n_prompt[b];
    if (n < 0 || n > pr.stride) throw std::runtime_error("prefill_prompts: prompt length " + std::to_string(n) + " of clip " + std::to_string(b) + " out of range");
    if (n == 0) continue;
    if (!pr.ids) throw std::runtime_error("prefill_prompts: no prompt ids");
    const int P = std::min(n, keep);
    const int32_t* src = pr.ids + (size_t)b * pr.stride + (n - P);
    for (int i = 0; i < P; ++i)
      if (src[i] < 0 || src[i] >= cfg.n_vocab || (src[i] >= cfg.eot && src[i] < ts_begin))
        throw std::runtime_error("prefill_prompts: id " + std::to_string(src[i]) + " of clip " + std::to_string(b) + " is neither text nor a timestamp");
    const int L = P + 3;
    if (L + 1 > cfg.n_text_ctx) throw std::runtime_error("prefill_prompts: the prompt leaves no room in the context");
    pl.row0.push_back(pl.rows); pl.len.push_back(L); pl.slot.push_back(b); pl.sot_row.push_back(pl.rows + P + 1); pl.n_kept.push_back(P);
    for (int i = 0; i < L; ++i) {
      pl.ctx.push_back(i == 0 ? sot_prev : i <= P ? (int)src[i - 1] : sot_seq[i - P - 1]);
      pl.row_pos.push_back(i);
      pl.row_slot.push_back(b);
    }
    pl.rows += L;
    pl.max_len = std::max(pl.max_len, L);
  }
  return pl;
}

// The route of a prompted call. AX_WHISPER_PREFILL (read at first use, per engine): "prefill" the prefill pass, "step" the step-fed
// route; unset: the prefill pass, which measured 9.5 to 34 times faster than the step-fed route at 1, 8 and 64 clips
// (profiles/prefill_bench.txt). A decoder shape the prefill kernels do not take goes the step-fed route whatever was asked.
// AX_WHISPER_GetConfigInt(h, "prefill") = the route this handle's prompted calls take: 0 the prefill pass, 1 step-fed.
int Engine::prefill_route() {
  if (prefill_env_ < 0) {
    const char* e = getenv("AX_WHISPER_PREFILL");
    if (!e || !e[0] || !strcmp(e, "prefill")) prefill_env_ = 0;
    else if (!strcmp(e, "step")) prefill_env_ = 1;
    else throw std::runtime_error("AX_WHISPER_PREFILL must be prefill or step");
    if (!prefill_supported()) prefill_env_ = 1;
    cfg_.ints["prefill"] = prefill_env_;
  }
  if (prefill_force_ == 0 && !prefill_supported()) throw std::runtime_error("bench prefill_pass: the prefill kernels do not take this decoder shape");
  return prefill_force_ >= 0 ? prefill_force_ : prefill_env_;
}

bool Engine::prefill_supported() const {
  const int d = cfg_.n_text_state;
  return d % 128 == 0 && cfg_.n_text_head * layout::kKvDim == d && cfg_.n_audio_ctx <= t_pad_;
}

// scratch of the prefill pass, grown on demand (allocation: nobody captures meanwhile)
void Engine::ensure_prefill_scratch(int rows, int clips) {
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  const int d = cfg_.n_text_state;
  PrefillScratch& p = prefill_;
  if (rows > p.rows_cap) {
    HIP_CHECK(hipStreamSynchronize(stream()));
    const size_t r = (size_t)rows;
    p.x = device_array<float>(r * d);
    p.ln = device_array<h16>(r * d);
    p.qkv = device_array<h16>(r * 3 * d);
    p.att = device_array<h16>(r * d);
    p.hid = device_array<h16>(r * 4 * d);
    p.row_tab = device_array<int>(r * 3);
    p.rows_cap = rows;
  }
  if (clips > p.clips_cap) {
    HIP_CHECK(hipStreamSynchronize(stream()));
    p.xg = device_array<float>((size_t)clips * d);
    p.nsp = device_array<float>(clips);
    p.clip_tab = device_array<int>((size_t)clips * 4);
    p.sot_logits.reset();
    p.clips_cap = clips;
  }
  if (d_ts_logits_ && !p.sot_logits) {  // (freed with the engine; re-made when the capacity grows)
    HIP_CHECK(hipStreamSynchronize(stream()));
    p.sot_logits = device_array<float>((size_t)p.clips_cap * ts_stride_);
  }
}

void Engine::prefill_prompts(int batch, const PromptSpec& prompts, bool want_no_speech, float* no_speech_out, float* sot_logits_out) {
  if (batch < 1 || batch > cap_) throw std::runtime_error("prefill_prompts: batch exceeds the slots");
  const PromptPlan pl = plan_prompts(cfg_, sot_seq_, batch, prompts);
  for (int b = 0; no_speech_out && b < batch; ++b) no_speech_out[b] = 0.f;
  if (sot_logits_out) std::fill(sot_logits_out, sot_logits_out + (size_t)batch * cfg_.n_vocab, 0.f);
  const int n = pl.clips();
  if (n == 0) return;
  const int route = prefill_route();
  if (want_no_speech) { require_scored_vocab(); ensure_ts_logits(); ensure_ts_scores(); }
  const int d = cfg_.n_text_state;
  hipStream_t s = stream();
  ensure_prefill_scratch(pl.rows, cap_);
  PrefillScratch& pf = prefill_;
  int *d_ctx = pf.row_tab, *d_row_pos = d_ctx + pl.rows, *d_row_slot = d_row_pos + pl.rows;
  int *d_row0 = pf.clip_tab, *d_len = d_row0 + n, *d_slot = d_len + n, *d_sot_row = d_slot + n;
  HIP_CHECK(hipMemcpyAsync(d_ctx, pl.ctx.data(), (size_t)pl.rows * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_row_pos, pl.row_pos.data(), (size_t)pl.rows * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_row_slot, pl.row_slot.data(), (size_t)pl.rows * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_row0, pl.row0.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_len, pl.len.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_slot, pl.slot.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_sot_row, pl.sot_row.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (pageable sources)

  if (route == 0) prefill_pass(pl.rows, n, pl.max_len, want_no_speech);
  else prefill_step_fed(batch, pl.slot, pl.len, pl.ctx, pl.row0, want_no_speech);

  PrefillHandoverParams h{};
  h.slot = d_slot; h.len = d_len; h.n_clips = n;
  h.off = d_off_; h.tok = d_tok_; h.n_out = d_nout_; h.transcribe = sot_seq_[2];
  h.tok_emb = tok_emb_; h.pos = dec_pos_; h.x = d_xdec_; h.d_model = d;
  if (want_no_speech) { h.no_speech = d_nospeech_; h.no_speech_clip = pf.nsp; }
  launch_prefill_handover(h, s);
  HIP_CHECK(hipGetLastError());
  if (want_no_speech && no_speech_out) {
    std::vector<float> v(n);
    HIP_CHECK(hipMemcpyAsync(v.data(), pf.nsp, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < n; ++c) no_speech_out[pl.slot[c]] = v[c];
  }
  if (want_no_speech && sot_logits_out)
    for (int c = 0; c < n; ++c)
      HIP_CHECK(hipMemcpyAsync(sot_logits_out + (size_t)pl.slot[c] * cfg_.n_vocab, pf.sot_logits + (size_t)c * ts_stride_, (size_t)cfg_.n_vocab * 4,
                               hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// All context rows of the prompted clips through the decoder layers in one pass: the residual stream fp32 [rows][d], activations
// h16 (the encoder's arithmetic: LayerNorm -> h16, MFMA GEMMs with fp32 accumulation), K and V into the slots' self caches.
void Engine::prefill_pass(int rows, int n_clips, int max_len, bool want_no_speech) {
  const int d = cfg_.n_text_state, H = cfg_.n_text_head, L = cfg_.n_text_layer, Tc = cfg_.n_text_ctx;
  hipStream_t s = stream();
  PrefillScratch& pf = prefill_;
  const int *d_ctx = pf.row_tab, *d_row_pos = d_ctx + rows, *d_row_slot = d_row_pos + rows;
  const int *d_row0 = pf.clip_tab, *d_len = d_row0 + n_clips, *d_slot = d_len + n_clips, *d_sot_row = d_slot + n_clips;
  const long self_stride = H * layout::kv_head_elems(Tc), cross_stride = H * layout::kv_head_elems(t_pad_);

  auto linear = [&](const h16* A, int K, const h16* W, const float* bias, void* C, int N, int epi) {
    GemmParams q{};
    q.A = A; q.lda = K; q.W = W; q.bias = bias; q.C = C; q.ldc = N;
    q.M = rows; q.N = N; q.K = K; q.batch = 1; q.d_model = d; q.epilogue = epi;
    launch_gemm(q, s);
  };
  auto attention = [&](const h16* q, int ldq, const h16* k, const h16* v, long stride, int keys_pad, int n_keys) {
    PrefillAttnParams a{};
    a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.kv_slot_stride = stride; a.keys_pad = keys_pad;
    a.out = pf.att; a.ldo = d; a.row0 = d_row0; a.len = d_len; a.slot = d_slot;
    a.n_clips = n_clips; a.max_len = max_len; a.n_head = H; a.n_keys = n_keys;
    launch_prefill_attention(a, s);
  };

  launch_prefill_embed(tok_emb_, dec_pos_, d_ctx, d_row_pos, pf.x, rows, d, s);
  for (int l = 0; l < L; ++l) {
    const DecLayerW& w = dec_[l];
    h16* sk = d_self_k_ + (size_t)l * cap_ * self_stride;
    h16* sv = d_self_v_ + (size_t)l * cap_ * self_stride;
    const h16* ck = d_cross_k_ + (size_t)l * cap_ * cross_stride;
    const h16* cv = d_cross_v_ + (size_t)l * cap_ * cross_stride;
    launch_layernorm_bf16(pf.x, w.attn_ln_w, w.attn_ln_b, pf.ln, rows, d, s);
    linear(pf.ln, d, w.w_qkv, w.b_qkv, pf.qkv, 3 * d, EPI_BIAS_BF16);
    PrefillStoreParams st{};
    st.qkv = pf.qkv; st.rows = rows; st.row_pos = d_row_pos; st.row_slot = d_row_slot;
    st.k_cache = sk; st.v_cache = sv; st.kv_slot_stride = self_stride; st.d_model = d; st.n_ctx_pad = Tc;
    launch_prefill_cache_store(st, s);
    attention(pf.qkv, 3 * d, sk, sv, self_stride, Tc, -1);
    linear(pf.att, d, w.w_o, w.b_o, pf.x, d, EPI_RESID_F32);
    launch_layernorm_bf16(pf.x, w.cross_ln_w, w.cross_ln_b, pf.ln, rows, d, s);
    linear(pf.ln, d, w.w_cq, w.b_cq, pf.qkv, d, EPI_BIAS_BF16);
    attention(pf.qkv, d, ck, cv, cross_stride, t_pad_, cfg_.n_audio_ctx);
    linear(pf.att, d, w.w_co, w.b_co, pf.x, d, EPI_RESID_F32);
    launch_layernorm_bf16(pf.x, w.mlp_ln_w, w.mlp_ln_b, pf.ln, rows, d, s);
    linear(pf.ln, d, w.w_fc1, w.b_fc1, pf.hid, 4 * d, EPI_BIAS_GELU_BF16);
    linear(pf.hid, 4 * d, w.w_fc2, w.b_fc2, pf.x, d, EPI_RESID_F32);
  }
  // the no-speech value of a prompted clip: log p(<|nospeech|>) of the row its sot position produced (decode offset 0 of an
  // unprompted clip, which a prompted slot never visits): those rows' final residuals through the existing logits launch
  if (want_no_speech) {
    const int n = n_clips;
    launch_prefill_gather_rows(pf.x, d_sot_row, pf.xg, n, d, s);
    GemvParams p{};
    p.W = tok_emb_; p.bias = nullptr; p.N = cfg_.n_vocab; p.K = d;
    p.prologue = PRO_LAYERNORM; p.in = pf.xg; p.ln_w = dec_ln_w_; p.ln_b = dec_ln_b_;
    p.epilogue = GEPI_LOGITS; p.state = d_state_; p.off = d_off_; p.amax_val = d_amax_val_; p.amax_idx = d_amax_idx_; p.amax_stride = n_amax_part_;
    p.skip_before_step = 0; p.logits_dump = d_ts_logits_; p.logits_dump_stride = ts_stride_;
    for (int c0 = 0; c0 < n; c0 += 4) {
      GemvParams q = p;
      q.batch = std::min(4, n - c0);
      q.in += (long)c0 * d; q.amax_val += (long)c0 * n_amax_part_; q.amax_idx += (long)c0 * n_amax_part_; q.off += c0;
      q.logits_dump += (long)c0 * ts_stride_;
      launch_gemv(q, s);
    }
    launch_row_logprob(d_ts_logits_, ts_stride_, cfg_.n_vocab, own_scores_.no_speech_id, n, pf.nsp, s);
    HIP_CHECK(hipMemcpyAsync(pf.sot_logits, d_ts_logits_, (size_t)n * ts_stride_ * 4, hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK(hipGetLastError());
}

// The step-fed route: the same context, one position per EXISTING decoder step (whichever sequence `batch` clips take), teacher-forced
// from position 0 (advance_kernel with a one-id prefix feeds forced[0], forced[1], ... = ctx[1:]). Every slot of the batch rides
// along for max_len steps: a shorter clip's surplus rows and an unprompted slot's rows land in cache rows at or beyond the offset
// the slot is handed over at, which no later step reads before writing; the loop state of all slots is then set back to what
// reset_decode_state left and the hand-over kernel moves the prompted ones. The no-speech row of clip c is the logits row of the
// step that fed its sot position.
void Engine::prefill_step_fed(int batch, const std::vector<int>& slot, const std::vector<int>& len, const std::vector<int>& ctx,
                              const std::vector<int>& row0, bool want_no_speech) {
  const int n = (int)slot.size(), Tc = cfg_.n_text_ctx;
  hipStream_t s = stream();
  int max_len = 0;
  for (int c = 0; c < n; ++c) max_len = std::max(max_len, len[c]);
  const int n_forced = max_len - 1;
  std::vector<int> forced((size_t)batch * n_forced, sot_seq_[0]), tok0(batch, sot_seq_[0]);
  for (int c = 0; c < n; ++c) {
    tok0[slot[c]] = ctx[row0[c]];
    for (int i = 1; i < len[c]; ++i) forced[(size_t)slot[c] * n_forced + i - 1] = ctx[row0[c] + i];
  }
  DeviceArray<int> d_forced = device_array<int>((size_t)batch * std::max(n_forced, 1));
  HIP_CHECK(hipMemcpyAsync(d_forced, forced.data(), forced.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_tok_, tok0.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s));
  launch_embed(tok_emb_, dec_pos_, d_tok_, d_off_, d_xdec_, batch, cfg_.n_text_state, s);
  HIP_CHECK(hipStreamSynchronize(s));  // (pageable sources)
  ensure_branch_streams(batch);
  for (int st = 0; st < max_len; ++st) {
    StepSpec spec{kDecodePlain};
    spec.feed = 1;
    for (int c = 0; want_no_speech && c < n; ++c)
      if (len[c] - 2 == st) spec.feed = 2;  // the position of sot: P + 1
    enqueue_decode_step(spec, batch, Tc, d_forced, n_forced, nullptr, 0, nullptr);
    for (int c = 0; spec.feed == 2 && c < n; ++c)
      if (len[c] - 2 == st) {
        launch_row_logprob(d_ts_logits_ + (size_t)slot[c] * ts_stride_, ts_stride_, cfg_.n_vocab, own_scores_.no_speech_id, 1, prefill_.nsp + c, s);
        HIP_CHECK(hipMemcpyAsync(prefill_.sot_logits + (size_t)c * ts_stride_, d_ts_logits_ + (size_t)slot[c] * ts_stride_, (size_t)ts_stride_ * 4,
                                 hipMemcpyDeviceToDevice, s));
      }
  }
  std::fill(tok0.begin(), tok0.end(), sot_seq_[0]);
  HIP_CHECK(hipMemsetAsync(d_off_, 0, (size_t)batch * 4, s));
  HIP_CHECK(hipMemcpyAsync(d_tok_, tok0.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s));
  launch_embed(tok_emb_, dec_pos_, d_tok_, d_off_, d_xdec_, batch, cfg_.n_text_state, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));  // (d_forced and tok0 leave scope)
}

// back to [n_text_layer][n_rows][d] fp32 from the blocked K / row-major V of the slot's self-attention cache (GetCrossKV's twin)
void Engine::get_self_kv(int slot, int n_rows, float* k_out, float* v_out) {
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  if (slot < 0 || slot >= cap_) throw std::runtime_error("slot out of range");
  const int d = cfg_.n_text_state, H = cfg_.n_text_head, L = cfg_.n_text_layer, Tc = cfg_.n_text_ctx;
  if (n_rows < 1 || n_rows > Tc) throw std::runtime_error("get_self_kv: n_rows out of range");
  const size_t head = (size_t)layout::kv_head_elems(Tc), per = H * head;
  std::vector<uint16_t> hk(per), hv(per);
  HIP_CHECK(hipStreamSynchronize(stream()));
  for (int l = 0; l < L; ++l) {
    HIP_CHECK(hipMemcpy(hk.data(), d_self_k_ + ((size_t)l * cap_ + slot) * per, per * 2, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hv.data(), d_self_v_ + ((size_t)l * cap_ + slot) * per, per * 2, hipMemcpyDeviceToHost));
    for (int h = 0; h < H; ++h)
      for (int t = 0; t < n_rows; ++t)
        for (int c = 0; c < layout::kKvDim; ++c) {
          k_out[((size_t)l * n_rows + t) * d + h * 64 + c] = h16_bits_to_float(hk[h * head + layout::k_index(t, c)]);
          v_out[((size_t)l * n_rows + t) * d + h * 64 + c] = h16_bits_to_float(hv[h * head + layout::v_index(t, c)]);
        }
  }
}

// stage level: after encode_mel, the decode state of slots [0, batch) as a prompted greedy loop finds it before its first step
void Engine::prefill_stage(int batch, const PromptSpec& prompts, float* no_speech_logprob, float* sot_logits) {
  require_no_stream("prefill_prompts");
  require_timestamp_vocab();
  HIP_CHECK(hipSetDevice(device_));
  if (batch < 1 || batch > cap_) throw std::runtime_error("prefill_prompts: batch exceeds the encoded slots");
  reset_decode_state(batch);
  prefill_prompts(batch, prompts, no_speech_logprob != nullptr || sot_logits != nullptr, no_speech_logprob, sot_logits);
}

void Engine::decode_forced_prompted(DecodeMode mode, int batch, const PromptSpec& prompts, const int32_t* forced, int n_forced, float* logits,
                                    int32_t* chosen, const ForcedScores* scores, const SampleSpec* sample) {
  if (mode < kDecodeTimestamps) throw std::runtime_error("prompted decode exists in the timestamp modes only");
  if (scores && scores->logits0) throw std::runtime_error("decode_forced_prompted: a prompted clip has no row of decode offset 0");
  const ScopedSet<const PromptSpec*> scope(prompt_, &prompts);
  decode_forced(mode, batch, forced, n_forced, logits, chosen, scores, sample);
}

void Engine::run_tokens_prompted(DecodeMode mode, const float* const* pcm, const int* n_samples, int batch, int max_new, const int* max_new_clip,
                                 const PromptSpec& prompts, int32_t* ids, int* n_ids, const ClipScores* scores, const SampleSpec* sample) {
  if (mode < kDecodeTimestamps) throw std::runtime_error("prompted decode exists in the timestamp modes only");
  (void)plan_prompts(cfg_, sot_seq_, std::max(batch, 0), prompts);  // a bad prompt fails before any GPU work
  const ScopedSet<const PromptSpec*> scope(prompt_, &prompts);
  run_tokens(mode, pcm, nullptr, 0, n_samples, batch, max_new, max_new_clip, ids, n_ids, scores, sample);
}

}  // inline namespace AXW_NS
}  // namespace axw
