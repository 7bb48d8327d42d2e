// engine_prefill.cpp — axw::Engine: prompt conditioning (DESIGN.md "Prompt conditioning"). prefill_prompts() is the ONE place a
// prompt enters the engine: between reset_decode_state and the first decoder step it brings every prompted slot to the state
// "context [sot_prev, prompt, sot, language] cached, `transcribe` about to be fed at offset L = P + 3", after which the existing
// steps (logits, rules, advance) run unchanged. Slots without a prompt are not touched. What it works on is its argument: the
// ClipContexts of the call (iengine.hpp), handed down from the entry point (run_tokens, decode_forced, prefill_stage, the long-form
// loop) through greedy_loop; the engine keeps no state of a call in progress.
// Two routes lead to that state: the prefill pass (decode_prefill.hip + the encoder's GEMM / LayerNorm, all rows at once) and the
// step-fed route (AX_WHISPER_PREFILL=step: one existing decoder step per position; the yardstick for error and time).
// A language and task per clip (DESIGN.md "Language and task per clip") is the same mechanism: the context [sot, language] is the
// prompted case with an empty prompt and no sot_prev, the task id is what the hand-over feeds; language detection runs in front.
// Out of scope: prompts and per-clip languages under beam search, in the Stream* slots and in the persistent launches; best_of above 1.
#include "engine_impl.hpp"

#include <climits>

namespace axw {
inline namespace AXW_NS {

namespace {
// the clips of one call that get a context, as the kernels' tables want them
struct PromptPlan {
  std::vector<int> ctx, row_pos, row_slot;             // per row
  std::vector<int> row0, len, slot, sot_row, n_kept;   // per context clip
  std::vector<int> task_tok, lang_row;                 // per context clip: the id fed at the hand-over; the row that holds its language id
  std::vector<int> detect;                             // the context clips that detect their language (indices into the arrays above)
  std::vector<int> lang_index;                         // per clip of the batch: its language index; -2: to be detected
  int rows = 0, max_len = 0;
  int clips() const { return (int)slot.size(); }
};
}  // namespace

// The context plan of a call. pr (or null: no clip is prompted): pr->n_prompt[b] ids of clip b at pr->ids + b * pr->stride, truncated
// to their last n_text_ctx / 2 - 1 (openai-whisper); lang (or null): the language and task of every clip. A clip gets a context
// ([sot_prev, prompt] if prompted) + [sot, language] when it is prompted, detects, asks for another language than the handle's or
// another task than transcribe (or when force says so); without `lang` this is exactly the prompted clips of the call.
static PromptPlan plan_contexts(const ModelConfig& cfg, const int* sot_seq, int handle_lang, int batch, const IEngine::PromptSpec* pr,
                                const IEngine::LangSpec* lang, bool force) {
  if (pr && !pr->n_prompt) throw std::runtime_error("prefill_prompts: no prompt lengths");
  const int keep = cfg.n_text_ctx / 2 - 1, ts_begin = cfg.no_timestamps + 1, n_lang = (int)cfg.lang_tokens.size();
  int sot_prev = -1, translate = -1;
  {
    const auto it = cfg.ints.find("sot_prev");
    if (it != cfg.ints.end() && it->second >= 0 && it->second < cfg.n_vocab) sot_prev = (int)it->second;
    const auto tr = cfg.ints.find("translate");
    if (tr != cfg.ints.end() && tr->second >= 0 && tr->second < cfg.n_vocab) translate = (int)tr->second;
  }
  if (pr && !lang && sot_prev < 0) throw std::runtime_error("prompted decode needs a sot_prev id inside the vocabulary");
  PromptPlan pl;
  pl.lang_index.assign(batch, handle_lang);
  for (int b = 0; b < batch; ++b) {
    const int n = pr ? pr->n_prompt[b] : 0;
    if (pr && (n < 0 || n > pr->stride)) throw std::runtime_error("prefill_prompts: prompt length " + std::to_string(n) + " of clip " + std::to_string(b) + " out of range");
    const int lg = lang && lang->lang ? lang->lang[b] : -1, task = lang && lang->task ? lang->task[b] : 0;
    if (lg < -2 || lg >= n_lang) throw std::runtime_error("language index " + std::to_string(lg) + " of clip " + std::to_string(b) + " is outside [-2, " + std::to_string(n_lang) + ")");
    if (task != 0 && task != 1) throw std::runtime_error("task " + std::to_string(task) + " of clip " + std::to_string(b) + " is neither 0 (transcribe) nor 1 (translate)");
    if (task == 1 && translate < 0) throw std::runtime_error("translate: the config has no translate id inside the vocabulary");
    if (lg == -2 && n_lang < 2) throw std::runtime_error("language detection needs a config with more than one language");
    pl.lang_index[b] = lg == -1 ? handle_lang : lg;
    if (n == 0 && !force && lg != -2 && pl.lang_index[b] == handle_lang && task == 0) continue;  // no context: the clip is not touched
    int P = 0;
    const int32_t* src = nullptr;
    if (n > 0) {
      if (!pr->ids) throw std::runtime_error("prefill_prompts: no prompt ids");
      if (sot_prev < 0) throw std::runtime_error("prompted decode needs a sot_prev id inside the vocabulary");
      P = std::min(n, keep);
      src = pr->ids + (size_t)b * pr->stride + (n - P);
      for (int i = 0; i < P; ++i)
        if (src[i] < 0 || src[i] >= cfg.n_vocab || (src[i] >= cfg.eot && src[i] < ts_begin))
          throw std::runtime_error("prefill_prompts: id " + std::to_string(src[i]) + " of clip " + std::to_string(b) + " is neither text nor a timestamp");
    }
    const int L = P ? P + 3 : 2, lead = L - 2;  // rows in front of sot
    if (L + 1 > cfg.n_text_ctx) throw std::runtime_error("prefill_prompts: the prompt leaves no room in the context");
    if (lg == -2) pl.detect.push_back(pl.clips());
    pl.row0.push_back(pl.rows); pl.len.push_back(L); pl.slot.push_back(b); pl.sot_row.push_back(pl.rows + lead); pl.n_kept.push_back(P);
    pl.task_tok.push_back(task == 1 ? translate : sot_seq[2]);
    pl.lang_row.push_back(pl.rows + lead + 1);
    for (int i = 0; i < L; ++i) {
      // (a detecting clip's language entry is the handle's until the detection kernel patches it)
      pl.ctx.push_back(i < lead ? (i == 0 ? sot_prev : (int)src[i - 1]) : i == lead ? sot_seq[0] : lg >= 0 ? cfg.lang_tokens[lg] : sot_seq[1]);
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
    p.det_tab = device_array<int>((size_t)clips * 2);
    p.task_tok = device_array<int>(clips);
    p.lang_idx = device_array<int>(clips);
    p.lang_lp = device_array<float>((size_t)clips * kLangMax);
    p.lang_logit = device_array<float>((size_t)clips * kLangMax);
    p.clips_cap = clips;
  }
  if (d_ts_logits_ && !p.sot_logits) {  // (freed with the engine; re-made when the capacity grows)
    HIP_CHECK(hipStreamSynchronize(stream()));
    p.sot_logits = device_array<float>((size_t)p.clips_cap * ts_stride_);
  }
}

static const IEngine::PromptSpec* or_null(const std::optional<IEngine::PromptSpec>& o) { return o ? &*o : nullptr; }
static const IEngine::LangSpec* or_null(const std::optional<IEngine::LangSpec>& o) { return o ? &*o : nullptr; }

void Engine::prefill_prompts(int batch, const ClipContexts& ctx, bool force_context, bool want_no_speech, float* no_speech_out,
                             float* sot_logits_out) {
  if (batch < 1 || batch > cap_) throw std::runtime_error("prefill_prompts: batch exceeds the slots");
  const bool per_lang = ctx.lang.has_value();
  PromptPlan pl = plan_contexts(cfg_, sot_seq_, handle_lang_, batch, or_null(ctx.prompts), or_null(ctx.lang), force_context);
  const int n_lang = (int)cfg_.lang_tokens.size();
  const LangResult lout = per_lang ? ctx.lang_out : LangResult{};
  for (int b = 0; no_speech_out && b < batch; ++b) no_speech_out[b] = 0.f;
  if (sot_logits_out) std::fill(sot_logits_out, sot_logits_out + (size_t)batch * cfg_.n_vocab, 0.f);
  if (lout.lang_logprob) std::fill(lout.lang_logprob, lout.lang_logprob + (size_t)batch * n_lang, 0.f);
  if (lout.lang_logit) std::fill(lout.lang_logit, lout.lang_logit + (size_t)batch * n_lang, 0.f);
  for (int b = 0; lout.detected && b < batch; ++b) lout.detected[b] = pl.lang_index[b];
  const int n = pl.clips(), nd = (int)pl.detect.size();
  if (n == 0) return;
  const int route = prefill_route();
  if (want_no_speech) { require_scored_vocab(); ensure_ts_logits(); ensure_ts_scores(); }
  const int d = cfg_.n_text_state;
  hipStream_t s = stream();
  ensure_prefill_scratch(pl.rows, cap_);
  if (per_lang) ensure_lang_buffers();
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
  if (per_lang) HIP_CHECK(hipMemcpyAsync(pf.task_tok, pl.task_tok.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (pageable sources)

  // detection first: the language entry of a detecting clip's context is written before the contexts are fed
  std::vector<int> det_slot(nd), det_row(nd), det_idx(nd);
  std::vector<float> det_lp((size_t)nd * n_lang), det_logit(lout.lang_logit ? (size_t)nd * n_lang : 0);
  for (int i = 0; i < nd; ++i) { det_slot[i] = pl.slot[pl.detect[i]]; det_row[i] = pl.lang_row[pl.detect[i]]; }
  if (nd > 0 && route == 0) {
    enqueue_detect_prefill(batch, det_slot, d_ctx, det_row, lout.lang_logit != nullptr);  // (no host round trip: the kernel patches d_ctx)
  } else if (nd > 0) {
    detect_step_fed(batch, det_slot, det_idx.data(), det_lp.data(), lout.lang_logit ? det_logit.data() : nullptr);
    for (int i = 0; i < nd; ++i) pl.ctx[det_row[i]] = cfg_.lang_tokens[det_idx[i]];
  }

  if (route == 0) prefill_pass(pl.rows, n, pl.max_len, want_no_speech);
  else prefill_step_fed(batch, pl.slot, pl.len, pl.ctx, pl.row0, want_no_speech);

  PrefillHandoverParams h{};
  h.slot = d_slot; h.len = d_len; h.n_clips = n;
  h.off = d_off_; h.tok = d_tok_; h.n_out = d_nout_; h.transcribe = sot_seq_[2];
  h.tok_emb = tok_emb_; h.pos = dec_pos_; h.x = d_xdec_; h.d_model = d;
  if (want_no_speech) { h.no_speech = d_nospeech_; h.no_speech_clip = pf.nsp; }
  if (per_lang) h.task_tok = pf.task_tok;
  launch_prefill_handover(h, s);
  HIP_CHECK(hipGetLastError());
  if (nd > 0) {
    if (route == 0) fetch_detected(nd, det_idx.data(), det_lp.data(), lout.lang_logit ? det_logit.data() : nullptr);
    for (int i = 0; i < nd; ++i) {
      const int b = det_slot[i];
      if (lout.detected) lout.detected[b] = det_idx[i];
      if (lout.lang_logprob) std::copy(det_lp.begin() + (size_t)i * n_lang, det_lp.begin() + (size_t)(i + 1) * n_lang, lout.lang_logprob + (size_t)b * n_lang);
      if (lout.lang_logit) std::copy(det_logit.begin() + (size_t)i * n_lang, det_logit.begin() + (size_t)(i + 1) * n_lang, lout.lang_logit + (size_t)b * n_lang);
    }
  }
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

// ------------------------------------------------------------------------------ language detection
void Engine::require_lang_call(DecodeMode mode, const char* what) const {
  if (mode < kDecodeTimestamps) throw std::runtime_error(std::string(what) + ": a language or task per clip exists in the timestamp modes only");
  require_no_stream(what);
  require_timestamp_vocab();
}

void Engine::check_contexts(DecodeMode mode, const ClipContexts& ctx, int batch, bool force_context, const char* what) const {
  if (!ctx.any()) return;
  if (ctx.lang) require_lang_call(mode, what);
  else if (mode < kDecodeTimestamps) throw std::runtime_error(std::string(what) + ": prompted decode exists in the timestamp modes only");
  (void)plan_contexts(cfg_, sot_seq_, handle_lang_, std::max(batch, 0), or_null(ctx.prompts), or_null(ctx.lang), force_context);
}

void Engine::ensure_lang_buffers() {
  if (prefill_.lang_tok) return;
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  const int n_lang = (int)cfg_.lang_tokens.size();
  if (n_lang > kLangMax) throw std::runtime_error("language list longer than " + std::to_string(kLangMax));
  for (int t : cfg_.lang_tokens)
    if (t < 0 || t >= cfg_.n_vocab) throw std::runtime_error("config: a language id lies outside the vocabulary");
  HIP_CHECK(hipStreamSynchronize(stream()));
  DeviceArray<int> tok = device_array<int>(n_lang);
  HIP_CHECK(hipMemcpy(tok, cfg_.lang_tokens.data(), (size_t)n_lang * 4, hipMemcpyHostToDevice));
  prefill_.lang_tok = std::move(tok);
}

LangDetectParams Engine::detect_params(const float* x, int n_clips, bool want_logit) const {
  LangDetectParams q{};
  q.x = x; q.ln_w = dec_ln_w_; q.ln_b = dec_ln_b_; q.tok_emb = tok_emb_;
  q.lang_tokens = prefill_.lang_tok; q.n_lang = (int)cfg_.lang_tokens.size();
  q.d_model = cfg_.n_text_state; q.n_clips = n_clips; q.fallback_index = handle_lang_;
  q.lang_logit = want_logit ? prefill_.lang_logit.get() : nullptr; q.lang_logprob = prefill_.lang_lp; q.lang_index = prefill_.lang_idx;
  return q;
}

// Detection on the prefill route. The [sot] position of every slot of the batch goes through the layers of ONE existing decoder step
// (offset 0, token sot, as reset_decode_state left them; openai-whisper's detect_language context, no prompt in front even for a
// prompted clip) WITHOUT its vocabulary projection and WITHOUT advance_kernel, so the slots' final residual rows stand in d_xdec_;
// the detection kernel reads the detecting slots' rows there and patches d_ctx, and the embedding launch puts x back to what the
// reset left. Offsets, tokens and counters were never moved. The host is waited for once, for the upload of the slot table; nothing
// waits between the detection and the context prefill that reads what it patched.
// (Not the one-row prefill pass: that pass keeps attention and LayerNorm outputs in the 16-bit type, which measured 0.76 (bf16) and
// 0.25 (half) of error in language logits whose smallest kept margin is 0.5 and 0.72, and it cost 2.1 ms against the 0.5 ms of a step.)
void Engine::enqueue_detect_prefill(int batch, const std::vector<int>& slot, int* d_ctx, const std::vector<int>& lang_row, bool want_logit) {
  const int nd = (int)slot.size();
  hipStream_t s = stream();
  PrefillScratch& pf = prefill_;
  std::vector<int> tab((size_t)nd * 2);  // [slot | the context entry to patch]
  for (int i = 0; i < nd; ++i) { tab[i] = slot[i]; tab[nd + i] = d_ctx ? lang_row[i] : 0; }
  HIP_CHECK(hipMemcpyAsync(pf.det_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (pageable source)
  ensure_branch_streams(batch);
  StepSpec spec{kDecodePlain};  // (cross_fp8 clear: detection and the step-fed contexts read the h16 cross K/V, as the prefill kernels do)
  spec.mask = 15 & ~4;  // no advance: offsets and tokens stay, x keeps the final residual
  spec.feed = 1;        // no vocabulary projection
  enqueue_decode_step(spec, batch, cfg_.n_text_ctx, nullptr, 0, nullptr, 0, nullptr);
  LangDetectParams q = detect_params(d_xdec_, nd, want_logit);
  q.x_row = pf.det_tab;
  if (d_ctx) { q.ctx = d_ctx; q.lang_row = pf.det_tab + nd; }
  launch_language_detect(q, s);
  launch_embed(tok_emb_, dec_pos_, d_tok_, d_off_, d_xdec_, batch, cfg_.n_text_state, s);
  HIP_CHECK(hipGetLastError());
}

void Engine::fetch_detected(int n, int* idx, float* lp, float* logit) {
  const size_t nl = cfg_.lang_tokens.size();
  hipStream_t s = stream();
  HIP_CHECK(hipMemcpyAsync(idx, prefill_.lang_idx, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(lp, prefill_.lang_lp, n * nl * 4, hipMemcpyDeviceToHost, s));
  if (logit) HIP_CHECK(hipMemcpyAsync(logit, prefill_.lang_logit, n * nl * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// The step-fed route's detection, the yardstick: one EXISTING decoder step at offset 0 (every slot of the batch feeds sot) with the
// logits dump, the language entries of the dumped rows picked on the host by the definition (first maximum in list order, NaN
// never wins; logsumexp over the entries that are not NaN; nothing finite: the handle's language, every value -inf).
void Engine::detect_step_fed(int batch, const std::vector<int>& slot, int* idx, float* lp, float* logit) {
  const int nd = (int)slot.size(), nl = (int)cfg_.lang_tokens.size(), nv = cfg_.n_vocab;
  hipStream_t s = stream();
  ensure_ts_logits();
  std::vector<int> forced(batch, sot_seq_[0]);
  DeviceArray<int> d_forced = device_array<int>(batch);
  HIP_CHECK(hipMemcpyAsync(d_forced, forced.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (pageable source)
  ensure_branch_streams(batch);
  StepSpec spec{kDecodePlain};  // (cross_fp8 clear: detection and the step-fed contexts read the h16 cross K/V, as the prefill kernels do)
  spec.feed = 2;
  enqueue_decode_step(spec, batch, cfg_.n_text_ctx, d_forced, 1, nullptr, 0, nullptr);
  std::vector<float> row(nv);
  for (int i = 0; i < nd; ++i) {
    HIP_CHECK(hipMemcpyAsync(row.data(), d_ts_logits_ + (size_t)slot[i] * ts_stride_, (size_t)nv * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    float m = -INFINITY;
    int best = -1;
    bool any_finite = false;
    for (int j = 0; j < nl; ++j) {
      const float x = row[cfg_.lang_tokens[j]];
      if (logit) logit[(size_t)i * nl + j] = x;
      if (x > m) { m = x; best = j; }
      any_finite = any_finite || std::isfinite(x);
    }
    float* out = lp + (size_t)i * nl;
    if (best < 0 || !any_finite) {
      idx[i] = handle_lang_;
      std::fill(out, out + nl, -INFINITY);
      continue;
    }
    idx[i] = best;
    double sum = 0.0;
    for (int j = 0; j < nl; ++j) {
      const float x = row[cfg_.lang_tokens[j]];
      if (x == x && m != INFINITY) sum += std::exp((double)x - (double)m);
    }
    for (int j = 0; j < nl; ++j) {
      const float x = row[cfg_.lang_tokens[j]];
      out[j] = x != x ? -INFINITY : m == INFINITY ? (x == INFINITY ? 0.f : -INFINITY) : (float)((double)x - ((double)m + std::log(sum)));
    }
  }
  // back to what reset_decode_state left (prefill_step_fed, or the caller, starts from offset 0)
  HIP_CHECK(hipMemsetAsync(d_off_, 0, (size_t)batch * 4, s));
  HIP_CHECK(hipMemcpyAsync(d_tok_, forced.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s));
  launch_embed(tok_emb_, dec_pos_, d_tok_, d_off_, d_xdec_, batch, cfg_.n_text_state, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));  // (d_forced and forced leave scope)
}

// All context rows of the prompted clips through the decoder layers in one pass: the residual stream fp32 [rows][d], activations
// h16 (the encoder's arithmetic: LayerNorm -> h16, MFMA GEMMs with fp32 accumulation), K and V into the slots' self caches.
void Engine::prefill_pass(int rows, int n_clips, int max_len, bool want_no_speech, const LayerHook* after_cq) {
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
    if (after_cq) (*after_cq)(l);
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
    StepSpec spec{kDecodePlain};  // (cross_fp8 clear: detection and the step-fed contexts read the h16 cross K/V, as the prefill kernels do)
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

// stage level: after encode_mel, the decode state of slots [0, batch) as a greedy loop under ctx finds it before its first step
void Engine::prefill_stage(int batch, const ClipContexts& ctx, float* no_speech_logprob, float* sot_logits) {
  require_no_stream("prefill_prompts");
  require_timestamp_vocab();
  HIP_CHECK(hipSetDevice(device_));
  if (batch < 1 || batch > cap_) throw std::runtime_error("prefill_prompts: batch exceeds the encoded slots");
  check_contexts(kDecodeTimestamps, ctx, batch, false, "prefill_prompts");
  reset_decode_state(batch);
  prefill_prompts(batch, ctx, false, no_speech_logprob != nullptr || sot_logits != nullptr, no_speech_logprob, sot_logits);
}

// ------------------------------------------------------------------------------ language detection: entry points
void Engine::detect_language_stage(int batch, const LangResult& out) {
  require_lang_call(kDecodeTimestamps, "detect_language");
  if (!out.detected) throw std::runtime_error("detect_language: no output array");
  if (cfg_.lang_tokens.size() < 2) throw std::runtime_error("language detection needs a config with more than one language");
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  if (batch < 1 || batch > cap_) throw std::runtime_error("detect_language: batch exceeds the encoded slots");
  const int nl = (int)cfg_.lang_tokens.size();
  reset_decode_state(batch);
  std::vector<int> slot(batch), idx(batch);
  for (int b = 0; b < batch; ++b) slot[b] = b;
  std::vector<float> lp((size_t)batch * nl), logit(out.lang_logit ? (size_t)batch * nl : 0);
  if (prefill_route() == 0) {
    ensure_prefill_scratch(batch, cap_);
    ensure_lang_buffers();
    enqueue_detect_prefill(batch, slot, nullptr, slot, out.lang_logit != nullptr);
    fetch_detected(batch, idx.data(), lp.data(), out.lang_logit ? logit.data() : nullptr);
  } else {
    detect_step_fed(batch, slot, idx.data(), lp.data(), out.lang_logit ? logit.data() : nullptr);
  }
  std::copy(idx.begin(), idx.end(), out.detected);
  if (out.lang_logprob) std::copy(lp.begin(), lp.end(), out.lang_logprob);
  if (out.lang_logit) std::copy(logit.begin(), logit.end(), out.lang_logit);
}

// front-end, encoder, detection: nothing is decoded
void Engine::detect_language(const float* const* pcm, const int* n_samples, int batch, const LangResult& out) {
  if (batch < 1) throw std::runtime_error("batch must be >= 1");
  require_lang_call(kDecodeTimestamps, "detect_language");
  if (!out.detected) throw std::runtime_error("detect_language: no output array");
  if (cfg_.lang_tokens.size() < 2) throw std::runtime_error("language detection needs a config with more than one language");
  HIP_CHECK(hipSetDevice(device_));
  ensure_capacity(batch);
  upload_pcm(pcm, n_samples, batch);
  run_frontend(d_pcm_, (int)pcm_stride_, n_samples, batch, false, true);
  run_encoder(batch);
  detect_language_stage(batch, out);
}

void Engine::language_logprob_rows(const float* rows, int n, float* lang_logprob, int* lang_index, float* lang_logit) {
  require_no_stream("language_logprob_rows");
  if (!rows || n < 1 || !lang_logprob || !lang_index) throw std::runtime_error("language_logprob_rows: bad arguments");
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  ensure_lang_buffers();
  const size_t d = (size_t)cfg_.n_text_state, nl = cfg_.lang_tokens.size();
  hipStream_t s = stream();
  HIP_CHECK(hipStreamSynchronize(s));
  DeviceArray<float> x = device_array<float>(n * d), lp = device_array<float>(n * nl), lg = device_array<float>(n * nl);
  DeviceArray<int> ix = device_array<int>(n);
  HIP_CHECK(hipMemcpy(x, rows, n * d * 4, hipMemcpyHostToDevice));
  LangDetectParams q = detect_params(x, n, true);
  q.lang_logit = lg; q.lang_logprob = lp; q.lang_index = ix;
  launch_language_detect(q, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipMemcpy(lang_logprob, lp, n * nl * 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(lang_index, ix, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (lang_logit) HIP_CHECK(hipMemcpy(lang_logit, lg, n * nl * 4, hipMemcpyDeviceToHost));
}

}  // inline namespace AXW_NS
}  // namespace axw
