// engine_align.cpp — axw::Engine: word-level timestamps (DESIGN.md "Word-level timestamps"). align_tokens() sits between an encoded
// batch and the host rule (words.hpp): the context [sot, language, task, no_timestamps, t_1 .. t_n, eot] of every clip goes through
// the prefill pass (engine_prefill.cpp: all rows at once, the tables of a prompted call) with one hook per layer, which takes the
// cross-attention queries of the layers that own an alignment head to align_qk_softmax_kernel and align_normalize_kernel
// (decode_align.hip); align_dtw_kernel then walks the head-averaged matrix, and the final residual rows of the text positions go
// through the existing logits launch for the token probabilities. The state is the call's: scratch is allocated and freed here, the
// decode state of the slots is not read, and of it only the self-attention caches are overwritten (every decode resets and
// rewrites them before it reads them).
// AX_WHISPER_WORD_ALIGN=host is the yardstick route: the P scratch of every aligned layer goes to the host, where words.hpp's
// align_normalize_host and align_path do what the two kernels do. AX_WHISPER_GetConfigInt(h, "word_align") = the route of this
// handle: 0 the kernels, 1 the host.
// The token probabilities have two routes (AlignRequest::logprob_route): rows, the logits launch four rows at a time, and fused,
// vocab_logprob.hip (no logits row is written). AX_WHISPER_WORD_LOGPROB=rows|fused overrides the request;
// AX_WHISPER_GetConfigInt(h, "word_logprob") = 0 no override, 1 rows, 2 fused.
// Out of scope: decoder shapes the prefill kernels refuse (an error), words under beam search and in Stream* (the long-form loop
// calls align_tokens once per pass: engine_long.cpp).
#include "engine_impl.hpp"
#include "words.hpp"

namespace axw {
inline namespace AXW_NS {

namespace {
constexpr size_t kAlignScratchBytes = (size_t)256 << 20;  // the P scratch of one chunk of clips stays under this
constexpr int kAlignLogitRows = 64;                       // rows per round of the token-probability logits
constexpr int kAlignChunkRows = 4096;                     // context rows of one chunk: bounds the prefill pass's scratch, which the engine keeps

// narrowing on the host, round to nearest even, as the device's conversions
uint16_t float_to_h16_bits(float f) {
#if AXW_F16
  const _Float16 h = (_Float16)f;
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1)) >> 16);
#endif
}
}  // namespace

std::vector<std::pair<int, int>> Engine::alignment_heads() const {
  return align_heads_.empty() ? default_alignment_heads(cfg_.n_text_layer, cfg_.n_text_head) : align_heads_;
}

// n == 0: back to what the handle was constructed with (the config file's list, or the default)
void Engine::set_alignment_heads(const int* pairs, int n) {
  if (n < 0 || (n > 0 && !pairs)) throw std::runtime_error("set_alignment_heads: bad arguments");
  align_heads_ = n == 0 ? config_heads_ : checked_alignment_heads(pairs, n, cfg_.n_text_layer, cfg_.n_text_head, "set_alignment_heads");
  cfg_.ints["n_alignment_heads"] = (long)alignment_heads().size();
}

// AX_WHISPER_WORD_ALIGN is read at first use (a mistyped value fails the first alignment call, not the construction of a handle
// that may never ask for words); what the variable holds is reported from the start: an unknown value reports the kernels' route.
int Engine::align_route() {
  if (align_env_ < 0) {
    const char* e = getenv("AX_WHISPER_WORD_ALIGN");
    if (!e || !e[0] || !strcmp(e, "gpu")) align_env_ = 0;
    else if (!strcmp(e, "host")) align_env_ = 1;
    else throw std::runtime_error("AX_WHISPER_WORD_ALIGN must be gpu or host");
    cfg_.ints["word_align"] = align_env_;
  }
  return align_force_ >= 0 ? align_force_ : align_env_;
}

// AX_WHISPER_WORD_LOGPROB, like AX_WHISPER_WORD_ALIGN: read (and a mistyped value refused) at the first alignment call
int Engine::logprob_route(int requested) {
  if (logprob_env_ < 0) {
    const char* e = getenv("AX_WHISPER_WORD_LOGPROB");
    if (!e || !e[0]) logprob_env_ = 0;
    else if (!strcmp(e, "rows")) logprob_env_ = 1;
    else if (!strcmp(e, "fused")) logprob_env_ = 2;
    else throw std::runtime_error("AX_WHISPER_WORD_LOGPROB must be rows or fused");
    cfg_.ints["word_logprob"] = logprob_env_;
  }
  if (requested != kAlignLogProbRows && requested != kAlignLogProbFused) throw std::runtime_error("align_tokens: unknown log-prob route " + std::to_string(requested));
  return logprob_env_ == 1 ? kAlignLogProbRows : logprob_env_ == 2 ? kAlignLogProbFused : requested;
}

// The rows route: the rows through the logits launch, four at a time, 64 dumped logits rows per round, one value out of each.
// The round's buffers are the call's own (the slots' argmax partials and offsets are not touched).
void Engine::token_logprob_rows(const float* x, const int* row, const int* id, int n, float* lp, hipStream_t s) {
  const int d = cfg_.n_text_state;
  const long vstride = ((long)cfg_.n_vocab + 3) / 4 * 4;
  DeviceArray<float> xg = device_array<float>((size_t)kAlignLogitRows * d), logits = device_array<float>((size_t)kAlignLogitRows * vstride),
                     amax_val = device_array<float>((size_t)4 * n_amax_part_);
  DeviceArray<int> amax_idx = device_array<int>((size_t)4 * n_amax_part_), off4 = device_array<int>(4, true);
  GemvParams g{};
  g.W = tok_emb_; g.bias = nullptr; g.N = cfg_.n_vocab; g.K = d;
  g.prologue = PRO_LAYERNORM; g.in = xg; g.ln_w = dec_ln_w_; g.ln_b = dec_ln_b_;
  g.epilogue = GEPI_LOGITS; g.state = d_state_; g.off = off4; g.amax_val = amax_val; g.amax_idx = amax_idx; g.amax_stride = n_amax_part_;
  g.skip_before_step = 0; g.logits_dump = logits; g.logits_dump_stride = vstride;
  for (int r0 = 0; r0 < n; r0 += kAlignLogitRows) {
    const int cnt = std::min(kAlignLogitRows, n - r0);
    if (row) launch_prefill_gather_rows(x, row + r0, xg, cnt, d, s);
    else g.in = x + (size_t)r0 * d;
    for (int q0 = 0; q0 < cnt; q0 += 4) {
      GemvParams q = g;
      q.batch = std::min(4, cnt - q0);
      q.in += (long)q0 * d;
      q.logits_dump += (long)q0 * vstride;
      launch_gemv(q, s);
    }
    launch_row_id_logprob(logits, vstride, cfg_.eot, id + r0, cnt, lp + r0, s);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));  // (the buffers leave scope)
}

// The fused route (vocab_logprob.hip): gather, LayerNorm into the 16-bit operand, main launch, merge. The rows that pad the last
// row tile are zeros.
void Engine::token_logprob_fused(const float* x, const int* row, const int* id, int n, float* lp, hipStream_t s) {
  const int d = cfg_.n_text_state;
  VocabLogProbParams p{};
  if (!vocab_logprob_plan(d, n, cfg_.eot, &p.row_tile, &p.n_splits, &p.split_cols))
    throw std::runtime_error("the fused token probabilities do not take " + std::to_string(n) + " rows of " + std::to_string(d));
  const size_t rows_pad = ((size_t)n + p.row_tile - 1) / p.row_tile * p.row_tile;
  DeviceArray<float> xg = device_array<float>(row ? (size_t)n * d : 1), part = device_array<float>((size_t)2 * p.n_splits * n), target = device_array<float>(n);
  DeviceArray<h16> a = device_array<h16>(rows_pad * d);
  if (rows_pad > (size_t)n) HIP_CHECK(hipMemsetAsync(a + (size_t)n * d, 0, (rows_pad - n) * d * sizeof(h16), s));
  if (row) launch_prefill_gather_rows(x, row, xg, n, d, s);
  launch_layernorm_bf16(const_cast<float*>(row ? (const float*)xg : x), dec_ln_w_, dec_ln_b_, a, n, d, s);  // (no partials: x is read only)
  p.a = a; p.W = tok_emb_; p.n_vocab = cfg_.n_vocab; p.id = id; p.rows = n; p.d = d; p.eot = cfg_.eot;
  p.part_m = part; p.part_s = part + (size_t)p.n_splits * n; p.target = target; p.out = lp;
  launch_vocab_logprob(p, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));  // (the buffers leave scope)
}

void Engine::vocab_logprob_rows(const float* x, int n_rows, const int32_t* ids, float* out, int route) {
  require_no_stream("vocab_logprob_rows");
  if (!x || !ids || !out || n_rows < 1 || (route != kAlignLogProbRows && route != kAlignLogProbFused)) throw std::runtime_error("vocab_logprob_rows: bad arguments");
  if (cfg_.eot < 1 || cfg_.eot > cfg_.n_vocab) throw std::runtime_error("vocab_logprob_rows: the config's eot lies outside the vocabulary");
  for (int r = 0; r < n_rows; ++r)
    if (ids[r] < 0 || ids[r] >= cfg_.eot) throw std::runtime_error("vocab_logprob_rows: id " + std::to_string(ids[r]) + " of row " + std::to_string(r) + " is not below eot");
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = stream();
  const size_t d = (size_t)cfg_.n_text_state;
  DeviceArray<float> dx = device_array<float>(n_rows * d), lp = device_array<float>(n_rows);
  DeviceArray<int> did = device_array<int>(n_rows);
  HIP_CHECK(hipMemcpyAsync(dx, x, n_rows * d * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(did, ids, (size_t)n_rows * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (pageable sources)
  if (route == kAlignLogProbFused) token_logprob_fused(dx, nullptr, did, n_rows, lp, s);
  else token_logprob_rows(dx, nullptr, did, n_rows, lp, s);
  HIP_CHECK(hipMemcpyAsync(out, lp, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

void Engine::align_tokens(const AlignRequest& rq) {
  require_no_stream("align_tokens");
  require_timestamp_vocab();
  const int batch = rq.batch, Tc = cfg_.n_text_ctx, d = cfg_.n_text_state, n_lang = (int)cfg_.lang_tokens.size();
  if (batch < 1 || batch > cap_) throw std::runtime_error("align_tokens: batch exceeds the encoded slots");
  if (!rq.ids || rq.stride < 1 || !rq.n_ids || !rq.num_frames || !rq.jump || !rq.token_logprob)
    throw std::runtime_error("align_tokens: bad arguments");
  if (!prefill_supported()) throw std::runtime_error("align_tokens: the prefill kernels do not take this decoder shape");
  const int route = align_route(), lp_route = logprob_route(rq.logprob_route);
  if (route == 0 && Tc - 4 >= kAlignDtwThreads) throw std::runtime_error("align_tokens: the DTW kernel takes at most " + std::to_string(kAlignDtwThreads + 3) + " context rows");
  int translate = -1;
  {
    const auto tr = cfg_.ints.find("translate");
    if (tr != cfg_.ints.end() && tr->second >= 0 && tr->second < cfg_.n_vocab) translate = (int)tr->second;
  }
  // the clips that have something to align, and what each needs
  struct Clip { int b, n, L, F, lang_tok, task_tok; };
  std::vector<Clip> clips;
  for (int b = 0; b < batch; ++b) {
    const int n = rq.n_ids[b];
    if (n < 0 || n > rq.stride) throw std::runtime_error("align_tokens: id count " + std::to_string(n) + " of clip " + std::to_string(b) + " out of range");
    const int lg = rq.lang ? rq.lang[b] : -1, task = rq.task ? rq.task[b] : 0;
    if (lg < -1 || lg >= n_lang) throw std::runtime_error("language index " + std::to_string(lg) + " of clip " + std::to_string(b) + " is outside [-1, " + std::to_string(n_lang) + ")");
    if (task != 0 && task != 1) throw std::runtime_error("task " + std::to_string(task) + " of clip " + std::to_string(b) + " is neither 0 (transcribe) nor 1 (translate)");
    if (task == 1 && translate < 0) throw std::runtime_error("translate: the config has no translate id inside the vocabulary");
    if (n == 0) continue;
    if (n + 5 > Tc) throw std::runtime_error("align_tokens: " + std::to_string(n) + " ids of clip " + std::to_string(b) + " and their 5 context ids exceed n_text_ctx");
    const int F = rq.num_frames[b] / 2;
    if (rq.num_frames[b] < 0 || F < 1 || F > cfg_.n_audio_ctx) throw std::runtime_error("align_tokens: frame count " + std::to_string(rq.num_frames[b]) + " of clip " + std::to_string(b) + " out of range");
    for (int i = 0; i < n; ++i) {
      const int t = rq.ids[(size_t)b * rq.stride + i];
      if (t < 0 || t >= cfg_.eot) throw std::runtime_error("align_tokens: id " + std::to_string(t) + " of clip " + std::to_string(b) + " is not text");
    }
    if (rq.matrix && (rq.m_rows < n + 5 || rq.m_ld < F)) throw std::runtime_error("align_tokens: the matrix output is too small for clip " + std::to_string(b));
    clips.push_back(Clip{b, n, n + 5, F, lg >= 0 ? cfg_.lang_tokens[lg] : sot_seq_[1], task == 1 ? translate : sot_seq_[2]});
  }
  if (clips.empty()) return;

  // the aligned layers and their heads
  const std::vector<std::pair<int, int>> heads = alignment_heads();
  std::vector<std::vector<int>> layer_heads(cfg_.n_text_layer);
  for (const auto& lh : heads) layer_heads[lh.first].push_back(lh.second);
  size_t max_layer_heads = 0;
  for (const auto& v : layer_heads) max_layer_heads = std::max(max_layer_heads, v.size());
  const float inv_heads = 1.f / (float)heads.size();

  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = stream();
  const long cross_stride = (long)cfg_.n_text_head * layout::kv_head_elems(t_pad_);

  // chunks of consecutive clips whose P scratch fits the budget
  for (size_t c0 = 0; c0 < clips.size();) {
    size_t c1 = c0;
    int rows = 0, max_len = 0, max_f = 0;
    while (c1 < clips.size()) {
      const int ml = std::max(max_len, clips[c1].L), mf = std::max(max_f, clips[c1].F);
      const size_t bytes = (c1 - c0 + 1) * std::max<size_t>(max_layer_heads, 1) * ml * ((mf + 63) / 64 * 64) * 4;
      if (c1 > c0 && (bytes > kAlignScratchBytes || rows + clips[c1].L > kAlignChunkRows)) break;
      max_len = ml; max_f = mf; rows += clips[c1].L;
      ++c1;
    }
    const int n = (int)(c1 - c0), f_pad = (max_f + 63) / 64 * 64, rows_pad = max_len;
    // tables: the prefill pass's (context ids, positions, slots per row; first row, length, slot per clip) + the clips' frame counts,
    // the heads of every aligned layer, and the rows and ids of the token probabilities
    std::vector<int> ctx, row_pos, row_slot, row0(n), len(n), slot(n), zeros(n, 0), n_keys(n), lp_row, lp_id;
    for (int c = 0; c < n; ++c) {
      const Clip& k = clips[c0 + c];
      row0[c] = (int)ctx.size(); len[c] = k.L; slot[c] = k.b; n_keys[c] = k.F;
      const int32_t* t = rq.ids + (size_t)k.b * rq.stride;
      for (int i = 0; i < k.L; ++i) {
        ctx.push_back(i == 0 ? sot_seq_[0] : i == 1 ? k.lang_tok : i == 2 ? k.task_tok : i == 3 ? sot_seq_[3] : i < k.L - 1 ? (int)t[i - 4] : cfg_.eot);
        row_pos.push_back(i);
        row_slot.push_back(k.b);
      }
      for (int i = 0; i < k.n; ++i) { lp_row.push_back(row0[c] + 3 + i); lp_id.push_back((int)t[i]); }
    }
    ensure_prefill_scratch(rows, cap_);
    PrefillScratch& pf = prefill_;
    int *d_ctx = pf.row_tab, *d_row_pos = d_ctx + rows, *d_row_slot = d_row_pos + rows;
    int *d_row0 = pf.clip_tab, *d_len = d_row0 + n, *d_slot = d_len + n, *d_sot_row = d_slot + n;
    std::vector<int> head_tab;
    std::vector<int> head_off(cfg_.n_text_layer, 0);
    for (int l = 0; l < cfg_.n_text_layer; ++l) {
      head_off[l] = (int)head_tab.size();
      head_tab.insert(head_tab.end(), layer_heads[l].begin(), layer_heads[l].end());
    }
    const int n_lp = (int)lp_row.size();
    DeviceArray<int> d_nkeys = device_array<int>(n), d_heads = device_array<int>(head_tab.size()), d_lp_row = device_array<int>(n_lp),
                     d_lp_id = device_array<int>(n_lp), d_jump = device_array<int>((size_t)n * Tc);
    DeviceArray<float> P = device_array<float>((size_t)n * std::max<size_t>(max_layer_heads, 1) * rows_pad * f_pad),
                       matrix = device_array<float>((size_t)n * rows_pad * f_pad), d_lp = device_array<float>(n_lp);
    const long trace_stride = (long)(rows_pad - 3) * (max_f + 1);
    DeviceArray<uint8_t> trace = device_array<uint8_t>(route == 0 ? (size_t)n * trace_stride : 1);
    auto up = [&](int* dst, const std::vector<int>& src) { HIP_CHECK(hipMemcpyAsync(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice, s)); };
    up(d_ctx, ctx); up(d_row_pos, row_pos); up(d_row_slot, row_slot);
    up(d_row0, row0); up(d_len, len); up(d_slot, slot); up(d_sot_row, zeros);
    up(d_nkeys, n_keys); up(d_heads, head_tab); up(d_lp_row, lp_row); up(d_lp_id, lp_id);
    HIP_CHECK(hipMemsetAsync(matrix, 0, (size_t)n * rows_pad * f_pad * 4, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (pageable sources)

    std::vector<float> h_matrix, h_P;
    if (route == 1) h_matrix.assign((size_t)n * rows_pad * f_pad, 0.f);
    const LayerHook hook = [&](int l) {
      const int na = (int)layer_heads[l].size();
      if (na == 0) return;
      AlignQKParams q{};
      q.q = pf.qkv; q.ldq = d;
      q.k = d_cross_k_ + (size_t)l * cap_ * cross_stride; q.kv_slot_stride = cross_stride; q.keys_pad = t_pad_;
      q.row0 = d_row0; q.len = d_len; q.slot = d_slot; q.n_keys = d_nkeys;
      q.heads = d_heads + head_off[l]; q.n_align = na;
      q.P = P; q.rows_pad = rows_pad; q.f_pad = f_pad; q.n_clips = n; q.max_len = max_len;
      launch_align_qk_softmax(q, s);
      if (route == 0) {
        AlignNormParams m{};
        m.P = P; m.rows_pad = rows_pad; m.f_pad = f_pad; m.n_align = na; m.len = d_len; m.n_keys = d_nkeys;
        m.matrix = matrix; m.m_rows = rows_pad; m.m_ld = f_pad; m.inv_heads = inv_heads; m.n_clips = n; m.max_keys = max_f;
        launch_align_normalize(m, s);
      } else {
        const size_t count = (size_t)n * na * rows_pad * f_pad;
        h_P.resize(count);
        HIP_CHECK(hipMemcpyAsync(h_P.data(), P, count * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (int c = 0; c < n; ++c)
          align_normalize_host(h_P.data() + (size_t)c * na * rows_pad * f_pad, rows_pad, f_pad, na, len[c], n_keys[c],
                               h_matrix.data() + (size_t)c * rows_pad * f_pad, f_pad, inv_heads);
      }
    };
    prefill_pass(rows, n, max_len, false, &hook);

    // the path
    std::vector<int> h_jump((size_t)n * Tc, 0);
    if (route == 0) {
      AlignDtwParams w{};
      w.matrix = matrix; w.m_rows = rows_pad; w.m_ld = f_pad; w.len = d_len; w.n_keys = d_nkeys;
      w.trace = trace; w.trace_clip_stride = trace_stride; w.jump = d_jump; w.jump_ld = Tc; w.n_clips = n; w.max_len = max_len;
      launch_align_dtw(w, s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(h_jump.data(), d_jump, h_jump.size() * 4, hipMemcpyDeviceToHost, s));
      if (rq.matrix) {
        h_matrix.resize((size_t)n * rows_pad * f_pad);
        HIP_CHECK(hipMemcpyAsync(h_matrix.data(), matrix, h_matrix.size() * 4, hipMemcpyDeviceToHost, s));
      }
    } else {
      for (int c = 0; c < n; ++c)
        align_path(h_matrix.data() + ((size_t)c * rows_pad + 3) * f_pad, len[c] - 4, n_keys[c], f_pad, h_jump.data() + (size_t)c * Tc);
    }

    // token probabilities: the final residual rows of positions 3 .. n + 2
    if (lp_route == kAlignLogProbFused) token_logprob_fused(pf.x, d_lp_row, d_lp_id, n_lp, d_lp, s);
    else token_logprob_rows(pf.x, d_lp_row, d_lp_id, n_lp, d_lp, s);
    HIP_CHECK(hipGetLastError());
    std::vector<float> h_lp(n_lp);
    HIP_CHECK(hipMemcpyAsync(h_lp.data(), d_lp, (size_t)n_lp * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));

    for (int c = 0, at = 0; c < n; ++c) {
      const Clip& k = clips[c0 + c];
      std::copy(h_jump.begin() + (size_t)c * Tc, h_jump.begin() + (size_t)c * Tc + k.n + 1, rq.jump + (size_t)k.b * (rq.stride + 1));
      std::copy(h_lp.begin() + at, h_lp.begin() + at + k.n, rq.token_logprob + (size_t)k.b * rq.stride);
      at += k.n;
      if (rq.matrix)
        for (int i = 0; i < k.L; ++i)
          std::copy(h_matrix.begin() + ((size_t)c * rows_pad + i) * f_pad, h_matrix.begin() + ((size_t)c * rows_pad + i) * f_pad + k.F,
                    rq.matrix + ((size_t)k.b * rq.m_rows + i) * rq.m_ld);
    }
    c0 = c1;
  }
}

// One kernel alone on host data (tests). Needs the engine for its device and its 16-bit type.
void Engine::align_kernel(int which, const AlignKernelIO& io) {
  require_no_stream("align_kernel");
  const int n = io.n_clips;
  if (which < 0 || which > 2 || n < 1 || !io.len || !io.n_keys) throw std::runtime_error("align_kernel: bad arguments");
  int max_len = 0, max_keys = 0;
  for (int c = 0; c < n; ++c) {
    if (io.len[c] < 0 || io.n_keys[c] < 0) throw std::runtime_error("align_kernel: negative length");
    max_len = std::max(max_len, io.len[c]);
    max_keys = std::max(max_keys, io.n_keys[c]);
  }
  // every index a kernel forms is checked here
  if (which <= 1) {
    if (!io.P || io.n_align < 1 || io.rows_pad < max_len || io.f_pad % 64 != 0 || io.f_pad < max_keys) throw std::runtime_error("align_kernel: the P array does not hold the clips");
  }
  if (which >= 1) {
    if (!io.matrix || io.m_rows < max_len || io.m_ld < max_keys || io.m_ld % 4 != 0) throw std::runtime_error("align_kernel: the matrix does not hold the clips");
  }
  if (which == 0) {
    if (!io.q || !io.k || !io.row0 || !io.slot || !io.heads || io.n_head < 1 || io.keys_pad % 64 != 0 || io.keys_pad < max_keys || io.n_slots < 1)
      throw std::runtime_error("align_kernel: bad query or key arrays");
    for (int c = 0; c < n; ++c)
      if (io.row0[c] < 0 || io.row0[c] + io.len[c] > io.rows || io.slot[c] < 0 || io.slot[c] >= io.n_slots)
        throw std::runtime_error("align_kernel: a clip's rows or slot lie outside the arrays");
    for (int a = 0; a < io.n_align; ++a)
      if (io.heads[a] < 0 || io.heads[a] >= io.n_head) throw std::runtime_error("align_kernel: head out of range");
  }
  if (which == 2) {
    if (!io.jump || max_len - 4 >= kAlignDtwThreads) throw std::runtime_error("align_kernel: bad jump array or too many rows");
    for (int c = 0; c < n; ++c)
      if (io.len[c] - 4 > io.jump_ld) throw std::runtime_error("align_kernel: the jump array does not hold the clips");
  }
  std::lock_guard<std::recursive_mutex> capture_lock(device_capture_mutex(device_));
  HIP_CHECK(hipSetDevice(device_));
  hipStream_t s = stream();
  DeviceArray<int> d_len = device_array<int>(n), d_nkeys = device_array<int>(n);
  HIP_CHECK(hipMemcpyAsync(d_len, io.len, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_nkeys, io.n_keys, (size_t)n * 4, hipMemcpyHostToDevice, s));
  const size_t p_count = which <= 1 ? (size_t)n * io.n_align * io.rows_pad * io.f_pad : 1;
  const size_t m_count = which >= 1 ? (size_t)n * io.m_rows * io.m_ld : 1;
  DeviceArray<float> P = device_array<float>(p_count), matrix = device_array<float>(m_count);
  if (which <= 1) HIP_CHECK(hipMemcpyAsync(P, io.P, p_count * 4, hipMemcpyHostToDevice, s));
  if (which >= 1) HIP_CHECK(hipMemcpyAsync(matrix, io.matrix, m_count * 4, hipMemcpyHostToDevice, s));
  if (which == 0) {
    const int d = io.n_head * 64;
    const size_t q_count = (size_t)io.rows * d, head_elems = (size_t)layout::kv_head_elems(io.keys_pad), k_count = (size_t)io.n_slots * io.n_head * head_elems;
    std::vector<uint16_t> hq(q_count), hk(k_count);
    for (size_t i = 0; i < q_count; ++i) hq[i] = float_to_h16_bits(io.q[i]);
    for (int sl = 0; sl < io.n_slots; ++sl)
      for (int h = 0; h < io.n_head; ++h)
        for (int t = 0; t < io.keys_pad; ++t)
          for (int e = 0; e < 64; ++e)
            hk[((size_t)sl * io.n_head + h) * head_elems + layout::k_index(t, e)] = float_to_h16_bits(io.k[(((size_t)sl * io.n_head + h) * io.keys_pad + t) * 64 + e]);
    DeviceArray<h16> dq = device_array<h16>(q_count), dk = device_array<h16>(k_count);
    DeviceArray<int> d_row0 = device_array<int>(n), d_slot = device_array<int>(n), d_heads = device_array<int>(io.n_align);
    HIP_CHECK(hipMemcpyAsync(dq, hq.data(), q_count * 2, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dk, hk.data(), k_count * 2, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_row0, io.row0, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_slot, io.slot, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_heads, io.heads, (size_t)io.n_align * 4, hipMemcpyHostToDevice, s));
    AlignQKParams q{};
    q.q = dq; q.ldq = d; q.k = dk; q.kv_slot_stride = (long)io.n_head * head_elems; q.keys_pad = io.keys_pad;
    q.row0 = d_row0; q.len = d_len; q.slot = d_slot; q.n_keys = d_nkeys; q.heads = d_heads; q.n_align = io.n_align;
    q.P = P; q.rows_pad = io.rows_pad; q.f_pad = io.f_pad; q.n_clips = n; q.max_len = max_len;
    launch_align_qk_softmax(q, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(io.P, P, p_count * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the host arrays and the buffers leave scope)
  } else if (which == 1) {
    AlignNormParams m{};
    m.P = P; m.rows_pad = io.rows_pad; m.f_pad = io.f_pad; m.n_align = io.n_align; m.len = d_len; m.n_keys = d_nkeys;
    m.matrix = matrix; m.m_rows = io.m_rows; m.m_ld = io.m_ld; m.inv_heads = io.inv_heads; m.n_clips = n; m.max_keys = max_keys;
    launch_align_normalize(m, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(io.matrix, matrix, m_count * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  } else {
    const long trace_stride = (long)std::max(max_len - 3, 1) * (max_keys + 1);
    DeviceArray<uint8_t> trace = device_array<uint8_t>((size_t)n * trace_stride);
    DeviceArray<int> d_jump = device_array<int>((size_t)n * io.jump_ld);
    HIP_CHECK(hipMemcpyAsync(d_jump, io.jump, (size_t)n * io.jump_ld * 4, hipMemcpyHostToDevice, s));
    AlignDtwParams w{};
    w.matrix = matrix; w.m_rows = io.m_rows; w.m_ld = io.m_ld; w.len = d_len; w.n_keys = d_nkeys;
    w.trace = trace; w.trace_clip_stride = trace_stride; w.jump = d_jump; w.jump_ld = io.jump_ld; w.n_clips = n; w.max_len = max_len;
    launch_align_dtw(w, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(io.jump, d_jump, (size_t)n * io.jump_ld * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

}  // inline namespace AXW_NS
}  // namespace axw
