// decode_timestamps.hip — Whisper's timestamp rules between the logits launch and advance_kernel (DESIGN.md "Segment
// timestamps"). The rules decide, at every sampled step, which ids may follow the clip's history; rule 5 compares the
// logsumexp of the timestamp logits with the best text logit, so the choice cannot be made from argmax partials: the
// logits launch dumps the whole row and this kernel reads it once.
//
// One workgroup (four waves) per clip. One pass over the clip's fp32 row (16-byte loads; the row stride is a multiple of
// four floats) keeps, per thread: the first best unmasked id below T, the first best unmasked timestamp, and an online
// (max, sum) logsumexp over the unmasked timestamps. Wave reductions + LDS merge them; thread 0 applies rule 5 and writes
// ONE argmax partial per clip, which advance_kernel merges with n_part = 1 unchanged.
//
// Scored form (DESIGN.md "Confidence"): the same pass also keeps an online (max, sum) over the unmasked text ids and eot, so that
// thread 0 knows logsumexp of the final allowed set A and writes log p(chosen) = x[chosen] - logsumexp(x[A]) and the decision id
// at the clip's history length. At decode offset 0 (the step that fed sot) the scored launch takes the whole-row branch instead:
// log p(<|nospeech|>) over the unfiltered row.
//
// Sampled form (DESIGN.md "Temperature fallback"): the scored form whose decision, for a clip at temperature t > 0, is drawn from
// softmax(x[A] / t) by Gumbel-max with Philox4x32-10 noise: two more (key, id) pairs per thread (text and eot / timestamps, since
// rule 5 is only known after the reduction), reduced like the argmax pairs.
//
// Stream form (DESIGN.md "Slot stream in timestamp mode"): stream_rules_kernel, the scored form for slots that are refilled while the
// others decode: a slot whose done flag is set is left alone, offset 0 also picks the clip's language from the row when asked to.
//
// The three kernels are instantiations of one body, rules_body<MODE>: a lower form compiles none of what a higher one adds. The rules
// themselves, the logsumexp helpers and the decision are decode_rules.hpp's, shared with decode_beam.hip.
#include "decode_rules.hpp"

namespace axw {
inline namespace AXW_NS {

// (m, s) of the whole workgroup -> thread 0 (fixed order: lanes by xor butterfly, then waves 0..3)
__device__ __forceinline__ void lse_block_reduce(float& m, float& s, float* sh_m, float* sh_s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  lse_wave_reduce(m, s);
  if (lane == 0) { sh_m[wave] = m; sh_s[wave] = s; }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w) lse_merge(m, s, sh_m[w], sh_s[w]);
}

// log p(row[id]) over the WHOLE row (NaN entries left out), by one workgroup; thread 0 writes *out
__device__ __forceinline__ void row_logprob(const float* row, int nv, int id, float* out) {
  __shared__ float sh_m[4], sh_s[4];
  const int tid = threadIdx.x;
  float m = -INFINITY, s = 0.f;
  for (int c = tid; 4 * c < nv; c += 256) {  // (the row's stride is a multiple of four floats: the last chunk stays inside it)
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = (4 * c + e < nv && v[e] == v[e]) ? v[e] : -INFINITY;
    lse_add4(m, s, x[0], x[1], x[2], x[3]);
  }
  lse_block_reduce(m, s, sh_m, sh_s);
  if (tid == 0) *out = logprob_of(row[id], m, s);
}

// ---- sampled form's noise (DESIGN.md "Temperature fallback")
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): counter c, key k -> four words; no state in memory
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Gumbel-max key of one logit: x / t + g, g = -log(-log(u)), u = ((word >> 9) + 0.5) * 2^-23, never 0 or 1 (the accurate logf)
__device__ __forceinline__ float gumbel_key(float x, float t, unsigned word) {
  const float u = ((float)(word >> 9) + 0.5f) * 0x1p-23f;  // exact: 24 bits
  return x / t - logf(-logf(u));
}

// ---- the rules kernels: one body in three forms, each of which has everything the one before it has
enum RulesMode { kRulesPlain, kRulesScored, kRulesSampled };

// kRulesPlain: the argmax partial alone (q and r are not read). kRulesScored: plus the (max, sum) pair of the unmasked ids of
// [0, E], the no-speech branch and the score stores of q. kRulesSampled: plus, for a clip whose temperature is above 0, two Gumbel
// (key, id) pairs per thread: the decision is drawn from softmax(x[A] / t) over the final allowed set A, as argmax of x / t + Gumbel
// noise, the noise of id i at history length n being word i & 3 of Philox(counter (i >> 2, n, stream), key seed), whatever the
// suppress set (p.suppress; decode_rules.hpp) holds: a suppressed id is masked like one that a rule masks. Rules 1 to 5 are
// decided on the untempered logits and the recorded log-probability is the untempered one; a clip with t <= 0 takes the scored
// form's decision and computes no random number.
// kSet: the instantiation of a launch with a suppress set, mask its words. Without one (kSet false, mask not read) the body compiles to
// what it was before there were sets: the kernels below exist in both forms and the launch functions choose by TsRulesParams::suppress.
template <RulesMode MODE, bool kSet>
__device__ __forceinline__ void rules_body(const TsRulesArgs& p, const unsigned* mask, const TsScoreParams& q, const TsSampleParams& r) {
  constexpr bool kScore = MODE >= kRulesScored, kSample = MODE == kRulesSampled;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int T = p.ts_begin, E = p.eot;
  // only clips that sample at this step: past the prefix and not finished
  if (p.off && p.off[b] < p.n_prefix - 1) {
    // the step that fed sot: the no-speech value of this clip
    if constexpr (kScore)
      if (q.no_speech && p.off[b] == 0) row_logprob(p.logits + (long)b * p.stride, p.n_vocab, q.no_speech_id, q.no_speech + b);
    return;
  }
  if (p.done && p.done[b]) return;
  const RulesHistory h = rules_history(p, b);
  const int n = h.n;
  const AllowedSets a = allowed_sets(h.seq, n, T, E, p.n_vocab);

  // ---- the clip's temperature and random stream (uniform over the workgroup)
  float temp = 0.f;
  unsigned k0 = 0, k1 = 0, c2 = 0, c3 = 0;
  if constexpr (kSample) {
    temp = r.temperature[b];
    const unsigned long long sid = r.stream[b], seed = r.seed[0];
    k0 = (unsigned)seed; k1 = (unsigned)(seed >> 32); c2 = (unsigned)sid; c3 = (unsigned)(sid >> 32);
  }
  const bool draw = kSample && temp > 0.f;

  // ---- one pass over the row
  const float* row = p.logits + (long)b * p.stride;
  [[maybe_unused]] const unsigned* suppress = nullptr;
  if constexpr (kSet) suppress = suppress_stage(mask, E);
  float tv = -INFINITY, sv = -INFINITY;  // the first best unmasked id of [0, E] / unmasked timestamp
  int ti = 0x7fffffff, si = 0x7fffffff;
  float m = -INFINITY, s = 0.f;          // online logsumexp over the unmasked timestamps
  float mt = -INFINITY, st = 0.f;        // scored: online logsumexp over the unmasked text ids and eot
  float gt = -INFINITY, gs = -INFINITY;  // a clip that draws: best Gumbel key over the unmasked text ids and eot / timestamps
  int gti = 0x7fffffff, gsi = 0x7fffffff;
  // text ids [0, E]: chunks of four floats; NaN never compares greater (it counts as masked)
  for (int c = (a.text_begin >> 2) + tid; 4 * c < a.text_end; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    [[maybe_unused]] unsigned sup = 0;
    if constexpr (kSet) sup = suppress_bits4(suppress, c);
    [[maybe_unused]] float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      bool on = text_id_on(a, i, E);
      if constexpr (kSet) on = on && !suppressed(sup, e);
      if (on && v[e] > tv) { tv = v[e]; ti = i; }
      x[e] = (on && v[e] == v[e]) ? v[e] : -INFINITY;
    }
    if constexpr (kScore) lse_add4(mt, st, x[0], x[1], x[2], x[3]);
    if (draw) {
      unsigned w[4];
      philox4x32_10((unsigned)c, (unsigned)n, c2, c3, k0, k1, w);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float key = gumbel_key(x[e], temp, w[e]);  // (a masked id: -inf)
        if (key > gt) { gt = key; gti = 4 * c + e; }
      }
    }
  }
  for (int c = (a.ts_lo >> 2) + tid; 4 * c < a.ts_hi; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    unsigned w[4];
    if (draw) philox4x32_10((unsigned)c, (unsigned)n, c2, c3, k0, k1, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      if (timestamp_on(a, i) && v[e] == v[e]) {
        if (v[e] > sv) { sv = v[e]; si = i; }
        lse_merge(m, s, v[e], 1.f);
        if (draw) {
          const float key = gumbel_key(v[e], temp, w[e]);
          if (key > gs) { gs = key; gsi = i; }
        }
      }
    }
  }
  // ---- reductions: first maximum wins (lower index on ties), logsumexp pairs merged in a fixed order (lanes by xor butterfly,
  // then waves 0..3); thread 0 ends with the workgroup's values
  __shared__ float s_tv[4], s_sv[4], s_m[4], s_s[4], s_mt[4], s_st[4], s_gt[4], s_gs[4];
  __shared__ int s_ti[4], s_si[4], s_gti[4], s_gsi[4];
  wave_argmax(tv, ti);
  wave_argmax(sv, si);
  lse_wave_reduce(m, s);
  if constexpr (kScore) lse_wave_reduce(mt, st);
  if (draw) {
    wave_argmax(gt, gti);
    wave_argmax(gs, gsi);
    if (lane == 0) { s_gt[wave] = gt; s_gti[wave] = gti; s_gs[wave] = gs; s_gsi[wave] = gsi; }
  }
  if constexpr (kScore)
    if (lane == 0) { s_mt[wave] = mt; s_st[wave] = st; }
  if (lane == 0) { s_tv[wave] = tv; s_ti[wave] = ti; s_sv[wave] = sv; s_si[wave] = si; s_m[wave] = m; s_s[wave] = s; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < 4; ++w) {
    argmax_take(tv, ti, s_tv[w], s_ti[w]);
    argmax_take(sv, si, s_sv[w], s_si[w]);
    lse_merge(m, s, s_m[w], s_s[w]);
    if constexpr (kScore) lse_merge(mt, st, s_mt[w], s_st[w]);
    if (draw) {
      argmax_take(gt, gti, s_gt[w], s_gti[w]);
      argmax_take(gs, gsi, s_gs[w], s_gsi[w]);
    }
  }
  // ---- the decision: the winner of the final allowed set by logit, or by key for a clip that draws
  const bool rule5 = rule5_fires(m, s, tv);
  float bv = -INFINITY;
  int bi = E;
  const Pick pick = final_pick(rule5, draw ? gt : tv, draw ? gs : sv);
  if (pick == Pick::kText) { bi = draw ? gti : ti; bv = draw ? row[bi] : tv; }
  if (pick == Pick::kTimestamp) { bi = draw ? gsi : si; bv = draw ? row[bi] : sv; }
  p.amax_val[(long)b * p.amax_stride] = bv;
  p.amax_idx[(long)b * p.amax_stride] = bi;
  if constexpr (kScore) {
    final_set_merge(rule5, m, s, mt, st);
    if (n < q.stride) {
      q.logprob[(long)b * q.stride + n] = logprob_of(bv, m, s);
      q.decision[(long)b * q.stride + n] = bi;
    }
  }
}

__global__ __launch_bounds__(256) void timestamp_rules_kernel(TsRulesArgs p) { rules_body<kRulesPlain, false>(p, nullptr, TsScoreParams{}, TsSampleParams{}); }

__global__ __launch_bounds__(256) void timestamp_rules_scored_kernel(TsRulesArgs p, TsScoreParams q) {
  rules_body<kRulesScored, false>(p, nullptr, q, TsSampleParams{});
}

__global__ __launch_bounds__(256) void timestamp_rules_sampled_kernel(TsRulesArgs p, TsScoreParams q, TsSampleParams r) {
  rules_body<kRulesSampled, false>(p, nullptr, q, r);
}

// the same three under a suppress set (dynamic LDS: suppress_lds_bytes)
__global__ __launch_bounds__(256) void timestamp_rules_suppress_kernel(TsRulesArgs p, const unsigned* mask) {
  rules_body<kRulesPlain, true>(p, mask, TsScoreParams{}, TsSampleParams{});
}

__global__ __launch_bounds__(256) void timestamp_rules_scored_suppress_kernel(TsRulesArgs p, const unsigned* mask, TsScoreParams q) {
  rules_body<kRulesScored, true>(p, mask, q, TsSampleParams{});
}

__global__ __launch_bounds__(256) void timestamp_rules_sampled_suppress_kernel(TsRulesArgs p, const unsigned* mask, TsScoreParams q, TsSampleParams r) {
  rules_body<kRulesSampled, true>(p, mask, q, r);
}

// ---- slot stream in timestamp mode (DESIGN.md "Slot stream in timestamp mode"): the scored form for slots that are refilled while
// the others decode. One workgroup per slot; every branch below is uniform over the workgroup.
//   done[b] set (idle, or finished and not yet refilled): NOTHING, checked before the offset — an idle slot rests at offset 0 with a
//     stale row, and the scored kernel's order (offset first) would overwrite its no-speech value and detect a language nobody asked for;
//   offset 0: no_speech[b] as the scored kernel writes it; with detect[b], openai-whisper's detect_language from the same row (the
//     context is [sot] at position 0 over the clip's own cross K/V): thread j < n_lang gathers row[lang_tokens[j]] into LDS; wave 0
//     then holds languages l and l + 64 in lane l and takes the first maximum in list order (NaN never wins; lanes by xor butterfly)
//     and sum exp(x - max) over the entries that are not NaN (lanes by xor butterfly: decode_language.hip step 3, the same arithmetic);
//     lang_logprob[j] = x[j] - (max + log sum), -inf for NaN; nothing finite: fallback_index, every value -inf. Lane 0 writes
//     slot_ctx[4 b + 1], which this step's advance launch feeds next on the same stream: no extra pass, no host round trip;
//   offset 1 (the language id was fed): nothing;
//   offset >= n_prefix - 1: rules_body<kRulesScored>, whose own offset and done tests then pass.
__global__ __launch_bounds__(256) void stream_rules_kernel(TsRulesArgs p, TsScoreParams q, StreamRulesParams t) {
#define AXW_STREAM_SET false
#define AXW_STREAM_MASK nullptr
#include "stream_rules_body.inc"
#undef AXW_STREAM_SET
#undef AXW_STREAM_MASK
}

__global__ __launch_bounds__(256) void stream_rules_suppress_kernel(TsRulesArgs p, const unsigned* mask, TsScoreParams q, StreamRulesParams t) {
#define AXW_STREAM_SET true
#define AXW_STREAM_MASK mask
#include "stream_rules_body.inc"
#undef AXW_STREAM_SET
#undef AXW_STREAM_MASK
}

// log p(row[id]) over the whole row, one workgroup per row (the no-speech value on rows of the caller's)
__global__ __launch_bounds__(256) void row_logprob_kernel(const float* logits, long stride, int n_vocab, int id, float* out) {
  row_logprob(logits + (long)blockIdx.x * stride, n_vocab, id, out + blockIdx.x);
}

// dynamic LDS of a rules launch under a set: the image of the suppress mask's words of [0, eot] (decode_rules.hpp: suppress_stage)
static size_t suppress_lds_bytes(const TsRulesParams& p) { return ((size_t)(p.eot >> 5) + 1) * sizeof(unsigned); }
// (the kernels take the arguments without the set: a launch without one is the launch it was before there were sets)
static const TsRulesArgs& args_of(const TsRulesParams& p) { return p; }

static void check_rules_params(const TsRulesParams& p) {
  if (p.stride % 4 != 0 || p.stride < p.n_vocab || p.ts_begin <= p.eot || p.ts_begin > p.n_vocab) {
    fprintf(stderr, "[ax_whisper] launch_timestamp_rules: unsupported row stride %ld / ids (eot %d, T %d, vocab %d)\n", p.stride, p.eot,
            p.ts_begin, p.n_vocab);
    abort();
  }
}

void launch_timestamp_rules(const TsRulesParams& p, hipStream_t s) {
  check_rules_params(p);
  if (p.suppress) hipLaunchKernelGGL(timestamp_rules_suppress_kernel, dim3(p.batch), dim3(256), suppress_lds_bytes(p), s, args_of(p), p.suppress);
  else hipLaunchKernelGGL(timestamp_rules_kernel, dim3(p.batch), dim3(256), 0, s, args_of(p));
}

static bool score_params_ok(const TsRulesParams& p, const TsScoreParams& q) {
  return q.logprob && q.decision && q.stride >= 1 && (!q.no_speech || (q.no_speech_id >= 0 && q.no_speech_id < p.n_vocab));
}

void launch_timestamp_rules_scored(const TsRulesParams& p, const TsScoreParams& q, hipStream_t s) {
  check_rules_params(p);
  if (!score_params_ok(p, q)) {
    fprintf(stderr, "[ax_whisper] launch_timestamp_rules_scored: bad score arrays / no-speech id %d\n", q.no_speech_id);
    abort();
  }
  if (p.suppress) hipLaunchKernelGGL(timestamp_rules_scored_suppress_kernel, dim3(p.batch), dim3(256), suppress_lds_bytes(p), s, args_of(p), p.suppress, q);
  else hipLaunchKernelGGL(timestamp_rules_scored_kernel, dim3(p.batch), dim3(256), 0, s, args_of(p), q);
}

void launch_timestamp_rules_sampled(const TsRulesParams& p, const TsScoreParams& q, const TsSampleParams& r, hipStream_t s) {
  check_rules_params(p);
  if (!score_params_ok(p, q) || !r.temperature || !r.stream || !r.seed) {
    fprintf(stderr, "[ax_whisper] launch_timestamp_rules_sampled: bad score or sample arrays / no-speech id %d\n", q.no_speech_id);
    abort();
  }
  if (p.suppress) hipLaunchKernelGGL(timestamp_rules_sampled_suppress_kernel, dim3(p.batch), dim3(256), suppress_lds_bytes(p), s, args_of(p), p.suppress, q, r);
  else hipLaunchKernelGGL(timestamp_rules_sampled_kernel, dim3(p.batch), dim3(256), 0, s, args_of(p), q, r);
}

void launch_stream_rules(const TsRulesParams& p, const TsScoreParams& q, const StreamRulesParams& t, hipStream_t s) {
  check_rules_params(p);
  if (!score_params_ok(p, q) || !q.no_speech || !p.off || !p.done || p.forced || !t.detect || !t.slot_ctx || !t.lang_tokens || !t.lang_out ||
      !t.lang_logprob || t.n_lang < 1 || t.n_lang > kLangMax || t.fallback_index < 0 || t.fallback_index >= t.n_lang) {
    fprintf(stderr, "[ax_whisper] launch_stream_rules: bad score or slot arrays / n_lang %d\n", t.n_lang);
    abort();
  }
  if (p.suppress) hipLaunchKernelGGL(stream_rules_suppress_kernel, dim3(p.batch), dim3(256), suppress_lds_bytes(p), s, args_of(p), p.suppress, q, t);
  else hipLaunchKernelGGL(stream_rules_kernel, dim3(p.batch), dim3(256), 0, s, args_of(p), q, t);
}

void launch_row_logprob(const float* logits, long stride, int n_vocab, int id, int batch, float* out, hipStream_t s) {
  if (stride % 4 != 0 || stride < n_vocab || id < 0 || id >= n_vocab) {
    fprintf(stderr, "[ax_whisper] launch_row_logprob: unsupported row stride %ld / id %d (vocab %d)\n", stride, id, n_vocab);
    abort();
  }
  hipLaunchKernelGGL(row_logprob_kernel, dim3(batch), dim3(256), 0, s, logits, stride, n_vocab, id, out);
}

}  // inline namespace AXW_NS
}  // namespace axw
