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
// log p(<|nospeech|>) over the unfiltered row. The unscored kernel is untouched by all of this.
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

// (m, s): logsumexp = m + log(s). m == -inf: empty; m == +inf: +inf (s is kept at 1)
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  if (m2 > m) {
    const float tm = m, ts = s;
    m = m2; s = s2; m2 = tm; s2 = ts;
  }
  if (m2 == -INFINITY) return;
  if (m == INFINITY) { s = 1.f; return; }
  s += s2 * expf(m2 - m);
}

// four logits at once (masked ones as -inf): the running maximum moves at most once per chunk
__device__ __forceinline__ void lse_add4(float& m, float& s, float x0, float x1, float x2, float x3) {
  const float cm = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
  if (cm == -INFINITY) return;
  if (cm > m) { s = m == -INFINITY ? 0.f : s * expf(m - cm); m = cm; }
  if (m == INFINITY) { s = 1.f; return; }
  s += (expf(x0 - m) + expf(x1 - m)) + (expf(x2 - m) + expf(x3 - m));
}

// (m, s) of the whole workgroup -> thread 0 (fixed order: lanes by xor butterfly, then waves 0..3)
__device__ __forceinline__ void lse_block_reduce(float& m, float& s, float* sh_m, float* sh_s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
  if (lane == 0) { sh_m[wave] = m; sh_s[wave] = s; }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w) lse_merge(m, s, sh_m[w], sh_s[w]);
}

// x - lse with the edge cases of the contract: nothing finite in the set: -inf; x = +inf: 0
__device__ __forceinline__ float logprob_of(float x, float m, float s) {
  if (m == -INFINITY || x == -INFINITY) return -INFINITY;
  if (x == INFINITY) return 0.f;
  return x - (m == INFINITY ? m : m + logf(s));
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

__global__ __launch_bounds__(256) void timestamp_rules_kernel(TsRulesParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int T = p.ts_begin, E = p.eot, nv = p.n_vocab;
  // only clips that sample at this step: past the prefix and not finished
  if (p.off && p.off[b] < p.n_prefix - 1) return;
  if (p.done && p.done[b]) return;

  // ---- the clip's history: ids sampled so far (prefix excluded)
  const int* seq;
  int n;
  if (p.forced) {
    seq = p.forced + (long)b * p.n_forced;
    n = min(max(p.off[b] - (p.n_prefix - 1), 0), p.n_forced);
  } else {
    seq = p.out_ids + (long)b * p.n_ctx;
    n = min(max(p.n_out[b], 0), p.n_ctx);
  }
  __shared__ int s_last[4];
  __shared__ float s_tv[4], s_sv[4], s_m[4], s_s[4];
  __shared__ int s_ti[4], s_si[4];
  int last = -1;  // index of the clip's last timestamp
  for (int i = tid; i < n; i += 256)
    if (seq[i] >= T) last = i;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) s_last[wave] = last;
  __syncthreads();
  last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
  const bool last_ts = n >= 1 && seq[n - 1] >= T;
  const bool penult_ts = n < 2 || seq[n - 2] >= T;
  const bool pair_open = last_ts && !penult_ts;  // one timestamp after text: the closing half of a pair may follow
  // ---- the allowed sets: [0, E) iff text_on, E iff eot_on, [E + 1, T) never, [ts_lo, ts_hi)
  const bool text_on = n > 0 && !pair_open;  // rules 2 (mask [0, E)) and 4
  const bool eot_on = n > 0;                 // rule 4
  int ts_lo = T, ts_hi = nv;
  if (last >= 0) ts_lo = min(max(seq[last], T) + (pair_open ? 0 : 1), nv);  // rule 3
  if (last_ts && penult_ts) ts_hi = T;                                       // rule 2: a pair just closed
  if (n == 0) ts_hi = min(ts_hi, T + 51);                                    // rule 4: <= 1.0 s
  ts_lo = min(ts_lo, ts_hi);

  const float* row = p.logits + (long)b * p.stride;
  float tv = -INFINITY, sv = -INFINITY, m = -INFINITY, s = 0.f;
  int ti = 0x7fffffff, si = 0x7fffffff;
  // text ids [0, E]: chunks of four floats; NaN never compares greater (it counts as masked)
  const int text_end = text_on ? E + 1 : (eot_on ? E + 1 : 0);
  const int text_begin = text_on ? 0 : (eot_on ? E : 0);
  for (int c = (text_begin >> 2) + tid; 4 * c < text_end; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      const bool on = i < E ? text_on : (i == E && eot_on);
      if (on && v[e] > tv) { tv = v[e]; ti = i; }
    }
  }
  for (int c = (ts_lo >> 2) + tid; 4 * c < ts_hi; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      if (i >= ts_lo && i < ts_hi && v[e] == v[e]) {
        if (v[e] > sv) { sv = v[e]; si = i; }
        lse_merge(m, s, v[e], 1.f);
      }
    }
  }
  // ---- reductions: first maximum wins (lower index on ties), logsumexp pairs merged in a fixed order
  wave_argmax(tv, ti);
  wave_argmax(sv, si);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
  if (lane == 0) { s_tv[wave] = tv; s_ti[wave] = ti; s_sv[wave] = sv; s_si[wave] = si; s_m[wave] = m; s_s[wave] = s; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      argmax_take(tv, ti, s_tv[w], s_ti[w]);
      argmax_take(sv, si, s_sv[w], s_si[w]);
      lse_merge(m, s, s_m[w], s_s[w]);
    }
    const float lse = (m == -INFINITY || m == INFINITY) ? m : m + logf(s);
    float bv = -INFINITY;
    int bi = E;  // nothing finite left: eot, the clip ends
    if (lse > tv) {  // rule 5: the timestamps' probability mass beats every single text id
      bv = sv; bi = si;
    } else if (tv > -INFINITY && tv >= sv) {
      bv = tv; bi = ti;
    } else if (sv > -INFINITY) {
      bv = sv; bi = si;
    }
    p.amax_val[(long)b * p.amax_stride] = bv;
    p.amax_idx[(long)b * p.amax_stride] = bi;
  }
}

// The scored form: timestamp_rules_kernel line for line, plus the text-range (max, sum), the no-speech branch and the score stores.
// A kernel of its own and not a template parameter of the one above: routed through a shared body, the unscored kernel came out
// of hipcc with another register allocation, and timestamp mode without scores is to keep the instructions it had.
__global__ __launch_bounds__(256) void timestamp_rules_scored_kernel(TsRulesParams p, TsScoreParams q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int T = p.ts_begin, E = p.eot, nv = p.n_vocab;
  // only clips that sample at this step: past the prefix and not finished
  if (p.off && p.off[b] < p.n_prefix - 1) {
    // the step that fed sot: the no-speech value of this clip
    if (q.no_speech && p.off[b] == 0) row_logprob(p.logits + (long)b * p.stride, p.n_vocab, q.no_speech_id, q.no_speech + b);
    return;
  }
  if (p.done && p.done[b]) return;

  // ---- the clip's history: ids sampled so far (prefix excluded)
  const int* seq;
  int n;
  if (p.forced) {
    seq = p.forced + (long)b * p.n_forced;
    n = min(max(p.off[b] - (p.n_prefix - 1), 0), p.n_forced);
  } else {
    seq = p.out_ids + (long)b * p.n_ctx;
    n = min(max(p.n_out[b], 0), p.n_ctx);
  }
  __shared__ int s_last[4];
  __shared__ float s_tv[4], s_sv[4], s_m[4], s_s[4];
  __shared__ int s_ti[4], s_si[4];
  int last = -1;  // index of the clip's last timestamp
  for (int i = tid; i < n; i += 256)
    if (seq[i] >= T) last = i;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) s_last[wave] = last;
  __syncthreads();
  last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
  const bool last_ts = n >= 1 && seq[n - 1] >= T;
  const bool penult_ts = n < 2 || seq[n - 2] >= T;
  const bool pair_open = last_ts && !penult_ts;  // one timestamp after text: the closing half of a pair may follow
  // ---- the allowed sets: [0, E) iff text_on, E iff eot_on, [E + 1, T) never, [ts_lo, ts_hi)
  const bool text_on = n > 0 && !pair_open;  // rules 2 (mask [0, E)) and 4
  const bool eot_on = n > 0;                 // rule 4
  int ts_lo = T, ts_hi = nv;
  if (last >= 0) ts_lo = min(max(seq[last], T) + (pair_open ? 0 : 1), nv);  // rule 3
  if (last_ts && penult_ts) ts_hi = T;                                       // rule 2: a pair just closed
  if (n == 0) ts_hi = min(ts_hi, T + 51);                                    // rule 4: <= 1.0 s
  ts_lo = min(ts_lo, ts_hi);

  const float* row = p.logits + (long)b * p.stride;
  float tv = -INFINITY, sv = -INFINITY, m = -INFINITY, s = 0.f;
  float mt = -INFINITY, st = 0.f;  // online logsumexp over the unmasked text ids and eot
  int ti = 0x7fffffff, si = 0x7fffffff;
  // text ids [0, E]: chunks of four floats; NaN never compares greater (it counts as masked)
  const int text_end = text_on ? E + 1 : (eot_on ? E + 1 : 0);
  const int text_begin = text_on ? 0 : (eot_on ? E : 0);
  for (int c = (text_begin >> 2) + tid; 4 * c < text_end; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      const bool on = i < E ? text_on : (i == E && eot_on);
      if (on && v[e] > tv) { tv = v[e]; ti = i; }
      x[e] = (on && v[e] == v[e]) ? v[e] : -INFINITY;
    }
    lse_add4(mt, st, x[0], x[1], x[2], x[3]);
  }
  for (int c = (ts_lo >> 2) + tid; 4 * c < ts_hi; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      if (i >= ts_lo && i < ts_hi && v[e] == v[e]) {
        if (v[e] > sv) { sv = v[e]; si = i; }
        lse_merge(m, s, v[e], 1.f);
      }
    }
  }
  // ---- reductions: first maximum wins (lower index on ties), logsumexp pairs merged in a fixed order
  wave_argmax(tv, ti);
  wave_argmax(sv, si);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
  __shared__ float s_mt[4], s_st[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(mt, o, 64), s2 = __shfl_xor(st, o, 64);
    lse_merge(mt, st, m2, s2);
  }
  if (lane == 0) { s_mt[wave] = mt; s_st[wave] = st; }
  if (lane == 0) { s_tv[wave] = tv; s_ti[wave] = ti; s_sv[wave] = sv; s_si[wave] = si; s_m[wave] = m; s_s[wave] = s; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      argmax_take(tv, ti, s_tv[w], s_ti[w]);
      argmax_take(sv, si, s_sv[w], s_si[w]);
      lse_merge(m, s, s_m[w], s_s[w]);
      lse_merge(mt, st, s_mt[w], s_st[w]);
    }
    const float lse = (m == -INFINITY || m == INFINITY) ? m : m + logf(s);
    float bv = -INFINITY;
    int bi = E;  // nothing finite left: eot, the clip ends
    if (lse > tv) {  // rule 5: the timestamps' probability mass beats every single text id
      bv = sv; bi = si;
    } else if (tv > -INFINITY && tv >= sv) {
      bv = tv; bi = ti;
    } else if (sv > -INFINITY) {
      bv = sv; bi = si;
    }
    p.amax_val[(long)b * p.amax_stride] = bv;
    p.amax_idx[(long)b * p.amax_stride] = bi;
    // A = the timestamps alone when rule 5 fired, else text, eot and timestamps (timestamp pair first: a fixed order)
    if (!(lse > tv)) lse_merge(m, s, mt, st);
    if (n < q.stride) {
      q.logprob[(long)b * q.stride + n] = logprob_of(bv, m, s);
      q.decision[(long)b * q.stride + n] = bi;
    }
  }
}

// log p(row[id]) over the whole row, one workgroup per row (the no-speech value on rows of the caller's)
__global__ __launch_bounds__(256) void row_logprob_kernel(const float* logits, long stride, int n_vocab, int id, float* out) {
  row_logprob(logits + (long)blockIdx.x * stride, n_vocab, id, out + blockIdx.x);
}

static void check_rules_params(const TsRulesParams& p) {
  if (p.stride % 4 != 0 || p.stride < p.n_vocab || p.ts_begin <= p.eot || p.ts_begin > p.n_vocab) {
    fprintf(stderr, "[ax_whisper] launch_timestamp_rules: unsupported row stride %ld / ids (eot %d, T %d, vocab %d)\n", p.stride, p.eot,
            p.ts_begin, p.n_vocab);
    abort();
  }
}

void launch_timestamp_rules(const TsRulesParams& p, hipStream_t s) {
  check_rules_params(p);
  hipLaunchKernelGGL(timestamp_rules_kernel, dim3(p.batch), dim3(256), 0, s, p);
}

void launch_timestamp_rules_scored(const TsRulesParams& p, const TsScoreParams& q, hipStream_t s) {
  check_rules_params(p);
  if (!q.logprob || !q.decision || q.stride < 1 || (q.no_speech && (q.no_speech_id < 0 || q.no_speech_id >= p.n_vocab))) {
    fprintf(stderr, "[ax_whisper] launch_timestamp_rules_scored: bad score arrays / no-speech id %d\n", q.no_speech_id);
    abort();
  }
  hipLaunchKernelGGL(timestamp_rules_scored_kernel, dim3(p.batch), dim3(256), 0, s, p, q);
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
