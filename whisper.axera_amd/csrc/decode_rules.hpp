// decode_rules.hpp — Whisper's timestamp rules as device functions: the one statement of what decode_timestamps.hip (the plain,
// scored and sampled rules kernels) and decode_beam.hip (beam_candidates_kernel) decide alike. Shared: the logsumexp helpers, the
// way from a history to the allowed sets (rules 2, 3 and 4), the history selection of TsRulesParams, and rule 5 with the final-set
// merge and the pick of the winner. A change to a rule is made here and reaches all four kernels. Not shared: the loops over the
// row. The rules kernels keep one winner per range and add the timestamps to their (max, sum) pair one by one; the beam kernel
// feeds sorted lists and adds the timestamps in chunks of four, which rounds differently, and each form keeps its bits.
// Every function that holds a barrier is called by all 256 threads of the workgroup (four waves) or by none.
#pragma once
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

// ---- logsumexp as an online (m, s) pair: value = m + log(s). m == -inf: empty; m == +inf: +inf (s is kept at 1)
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

// the pairs of a wave's lanes -> every lane (fixed order: xor butterfly)
__device__ __forceinline__ void lse_wave_reduce(float& m, float& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
}

__device__ __forceinline__ float lse_value(float m, float s) { return (m == -INFINITY || m == INFINITY) ? m : m + logf(s); }

// x - lse with the edge cases of the contract: nothing finite in the set: -inf; x = +inf: 0
__device__ __forceinline__ float logprob_of(float x, float m, float s) {
  if (m == -INFINITY || x == -INFINITY) return -INFINITY;
  if (x == INFINITY) return 0.f;
  return x - (m == INFINITY ? m : m + logf(s));
}

// ---- the history of clip b under TsRulesParams: the ids sampled so far (prefix excluded), teacher-forced or greedy
struct RulesHistory {
  const int* seq;
  int n;
};
__device__ __forceinline__ RulesHistory rules_history(const TsRulesArgs& p, int b) {
  if (p.forced) return {p.forced + (long)b * p.n_forced, min(max(p.off[b] - (p.n_prefix - 1) - (p.base ? p.base[b] : 0), 0), p.n_forced)};
  return {p.out_ids + (long)b * p.n_ctx, min(max(p.n_out[b], 0), p.n_ctx)};
}

// ---- the allowed sets after a history: [0, E) iff text_on, E iff eot_on, [E + 1, T) never, [ts_lo, ts_hi)
struct AllowedSets {
  bool text_on, eot_on;
  int ts_lo, ts_hi;
  int text_begin, text_end;  // the part of [0, E] that a row loop has to visit (empty: 0, 0)
};
// T: id of 0.00 s, E: eot, nv: the vocabulary. One barrier.
__device__ __forceinline__ AllowedSets allowed_sets(const int* seq, int n, int T, int E, int nv) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int s_last[4];
  int last = -1;  // index of the history's last timestamp
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
  AllowedSets a;
  a.text_on = n > 0 && !pair_open;  // rules 2 (mask [0, E)) and 4
  a.eot_on = n > 0;                 // rule 4
  a.ts_lo = T;
  a.ts_hi = nv;
  if (last >= 0) a.ts_lo = min(max(seq[last], T) + (pair_open ? 0 : 1), nv);  // rule 3
  if (last_ts && penult_ts) a.ts_hi = T;                                       // rule 2: a pair just closed
  if (n == 0) a.ts_hi = min(a.ts_hi, T + 51);                                  // rule 4: <= 1.0 s
  a.ts_lo = min(a.ts_lo, a.ts_hi);
  a.text_end = a.text_on ? E + 1 : (a.eot_on ? E + 1 : 0);
  a.text_begin = a.text_on ? 0 : (a.eot_on ? E : 0);
  return a;
}
// The same sets for a loop that carries the history's four values instead of its ids (the persistent launch's rules instantiation,
// decode_persistent_rules.hpp): n, the id of the last timestamp (any value below T: none), whether the last id is a timestamp and
// whether the one before it is (neither is read where the history is too short). No barrier, no memory.
__device__ __forceinline__ AllowedSets allowed_sets_from_state(int n, int last_ts_id, bool last_is_ts, bool penult_is_ts, int T, int E, int nv) {
  const bool last_ts = n >= 1 && last_is_ts;
  const bool penult_ts = n < 2 || penult_is_ts;
  const bool pair_open = last_ts && !penult_ts;
  AllowedSets a;
  a.text_on = n > 0 && !pair_open;
  a.eot_on = n > 0;
  a.ts_lo = T;
  a.ts_hi = nv;
  if (n >= 1 && last_ts_id >= T) a.ts_lo = min(last_ts_id + (pair_open ? 0 : 1), nv);
  if (last_ts && penult_ts) a.ts_hi = T;
  if (n == 0) a.ts_hi = min(a.ts_hi, T + 51);
  a.ts_lo = min(a.ts_lo, a.ts_hi);
  a.text_end = a.text_on ? E + 1 : (a.eot_on ? E + 1 : 0);
  a.text_begin = a.text_on ? 0 : (a.eot_on ? E : 0);
  return a;
}
__device__ __forceinline__ bool text_id_on(const AllowedSets& a, int i, int E) { return i < E ? a.text_on : (i == E && a.eot_on); }
__device__ __forceinline__ bool timestamp_on(const AllowedSets& a, int i) { return i >= a.ts_lo && i < a.ts_hi; }

// ---- token suppression (DESIGN.md "Token suppression"): a suppressed id counts as -inf before rules 2 to 5. mask: bit i & 31 of
// word i >> 5 is set iff id i is suppressed, whole 16-byte groups of words over the vocabulary; the host leaves every bit from eot
// up clear, so eot needs no case of its own and only the text loops look. nullptr: no set (uniform over the workgroup).
// The four bits of the 16-byte chunk c of a row (ids 4 c .. 4 c + 3); mask: the words in global memory or an LDS image of them.
__device__ __forceinline__ unsigned suppress_bits4(const unsigned* mask, int c) { return (mask[c >> 3] >> ((c & 7) * 4)) & 15u; }

__device__ __forceinline__ bool suppressed(unsigned bits4, int e) { return (bits4 >> e) & 1u; }
// The words of ids [0, E] -> an image in the launch's dynamic LDS (suppress_lds_bytes), which is returned. One barrier: called by
// all 256 threads. Only the kernels' instantiation with a set holds a call.
// Measured per step with the 82 non-speech ids (profiles/suppress_tokens_bench.txt): the rules kernels are faster with the image
// (their loop waits for one dependent word per chunk otherwise), the beam kernel with the words read in its loop, so rules_body
// stages and beam_candidates_kernel does not.
__device__ __forceinline__ const unsigned* suppress_stage(const unsigned* mask, int E) {
  extern __shared__ unsigned s_suppress[];
  for (int i = threadIdx.x; i <= (E >> 5); i += 256) s_suppress[i] = mask[i];
  __syncthreads();
  return s_suppress;
}

// ---- rule 5 and the final allowed set A. (m, s): the pair of the unmasked timestamps; tv: the best unmasked id of [0, E]
// rule 5: the timestamps' probability mass beats every single text id
__device__ __forceinline__ bool rule5_fires(float m, float s, float tv) { return lse_value(m, s) > tv; }
// (m, s) -> the pair of A: the timestamps alone when rule 5 fired, else timestamps, text and eot (timestamp pair first: a fixed
// order); (mt, st): the pair of the unmasked ids of [0, E]
__device__ __forceinline__ void final_set_merge(bool rule5, float& m, float& s, float mt, float st) {
  if (!rule5) lse_merge(m, s, mt, st);
}
// The winner of A from the winners (value or key, id) of [0, E] and of the timestamps: the timestamps' when rule 5 fired, else
// the larger one (text ids are the lower ones: text on ties). Nothing above -inf: eot with -inf, the clip ends.
enum class Pick { kEot, kText, kTimestamp };
__device__ __forceinline__ Pick final_pick(bool rule5, float tv, float sv) {
  if (!rule5 && tv > -INFINITY && tv >= sv) return Pick::kText;
  return sv > -INFINITY ? Pick::kTimestamp : Pick::kEot;
}

}  // inline namespace AXW_NS
}  // namespace axw
