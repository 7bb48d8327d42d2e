// decode_persistent_rules.hpp — the timestamp rules inside the one-clip persistent launch: what the rules
// instantiation of decode_persistent_kernel adds to the plain one. The rules need, per step, rule 5 (the timestamps' probability mass
// against the best text logit), the final set's normaliser and the winner. All of them come from quantities that merge
// associatively, so a workgroup publishes them for its own vocabulary range in the hand-off that carries the argmax pair of the
// plain launch: one record of eight words instead of one pair,
//   tv, ti   first-best allowed id of [0, E]            sv, si   first-best allowed timestamp
//   mt, st   (max, sum) of the allowed ids of [0, E]    m, s     (max, sum) of the allowed timestamps
// NaN counts as masked, ties go to the lower index, a suppressed text id counts as -inf (rules_body, decode_timestamps.hip).
// The history is not scanned: allowed_sets_from_state (decode_rules.hpp) needs four values, which every workgroup carries.
// The decision is decode_rules.hpp's: rule5_fires, final_set_merge, final_pick, logprob_of.
// Every merge order below depends on lane, wave and workgroup indices alone: every workgroup derives the same bits from the same
// P records, and with them the same token.
#pragma once
#include "decode_persistent_common.hpp"
#include "decode_rules.hpp"

namespace axw {
inline namespace AXW_NS {

constexpr int kRecWords = 8;      // granules of a workgroup's record: four adjacent pairs, half a 128-byte line
constexpr int kRulesSupWords = 64;  // LDS image of the suppress mask over the workgroup's own rows: at most 2048 - 32 rows per workgroup
// LDS of the rules instantiation behind the plain launch's carve-up (128 bytes of slack, then four word arrays):
//   rec_c [NCW][8] the compute waves' records, rec_p [NPW][8] the poller waves' (resident rows), rec_g [NPW][4] the gather's wave
//   results (waves 0-3: tv, ti, sv, si; waves 4-7: mt, st, m, s), sup [kRulesSupWords]
constexpr int kRulesLdsWords = NCW * kRecWords + NPW * kRecWords + NPW * 4 + kRulesSupWords;
constexpr size_t kRulesLdsBytes = 128 + (size_t)kRulesLdsWords * 4;
// rows per workgroup the image covers (host: the route's precondition)
constexpr int kRulesMaxRange = kRulesSupWords * 32 - 32;

struct RulesRec {
  float tv; int ti;
  float sv; int si;
  float mt, st, m, s;
};
__device__ __forceinline__ RulesRec rules_rec_empty() { return {-INFINITY, 0x7fffffff, -INFINITY, 0x7fffffff, -INFINITY, 0.f, -INFINITY, 0.f}; }

// one logit of the row under the allowed sets; sup: the id's suppress bit (read for text ids only)
__device__ __forceinline__ void rules_rec_take(RulesRec& r, const AllowedSets& a, float x, int row, int E, bool sup) {
  if (row <= E) {
    const bool on = text_id_on(a, row, E) && !sup;
    if (on && x > r.tv) { r.tv = x; r.ti = row; }
    if (on && x == x) lse_merge(r.mt, r.st, x, 1.f);
  } else if (timestamp_on(a, row) && x == x) {
    if (x > r.sv) { r.sv = x; r.si = row; }
    lse_merge(r.m, r.s, x, 1.f);
  }
}
// the step that fed sot (scored mode): the whole row is the one set (mt, st); the <|nospeech|> logit travels as sv. A NaN logit
// (non-finite audio) cannot win a merge, so it travels as a mark in (tv, ti), which this step does not use otherwise: the value is
// then NaN, as row_logprob's x - logsumexp gives (decode_timestamps.hip)
__device__ __forceinline__ void rules_rec_take_whole(RulesRec& r, float x, int row, int no_speech_id) {
  if (x == x) lse_merge(r.mt, r.st, x, 1.f);
  if (row == no_speech_id) {
    if (x > r.sv) { r.sv = x; r.si = row; }
    if (x != x) { r.tv = 0.f; r.ti = row; }
  }
}
// no_speech_logprob from the grid's record of that step
__device__ __forceinline__ float rules_no_speech_logprob(const RulesRec& g) {
  return g.tv > -INFINITY ? __builtin_nanf("") : logprob_of(g.sv, g.mt, g.st);
}

// What a step's row loops need besides the row: the allowed sets, or `whole` for the step that fed sot; w0: first word of the LDS
// image of the suppress mask (the word of the workgroup's first row). Uniform over the workgroup.
struct RulesStep {
  AllowedSets a;
  int E, no_speech_id, w0;
  bool whole;
};
// sup: the image (zeros without a set)
__device__ __forceinline__ void rules_rec_row(RulesRec& r, const RulesStep& q, const unsigned* sup, float x, int row) {
  if (q.whole) {
    rules_rec_take_whole(r, x, row, q.no_speech_id);
  } else {
    const bool bit = row <= q.E && ((sup[(row >> 5) - q.w0] >> (row & 31)) & 1u);
    rules_rec_take(r, q.a, x, row, q.E, bit);
  }
}

// (m, s) of a wave's lanes -> every lane: the butterfly of wave_argmax (DPP inside a row, permlane swaps across rows; the
// __shfl_xor form of lse_wave_reduce is six dependent ds_bpermute round trips on the token's path). Every lane active.
__device__ __forceinline__ void lse_wave_reduce_dpp(float& m, float& s) {
#define AXW_LSE_STEP(CTRL) { const float m2 = dpp_mov<CTRL>(m), s2 = dpp_mov<CTRL>(s); lse_merge(m, s, m2, s2); }
  AXW_LSE_STEP(0xB1)
  AXW_LSE_STEP(0x4E)
  AXW_LSE_STEP(0x141)
  AXW_LSE_STEP(0x140)
#undef AXW_LSE_STEP
  {
    auto rm = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    auto rs = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    m = __uint_as_float(rm[0]); s = __uint_as_float(rs[0]);
    lse_merge(m, s, __uint_as_float(rm[1]), __uint_as_float(rs[1]));
  }
  {
    auto rm = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    auto rs = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    m = __uint_as_float(rm[0]); s = __uint_as_float(rs[0]);
    lse_merge(m, s, __uint_as_float(rm[1]), __uint_as_float(rs[1]));
  }
}
// the records of a wave's lanes -> every lane (every lane active; a lane without rows holds the empty record)
__device__ __forceinline__ void rules_rec_wave_reduce(RulesRec& r) {
  wave_argmax(r.tv, r.ti);
  wave_argmax(r.sv, r.si);
  lse_wave_reduce_dpp(r.mt, r.st);
  lse_wave_reduce_dpp(r.m, r.s);
}
__device__ __forceinline__ void rules_rec_store(unsigned* w, const RulesRec& r) {
  w[0] = __float_as_uint(r.tv); w[1] = (unsigned)r.ti; w[2] = __float_as_uint(r.sv); w[3] = (unsigned)r.si;
  w[4] = __float_as_uint(r.mt); w[5] = __float_as_uint(r.st); w[6] = __float_as_uint(r.m); w[7] = __float_as_uint(r.s);
}
__device__ __forceinline__ RulesRec rules_rec_load(const unsigned* w) {
  return {__uint_as_float(w[0]), (int)w[1], __uint_as_float(w[2]), (int)w[3], __uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]),
          __uint_as_float(w[7])};
}
// word k of a record (the one-instruction publish: lane k < 8 stores granule k)
__device__ __forceinline__ unsigned rules_rec_word(const RulesRec& r, int k) {
  const unsigned a = k == 0 ? __float_as_uint(r.tv) : k == 1 ? (unsigned)r.ti : k == 2 ? __float_as_uint(r.sv) : (unsigned)r.si;
  const unsigned b = k == 4 ? __float_as_uint(r.mt) : k == 5 ? __float_as_uint(r.st) : k == 6 ? __float_as_uint(r.m) : __float_as_uint(r.s);
  return k < 4 ? a : b;
}

// The workgroup's record from its waves' records in LDS, by ONE wave (all 64 lanes): lane l < NCW takes the compute waves' record l,
// lane NCW + l the poller waves' record l when the pollers held rows (with_pollers), every other lane the empty record; then the
// wave butterfly. Result in every lane.
__device__ __forceinline__ RulesRec rules_rec_fold(const unsigned* rec_c, const unsigned* rec_p, bool with_pollers, int lane) {
  RulesRec r = rules_rec_empty();
  if (lane < NCW) r = rules_rec_load(rec_c + lane * kRecWords);
  else if (lane < NCW + NPW && with_pollers) r = rules_rec_load(rec_p + (lane - NCW) * kRecWords);
  rules_rec_wave_reduce(r);
  return r;
}

// The grid's record from the eight wave results of the gather (rec_g): waves 0-3 hold (tv, ti, sv, si) of their 64 workgroups, waves
// 4-7 (mt, st, m, s); merged in wave order.
__device__ __forceinline__ RulesRec rules_rec_grid(const unsigned* rec_g) {
  RulesRec r{__uint_as_float(rec_g[0]), (int)rec_g[1], __uint_as_float(rec_g[2]), (int)rec_g[3],
             __uint_as_float(rec_g[16]), __uint_as_float(rec_g[17]), __uint_as_float(rec_g[18]), __uint_as_float(rec_g[19])};
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    argmax_take(r.tv, r.ti, __uint_as_float(rec_g[4 * w]), (int)rec_g[4 * w + 1]);
    argmax_take(r.sv, r.si, __uint_as_float(rec_g[4 * w + 2]), (int)rec_g[4 * w + 3]);
    lse_merge(r.mt, r.st, __uint_as_float(rec_g[16 + 4 * w]), __uint_as_float(rec_g[16 + 4 * w + 1]));
    lse_merge(r.m, r.s, __uint_as_float(rec_g[16 + 4 * w + 2]), __uint_as_float(rec_g[16 + 4 * w + 3]));
  }
  return r;
}

// The decision of a step from the grid's record (rules_body's, decode_timestamps.hip): the id, its logit and, over the final
// allowed set, its log-probability
struct RulesDecision {
  int id;
  float value, logprob;
};
__device__ __forceinline__ RulesDecision rules_decide(RulesRec r, int E) {
  const bool rule5 = rule5_fires(r.m, r.s, r.tv);
  RulesDecision d{E, -INFINITY, 0.f};
  const Pick pick = final_pick(rule5, r.tv, r.sv);
  if (pick == Pick::kText) { d.id = r.ti; d.value = r.tv; }
  if (pick == Pick::kTimestamp) { d.id = r.si; d.value = r.sv; }
  final_set_merge(rule5, r.m, r.s, r.mt, r.st);
  d.logprob = logprob_of(d.value, r.m, r.s);
  return d;
}

// The history's four values (allowed_sets_from_state) after one more id
struct RulesState {
  int last_ts;  // id of the history's last timestamp, -1: none
  bool last_is_ts, penult_is_ts;
};
__device__ __forceinline__ void rules_state_push(RulesState& h, int id, int T) {
  h.penult_is_ts = h.last_is_ts;
  h.last_is_ts = id >= T;
  if (id >= T) h.last_ts = id;
}

}  // inline namespace AXW_NS
}  // namespace axw
