// decode_beam_candidates.hpp — the sorted lists of beam_candidates_kernel (DESIGN.md "Beam search"), shared by the kernel's two
// instantiations of beam_candidates_body.inc: decode_beam.hip's, which is the kernel it always was, and decode_beam_rep.hip's under
// the repetition rules (DESIGN.md "Repetition rules").
#pragma once
#include "decode_rules.hpp"

namespace axw {
inline namespace AXW_NS {
namespace beam_cand {


constexpr int kM = kBeamMaxCand;  // list length: every M <= 9 is served by the same fully unrolled lists
constexpr int kNoId = 0x7fffffff;

// A thread's sorted top-kM list: value descending, and among equal values the id that came first (a thread meets its ids in
// ascending order, so that is the lower id). Static indices only: the arrays live in registers.
struct TopList {
  float v[kM];
  int i[kM];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < kM; ++j) { v[j] = -INFINITY; i[j] = kNoId; }
  }
  // NaN and -inf never enter (neither compares greater than the -inf the list starts with)
  __device__ __forceinline__ void push(float x, int id) {
    if (!(x > v[kM - 1])) return;
    v[kM - 1] = x; i[kM - 1] = id;
#pragma unroll
    for (int j = kM - 1; j > 0; --j) {
      const bool up = v[j] > v[j - 1];  // strict: never past an equal value that came earlier
      const float tv = v[j - 1];
      const int ti = i[j - 1];
      v[j - 1] = up ? v[j] : tv; i[j - 1] = up ? i[j] : ti;
      v[j] = up ? tv : v[j];     i[j] = up ? ti : i[j];
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j < kM - 1; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
    v[kM - 1] = -INFINITY; i[kM - 1] = kNoId;
  }
};

// the wave's M best (value descending, lowest id on ties) -> out_v / out_i [M] in LDS, by M rounds of wave_argmax over the heads
__device__ __forceinline__ void wave_top(TopList& l, int M, float* out_v, int* out_i, int lane) {
  for (int r = 0; r < M; ++r) {
    float bv = l.v[0];
    int bi = l.i[0];
    wave_argmax(bv, bi);
    if (bi != kNoId && bi == l.i[0]) l.pop();  // ids are unique over the wave: exactly one lane owns the winner
    if (lane == 0) { out_v[r] = bv; out_i[r] = bi; }
  }
}

}  // namespace beam_cand
}  // inline namespace AXW_NS
}  // namespace axw
