// decode_attention_common.hpp — what the single-query attention kernels share around their own key-block loops:
// decode_attention_kernel (decoder.hip) and decode_cross_attention_group_kernel (decode_attention_group.hip). The folded query value,
// the fused query projection of the one-row kernel, the merge of the four waves' records, the split hand-off and the output pair.
// The functions take values and pointers, never a parameter struct, so that a kernel which re-reads its parameters from the
// kernel-argument segment can pass what it read. decode_cross_attention_fp8_kernel (cross_kv_fp8.hip) does that, but still carries
// its own text of these pieces (common.hpp, DecAttnFp8Params, says why): a change to the hand-off is made here AND there.
#pragma once
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {
namespace attn {

using layout::kPartStride;
using layout::kAttnSplitMax;
using layout::kPartM;
using layout::kPartL;
using layout::kPartO;

// ------------------------------------------------------------------------------- folded query (QM 2)
// decode_gemm.hip "QUERY FOLD": the head's query value of one dimension is r (T - mu s) + c, from the row's T (written by the o
// launch), two constant vectors and the row's d / 16 block statistics. One wave per (row, head): lane = dimension, and the lanes below
// nst = d / 16 hold one block statistic {sum, centred squares} each.
struct FoldedQueryRegs { float tq, sj, cj; f32x2_t sp; };
__device__ __forceinline__ FoldedQueryRegs folded_query_request(const float* tq, const float* stat_part, const float* fold_s, const float* fold_c,
                                                                long row, int head, int lane, int d, int nst) {
  FoldedQueryRegs r{tq[row * d + head * 64 + lane], fold_s[head * 64 + lane], fold_c[head * 64 + lane], {0.f, 0.f}};
  if (lane < nst) r.sp = *reinterpret_cast<const f32x2_t*>(stat_part + (row * nst + lane) * 2);
  return r;
}
// Chan et al.: the row's mean from the block sums, its centred squares from the blocks' own + 16 (block mean - mean)^2
__device__ __forceinline__ float folded_query_value(const FoldedQueryRegs& r, int lane, int d, int nst) {
  const float mean = wave_sum(r.sp[0]) / (float)d;
  const float dm = r.sp[0] * (1.f / 16.f) - mean;
  const float m2 = wave_sum(lane < nst ? r.sp[1] + 16.f * dm * dm : 0.f);
  const float rstd = rsqrtf(m2 / (float)d + 1e-5f);
  return rstd * (r.tq - mean * r.sj) + r.cj;
}

// ------------------------------------------------------------------------------- fused query projection (QM 1), one row per workgroup
// q = Wq[head * 64 .. + 64][:] . LayerNorm(x[b]) + bq by the 256 threads of the (clip, head) workgroup (fp32 FMA on h16 weights,
// export_onnx.py:221-230): 4 lanes share a weight row, lane j takes the 16-byte chunks j, j + 4, ...
// NCHL > 0 (d_model = 32 NCHL: 384 / 512 / 768 / 1024): the lane's NCHL weight chunks are ALL requested up front, unconditionally — one
// memory round trip and straight-line code instead of one round trip per 8 chunks behind per-chunk bounds checks (which hipcc turns
// into a branch per load). NCHL == 0: any d_model <= 1024 that is a multiple of 32, 8 chunks per pass.
// Two steps, so that a kernel can put its workgroup-uniform "this clip is done" return between the requests and the first barrier.
template <int NCHL>
struct FusedQueryRegs {
  static constexpr int NWC = NCHL > 0 ? NCHL : 8;
  float xv[4], gg[4], bb[4];
  u32x4 wc[NWC];
  float bq;
  const h16* wr;  // this lane's weight row
};
template <int NCHL>
__device__ __forceinline__ FusedQueryRegs<NCHL> fused_query_request(const float* x, const float* ln_w, const float* ln_b, const h16* wq,
                                                                    const float* bq, int b, int head, int d, int tid) {
  FusedQueryRegs<NCHL> r;
  const float* xr = x + (long)b * d;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = tid + 256 * e;
    r.xv[e] = c < d ? xr[c] : 0.f;
    r.gg[e] = c < d ? ln_w[c] : 0.f;
    r.bb[e] = c < d ? ln_b[c] : 0.f;
  }
  // the first weight chunks of this lane's row
  const int qrow = tid >> 2, qj = tid & 3;
  r.wr = wq + (long)(head * 64 + qrow) * d;
  const int nch = d >> 3;  // 16-byte chunks per row
#pragma unroll
  for (int i = 0; i < r.NWC; ++i) {
    const int c = qj + 4 * i;
    if constexpr (NCHL > 0) r.wc[i] = *reinterpret_cast<const u32x4*>(r.wr + c * 8);
    else r.wc[i] = c < nch ? *reinterpret_cast<const u32x4*>(r.wr + c * 8) : u32x4{0u, 0u, 0u, 0u};
  }
  r.bq = bq[head * 64 + qrow];
  return r;
}
// Returns query value tid / 4 (in every lane of its quad). s_act: 1024 floats (16-byte aligned), s_red: 8 floats of LDS; two barriers.
// `projected` runs between the LayerNormed row's barrier and the weight arithmetic (measurement builds stamp the time there).
template <int NCHL, class F>
__device__ __forceinline__ float fused_query_finish(FusedQueryRegs<NCHL>& r, float* s_act, float* s_red, int d, int tid, int lane, int wave,
                                                    F&& projected) {
  const float* xv = r.xv;
  // statistics in one pass behind one barrier (as in the clip-block GEMM prologue: decode_gemm.hip): var = E[x^2] - mean^2
  float s1 = (xv[0] + xv[1]) + (xv[2] + xv[3]);
  float s2 = (xv[0] * xv[0] + xv[1] * xv[1]) + (xv[2] * xv[2] + xv[3] * xv[3]);  // (elements beyond d were loaded as 0)
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) { s_red[wave] = s1; s_red[4 + wave] = s2; }
  __syncthreads();
  const float mean = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / d;
  const float rstd = rsqrtf(fmaxf(((s_red[4] + s_red[5]) + (s_red[6] + s_red[7])) / d - mean * mean, 0.f) + 1e-5f);
#pragma unroll
  for (int e = 0; e < 4; ++e) { const int c = tid + 256 * e; if (c < d) s_act[c] = (xv[e] - mean) * rstd * r.gg[e] + r.bb[e]; }
  __syncthreads();
  projected();
  const int qj = tid & 3, nch = d >> 3;
  float a0 = 0.f, a1 = 0.f;
  if constexpr (NCHL > 0) {
    float b0 = 0.f, b1 = 0.f;  // four independent chains
#pragma unroll
    for (int i = 0; i < NCHL; ++i) {
      const int c = qj + 4 * i;
      const float4 y0 = *reinterpret_cast<const float4*>(s_act + c * 8), y1 = *reinterpret_cast<const float4*>(s_act + c * 8 + 4);
      a0 = fmaf(h16lo(r.wc[i][0]), y0.x, a0);
      a1 = fmaf(h16hi(r.wc[i][0]), y0.y, a1);
      b0 = fmaf(h16lo(r.wc[i][1]), y0.z, b0);
      b1 = fmaf(h16hi(r.wc[i][1]), y0.w, b1);
      a0 = fmaf(h16lo(r.wc[i][2]), y1.x, a0);
      a1 = fmaf(h16hi(r.wc[i][2]), y1.y, a1);
      b0 = fmaf(h16lo(r.wc[i][3]), y1.z, b0);
      b1 = fmaf(h16hi(r.wc[i][3]), y1.w, b1);
    }
    a0 += b0; a1 += b1;
  }
  for (int c0 = 0; c0 < nch && NCHL == 0; c0 += 32) {  // 8 chunks of this lane per pass
    u32x4 cur[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) cur[i] = r.wc[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int c = c0 + 32 + qj + 4 * i; r.wc[i] = c < nch ? *reinterpret_cast<const u32x4*>(r.wr + c * 8) : u32x4{0u, 0u, 0u, 0u}; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = c0 + qj + 4 * i;
      if (c < nch) {
        const float4 y0 = *reinterpret_cast<const float4*>(s_act + c * 8), y1 = *reinterpret_cast<const float4*>(s_act + c * 8 + 4);
        a0 = fmaf(h16lo(cur[i][0]), y0.x, a0);
        a1 = fmaf(h16hi(cur[i][0]), y0.y, a1);
        a0 = fmaf(h16lo(cur[i][1]), y0.z, a0);
        a1 = fmaf(h16hi(cur[i][1]), y0.w, a1);
        a0 = fmaf(h16lo(cur[i][2]), y1.x, a0);
        a1 = fmaf(h16hi(cur[i][2]), y1.y, a1);
        a0 = fmaf(h16lo(cur[i][3]), y1.z, a0);
        a1 = fmaf(h16hi(cur[i][3]), y1.w, a1);
      }
    }
  }
  float acc = a0 + a1;
  acc += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
  acc += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x4E, 0xf, 0xf, true));  // quad_perm [2,3,0,1]
  return acc + r.bq;
}

// ------------------------------------------------------------------------------- the four waves' records -> one
// r: wave 0's record (m, l, o[64]) in LDS, the other waves' `stride` floats apart; dim: the output dimension this thread merges
__device__ __forceinline__ void merge_wave_records(const float* r, int stride, int dim, float& m, float& l, float& ov) {
  m = fmaxf(fmaxf(r[kPartM], r[stride + kPartM]), fmaxf(r[2 * stride + kPartM], r[3 * stride + kPartM]));
  l = 0.f; ov = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __expf(r[w * stride + kPartM] - m);
      l += f * r[w * stride + kPartL];
      ov += f * r[w * stride + kPartO + dim];
    }
  }
}

// ------------------------------------------------------------------------------- split hand-off
// Splits of one (clip, head) in the batched path at FEW clips (3 clips x 12 heads are 36 workgroups for 256 CUs, each streaming its
// 24 key blocks one after the other). Every split publishes (m, l, o[64]) with write-through stores, drains them, and draws a
// ticket; whoever draws the last one folds all of them IN SPLIT ORDER (the result does not depend on who arrives last) and writes
// the output.
// The hand-off is the first row of MI355X_MICROARCH.md's table of hand-offs that need no acquire: every payload store is sc1
// (write-through), the storing wave drains vmcnt, ONE lane adds to an agent-scope counter, and the workgroup whose add came last —
// told by the value its add returned — reads the others' records with sc1 loads after that add has returned (the loads sit behind
// a branch on the returned value; the signal fences pin the compiler's ordering on both sides). An acq_rel RMW instead
// (buffer_wbl2 + buffer_inv per workgroup, what the C++ memory model would ask for) was measured at turbo dims, 16 clips, 2 splits:
// decode 151.5 -> 197.0 ms (round 3).
// The last arriver also stores 0 to the counter, for the next launch.
//
// One wave (lane = dim) publishes a record `mine` and waits until the stores have left its store queue.
__device__ __forceinline__ void publish_split_record(float* mine, int dim, float m, float l, float ov) {
  __hip_atomic_store(mine + kPartO + dim, ov, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (dim == 0) {
    __hip_atomic_store(mine + kPartM, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + kPartL, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ __forceinline__ void drain_split_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// The thread for which `drawer` holds draws the ticket (every other thread gets 0). The one-row kernels draw inside the wave that
// published and broadcast with readfirstlane; the group kernel, whose four waves all publish, draws behind a barrier and hands the
// ticket round through LDS.
__device__ __forceinline__ unsigned draw_split_ticket(unsigned* cnt, bool drawer) {
  unsigned ticket = 0;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if (drawer) ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  return ticket;
}
__device__ __forceinline__ void reset_split_counter(unsigned* cnt) { __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The last arriver's fold of dimension `dim`: base = record of split 0, (m, l, ov) = this split's own record. Every other split's
// record is requested before the first one is used: ONE memory round trip for the fold, not one per split (five dependent sc1 round
// trips at six splits were a quarter of the launch at four clips). Returns O / L.
__device__ __forceinline__ float fold_split_records(const float* base, int split, int n_split, int dim, float m, float l, float ov) {
  float ms[kAttnSplitMax], ls[kAttnSplitMax], os[kAttnSplitMax];
#pragma unroll
  for (int s2 = 0; s2 < kAttnSplitMax; ++s2) {
    ms[s2] = m; ls[s2] = l; os[s2] = ov;
    if (s2 < n_split && s2 != split) {
      const float* other = base + s2 * kPartStride;
      ms[s2] = __hip_atomic_load(other + kPartM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ls[s2] = __hip_atomic_load(other + kPartL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      os[s2] = __hip_atomic_load(other + kPartO + dim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  float M = -INFINITY, Ls = 0.f, O = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < kAttnSplitMax; ++s2) {
    if (s2 < n_split) {
      const float m2 = ms[s2], l2 = ls[s2], o2 = os[s2];
      const float mn = fmaxf(M, m2);
      const float f1 = M > -INFINITY ? __expf(M - mn) : 0.f, f2 = m2 > -INFINITY ? __expf(m2 - mn) : 0.f;
      Ls = fmaf(f1, Ls, f2 * l2);  // (spelled out: which of the two products is fused must not depend on the caller)
      O = fmaf(f1, O, f2 * o2);
      M = mn;
    }
  }
  return O / Ls;
}
// The one-row kernels' whole hand-off, called by the wave (lane = dim) that holds the workgroup's merged record: false = another
// split draws the last ticket and writes the output; true = y is the output value of `dim`. `at(k)`: measurement builds stamp the
// time at points 6 (records drained), 7 (ticket drawn) and 8 (folded).
template <class F>
__device__ __forceinline__ bool split_publish_and_fold(float* base, unsigned* cnt, int split, int n_split, int dim, float m, float l, float ov,
                                                       float& y, F&& at) {
  publish_split_record(base + split * kPartStride, dim, m, l, ov);
  drain_split_stores();
  at(6);
  const unsigned ticket = __builtin_amdgcn_readfirstlane(draw_split_ticket(cnt, dim == 0));
  at(7);
  if (ticket != (unsigned)n_split - 1u) return false;  // (the whole wave; the other waves are past their last use of LDS)
  y = fold_split_records(base, split, n_split, dim, m, l, ov);
  at(8);
  if (dim == 0) reset_split_counter(cnt);
  return true;
}

// ------------------------------------------------------------------------------- output
// y as element (row, k) of a fragment-major (hi, lo) h16 pair
__device__ __forceinline__ void store_out_pair(h16* out_hi, h16* out_lo, int row, int k, int nbs, float y) {
  const h16 yh = (h16)y;
  const long i = layout::frag_index(row, k, nbs);
  out_hi[i] = yh;
  out_lo[i] = (h16)(y - (float)yh);
}

}  // namespace attn
}  // inline namespace AXW_NS
}  // namespace axw
