// decode_persistent_common.hpp — what the persistent decode launches share (decode_persistent.hip: one clip per launch;
// decode_persistent2.hip: two or three clips per launch): lane-group reductions, {tag, value} granules and their polls,
// weight-row sets with the one-instruction publish, the 64-key attention block, the partial merge, the kernels' common
// prologue, and the host side's LDS size, shape table and launch.
#pragma once
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gptr_t;

constexpr int PT = 1024;           // threads per workgroup, one workgroup per CU
constexpr int NPW = 8, NCW = 8;    // poller waves, compute waves
constexpr int PL = NPW * 64;       // poller lanes
constexpr int CT = NCW * 64;       // compute threads
// A lane gives up on a hand-off by TIME: a real wait is microseconds, so the first kSpinFree polls (about a
// millisecond) never read the clock; after that the 100 MHz wall clock is sampled every 256 polls and the lane gives up
// kSpinTicks later (50 ms). A launch whose workgroups cannot all be resident (CUs taken by another process, a CU-masked
// stream, a partitioned device) therefore costs a request ~50 ms, not a second, before the engine falls back.
// Cache policy of the three streams of a decoder step (Whisper-small: 198 MB of layer weights, 80 MB of vocabulary
// rows, 55 MB of cross K/V against 256 MB of Infinity Cache + 32 MB of L2). The layer weights are the latency-critical
// loads (requested one hand-off ahead of their use) and are re-read every step: default policy, so that they are served
// from the Infinity Cache. The vocabulary rows are a once-per-step bandwidth-bound stream and the cross K/V tiles are
// requested a whole layer ahead: both non-temporal, so that they do not evict the layer weights. Measured (decode of
// one clip, A/B/A/B inside one GPU call): on one box all-default 121.0 / vocabulary nt 118.1 / both 118.1 ms, on
// another all-default 121.2 / vocabulary nt 121.2 / cross K/V nt 118.9 / both 119.1 ms — which of the two streams
// matters differs between boxes (allocation placement), both together are within 0.3 ms of the better everywhere.
// Every weight row nt: 129.1 ms (the layer weights do live in the cache between steps).
#ifndef AXW_VOCAB_NT
#define AXW_VOCAB_NT 1
#endif
#ifndef AXW_KV_NT_LDS
#define AXW_KV_NT_LDS 1
#endif
// The 64-key attention block's two products on the matrix pipe (1, attn_block below) or as v_dot2c / FMA dot products on the
// vector pipe (0, the form of rounds 5-7, kept for the A/B: profiles/attn_matrix_pipe_ab.txt)
#ifndef AXW_ATTN_MFMA
#define AXW_ATTN_MFMA 1
#endif
// The cross V tile in LDS with the 16-byte chunks of its rows permuted (1, layout::cross_v_swizzle: the transposed reads of the
// matrix-pipe block are then free of bank conflicts) or plain row-major as in HBM (0, the form of round 8, kept for the A/B:
// profiles/cross_segment_ab.txt)
#ifndef AXW_CROSS_V_SWIZZLE
#define AXW_CROSS_V_SWIZZLE 1
#endif
// The one-clip launch's merge of the cross-attention records: in registers by the lanes that gathered them, one workgroup barrier
// (1; only with the query fold, see decode_persistent.hip), or through LDS behind a barrier of its own (0, the form of rounds 5-8,
// which the multi-clip launch and the unfolded one-clip launch keep)
#ifndef AXW_CO_MERGE_IN_GATHER
#define AXW_CO_MERGE_IN_GATHER 1
#endif
constexpr bool kVocabNT = AXW_VOCAB_NT != 0;
constexpr bool kAttnMfma = AXW_ATTN_MFMA != 0;
constexpr bool kCrossVSwizzle = AXW_CROSS_V_SWIZZLE != 0;
constexpr bool kCoMergeInGather = AXW_CO_MERGE_IN_GATHER != 0;
constexpr int kKvAux = AXW_KV_NT_LDS ? 2 : 0;  // aux bits of global_load_lds: 2 = nt
constexpr int kSpinFree = 1024;
constexpr long long kSpinTicks = 5000000;
constexpr int kPS = layout::kPartStride;  // attention partial record in LDS: m, l, o[64]
constexpr int kCrossKeysPad = 24 * layout::kKvBlockKeys;  // allocated cross-attention keys per head: 1500 padded to 24 blocks
constexpr int kRec = 80;           // cross-attention partial record as granules: o[64] (four full lines), m, l; 5-line stride
constexpr int kCrossSplit = 3;     // cross-attention key ranges per head (8 blocks of 64 keys each = 8 compute waves)
constexpr int kKvBytes = 2 * NCW * 8192;  // LDS K/V region: K [8 blk][8][64][8] h16 + V [512 keys][64] h16

// ---------------------------------------------------------------------------------------- lane-group reductions
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum over aligned groups of LPR lanes (16, 32 or 64), result in every lane of the group; every lane of the wave
// must be active. DPP butterflies inside a 16-lane row, v_permlane{16,32}_swap across rows.
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  if constexpr (LPR >= 32) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  if constexpr (LPR >= 64) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  return v;
}
__device__ __forceinline__ float wsum(float v) { return group_sum<64>(v); }
__device__ __forceinline__ float wmax(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  return v;
}

// ---------------------------------------------------------------------------------------- granules
__device__ __forceinline__ void gput(u64* g, unsigned tag, float v) {
  __hip_atomic_store((gu64*)g, ((u64)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gput_u(u64* g, unsigned tag, unsigned v) {
  __hip_atomic_store((gu64*)g, ((u64)tag << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 gget(const u64* g) {
  return __hip_atomic_load((gu64*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned eget(const unsigned* e) {
  return __hip_atomic_load((gu32*)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pair polls: 16-byte sc1 loads of two adjacent granules (profiles/microbench/publish_shape.cpp: a hand-off gathered
// with 16-byte polls completes 0.25 us earlier than with 8-byte ones). pidx(k) = granule index of the k-th pair of this
// lane (even), < 0: none. v[2k], v[2k+1] = the two values. Returns true on give-up.
template <int NP, typename IDX>
__device__ __forceinline__ bool gather2(__amdgpu_buffer_rsrc_t rs, unsigned tag, unsigned (&v)[2 * NP], const unsigned* err, const int* ctl, IDX pidx) {
  bool ok[NP];
  int ix[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) { ix[k] = pidx(k); ok[k] = ix[k] < 0; v[2 * k] = 0u; v[2 * k + 1] = 0u; }
  long long t_start = 0;
  for (int spins = 0;; ++spins) {
    bool all = true;
    u32x4 x[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) if (!ok[k]) x[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, ix[k] * 8, 0, 16);  // aux 16 = sc1
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (!ok[k]) {
        if (x[k][1] == tag && x[k][3] == tag) { v[2 * k] = x[k][0]; v[2 * k + 1] = x[k][2]; ok[k] = true; } else all = false;
      }
    if (all) return false;
    if ((spins & 63) == 63 && *(volatile const int*)ctl) return true;  // a wave of this workgroup gave up
    if ((spins & 255) == 255 && spins >= kSpinFree) {
      if (eget(err)) return true;                                      // another workgroup gave up: leave as well
      const long long now = wall_clock64();
      if (t_start == 0) t_start = now;
      else if (now - t_start > kSpinTicks) return true;
    }
  }
}

// Lane `tid` collects granules idx(k) for k < MAXG (idx < 0: none) of epoch `tag`; returns true on give-up.
template <int MAXG, typename IDX>
__device__ __forceinline__ bool gather(const u64* buf, unsigned tag, unsigned (&v)[MAXG], const unsigned* err, const int* ctl, IDX idx) {
  bool ok[MAXG];
  int ix[MAXG];
#pragma unroll
  for (int k = 0; k < MAXG; ++k) { ix[k] = idx(k); ok[k] = ix[k] < 0; v[k] = 0u; }
  long long t_start = 0;
  for (int spins = 0;; ++spins) {
    bool all = true;
    u64 x[MAXG];
#pragma unroll
    for (int k = 0; k < MAXG; ++k) if (!ok[k]) x[k] = gget(buf + ix[k]);  // independent loads, one round trip
#pragma unroll
    for (int k = 0; k < MAXG; ++k)
      if (!ok[k]) {
        if ((unsigned)(x[k] >> 32) == tag) { v[k] = (unsigned)x[k]; ok[k] = true; } else all = false;
      }
    if (all) return false;
    if ((spins & 63) == 63 && *(volatile const int*)ctl) return true;  // a wave of this workgroup gave up
    if ((spins & 255) == 255 && spins >= kSpinFree) {
      if (eget(err)) return true;                                      // another workgroup gave up: leave as well
      const long long now = wall_clock64();
      if (t_start == 0) t_start = now;
      else if (now - t_start > kSpinTicks) return true;
    }
  }
}


// ---------------------------------------------------------------------------------------- weight rows
template <int LPR, int CH, bool NT = false>
__device__ __forceinline__ void rows_load(u32x4 (&w)[CH], const h16* W, int K, int row, int tid) {
  const int j = tid % LPR;
  const h16* wr = W + (long)row * K;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    if constexpr (NT) w[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + (j + LPR * i) * 8));
    else w[i] = *reinterpret_cast<const u32x4*>(wr + (j + LPR * i) * 8);
  }
}
#define AXW_FMA8(ACC0, ACC1, U, X0, X1)                       \
  ACC0 = fmaf(h16lo(U[0]), X0.x, ACC0);       \
  ACC1 = fmaf(h16hi(U[0]), X0.y, ACC1); \
  ACC0 = fmaf(h16lo(U[1]), X0.z, ACC0);       \
  ACC1 = fmaf(h16hi(U[1]), X0.w, ACC1); \
  ACC0 = fmaf(h16lo(U[2]), X1.x, ACC0);       \
  ACC1 = fmaf(h16hi(U[2]), X1.y, ACC1); \
  ACC0 = fmaf(h16lo(U[3]), X1.z, ACC0);       \
  ACC1 = fmaf(h16hi(U[3]), X1.w, ACC1);
// dot product of one weight row (registers) with the activation vector in LDS; LPR lanes share the row
template <int LPR, int CH>
__device__ __forceinline__ float rows_dot(const u32x4 (&w)[CH], const float* act, int tid) {
  const int j = tid % LPR;
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const float4 x0 = *reinterpret_cast<const float4*>(act + (j + LPR * i) * 8);
    const float4 x1 = *reinterpret_cast<const float4*>(act + (j + LPR * i) * 8 + 4);
    AXW_FMA8(a0, a1, w[i], x0, x1)
  }
  return group_sum<LPR>(a0 + a1);
}
template <int LPR, int CH>
__device__ __forceinline__ float rows_dot_reg(const u32x4 (&w)[CH], const float4 (&a)[CH][2]) {
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int i = 0; i < CH; ++i) { AXW_FMA8(a0, a1, w[i], a[i][0], a[i][1]) }
  return group_sum<LPR>(a0 + a1);
}

// ---------------------------------------------------------------------------------------- workgroup barrier
// s_barrier with only the LDS counter drained. HIP's __syncthreads() also drains vmcnt, which would make every
// barrier wait for the weight rows that were just requested for the NEXT phase.
__device__ __forceinline__ void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------------------- row sets
// The rows of one linear layer that this workgroup computes: slot = ctid / LPR handles row r0 + slot (+ k * slots),
// ctid = thread index among the compute waves. prefetch() issues the loads of the first pass one phase ahead.
template <int LPR, int CH>
struct RowSet {
  u32x4 w[CH];
  float bias;
  float sfac;  // run_ln only: s_j = sum_i W_ji g_i of this slot's row (the LayerNorm folded into the rows)
  int r0, r1;
  // first < 0: rows dealt evenly over all workgroups; else one full pass (SLOTS rows) per producer, producers =
  // workgroups first, first + 1, ... (the others get no rows)
  __device__ __forceinline__ void prefetch(const h16* W, const float* b, int K, int N, int wg, int P, int ctid, int first = -1) {
    if (first < 0) {
      r0 = (int)((unsigned)wg * (unsigned)N / (unsigned)P);  // wg * N < 2^31 (256 workgroups x 51866 rows)
      r1 = (int)((unsigned)(wg + 1) * (unsigned)N / (unsigned)P);
    } else {
      constexpr int SLOTS = CT / LPR;
      int pidx = wg - first;
      if (pidx < 0) pidx += P;
      r0 = pidx * SLOTS < N ? pidx * SLOTS : 0;
      r1 = pidx * SLOTS < N ? (r0 + SLOTS < N ? r0 + SLOTS : N) : 0;
    }
    const int slot = ctid / LPR, j = ctid % LPR;
    const int row = r0 + slot;
    rows_load<LPR, CH>(w, W, K, row < r1 ? row : r0, ctid);
    bias = (b && row < r1 && j == 0) ? b[row] : 0.f;
  }
  // The same for rows that carry their LayerNorm (decode_persistent.hip, round 5): bias = c_j = W beta + b, sfac = s_j = W g
  __device__ __forceinline__ void prefetch_ln(const h16* W, const float* sv, const float* cv, int K, int N, int wg, int P, int ctid, int first) {
    prefetch(W, cv, K, N, wg, P, ctid, first);
    const int slot = ctid / LPR, j = ctid % LPR, row = r0 + slot;
    sfac = (row < r1 && j == 0) ? sv[row] : 0.f;
  }
  // act holds g . x (not normalised): res = rstd (W (g . x) - mean s) + c. One pass, or two where the rows are dealt evenly.
  __device__ __forceinline__ void run_ln(const h16* W, const float* sv, const float* cv, int K, const float* act, int ctid, float (&res)[2], float mean, float rstd) {
    constexpr int SLOTS = CT / LPR;
    const int slot = ctid / LPR, j = ctid % LPR;
    res[0] = rstd * (rows_dot<LPR, CH>(w, act, ctid) - mean * sfac) + bias;
    res[1] = 0.f;
    const int row1 = r0 + slot + SLOTS;
    if (row1 < r1) {
      rows_load<LPR, CH>(w, W, K, row1, ctid);
      const float c1 = j == 0 ? cv[row1] : 0.f, s1 = j == 0 ? sv[row1] : 0.f;
      int ctid2 = ctid;
      asm volatile("" : "+v"(ctid2));
      res[1] = rstd * (rows_dot<LPR, CH>(w, act, ctid2) - mean * s1) + c1;
    }
  }
  // Computes this slot's rows (at most two passes: every supported shape has <= 2 * slots rows per workgroup) into
  // res[]. The caller requests the NEXT phase's rows before it publishes: a write-through store in front of a load
  // holds the load back for about a microsecond.
  __device__ __forceinline__ void run(const h16* W, const float* b, int K, const float* act, int ctid, float (&res)[2]) {
    constexpr int SLOTS = CT / LPR;
    const int slot = ctid / LPR, j = ctid % LPR;
    res[0] = rows_dot<LPR, CH>(w, act, ctid) + bias;
    res[1] = 0.f;
    const int row1 = r0 + slot + SLOTS;
    if (row1 < r1) {
      rows_load<LPR, CH>(w, W, K, row1, ctid);
      const float b1 = (b && j == 0) ? b[row1] : 0.f;
      int ctid2 = ctid;
      asm volatile("" : "+v"(ctid2));  // re-read the activations from LDS: keeping them live across both passes spills
      res[1] = rows_dot<LPR, CH>(w, act, ctid2) + b1;
    }
  }
  // Publishes this workgroup's rows (contiguous granules r0..r1-1 of `buf`) with ONE store instruction: the slot
  // leaders drop f(result) into pk[] (LDS), every compute wave bumps an LDS counter, and the wave that arrives last
  // stores all rows. Several waves each storing a few granules of the same 128-byte lines cost the hand-off 1.7 us
  // (profiles/microbench/publish_shape.cpp: 48 producers x 16 rows, 3.4 -> 1.75 us per phase).
  template <typename F>
  __device__ __forceinline__ void publish(int ctid, const float (&res)[2], float* pk, int* cnt, u64* buf, unsigned tag, F f) const {
    constexpr int SLOTS = CT / LPR;
    const int slot = ctid / LPR, j = ctid % LPR, lane = ctid & 63;
    if (j == 0) {
      if (r0 + slot < r1) pk[slot] = f(res[0]);
      if (r0 + slot + SLOTS < r1) pk[slot + SLOTS] = f(res[1]);
    }
    __builtin_amdgcn_wave_barrier();
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    if ((old + 1) % NCW == 0 && lane < r1 - r0) gput(buf + r0 + lane, tag, pk[lane]);
  }
};

// sum over the lanes that share (lane & 7): lane bits 3, 4, 5
__device__ __forceinline__ float sum_hi3(float v) {
  v += dpp_mov<0x128>(v);  // row_ror:8
  {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  return v;
}

// One 16-byte piece of a K/V block that lives in GLOBAL memory (the two-clip launch keeps clip 1's self-attention cache there,
// written by this workgroup's pollers with plain stores): a buffer load with sc0, so it is served by L2 and never by a line
// that L1 still holds from an earlier step. base: the block (wave-uniform), off: this lane's h16 offset inside it.
__device__ __forceinline__ u32x4 kv_global16(const h16* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 8192, 0x27000);  // one 64-key block
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off * 2, 0, 1);  // aux 1 = sc0
}
// One wave, one block of 64 keys in LDS: kblk = [8 (d/8)][64 keys][8] h16. Writes the softmax partial (m, l, o[64]) to
// part[0..66). qp: the query as packed h16 pairs, [32] hi then [32] lo (q = hi + lo). pw: 64 dwords of wave-private LDS
// scratch. lane = key for the scores and the mask, lane = dim for the output.
// Two compute waves share a SIMD and the block was VALU-bound as dot products (skipping its arithmetic altogether shortened
// the decode of one clip by 12.6 %), so both products run on the matrix pipe, which nothing else in this launch uses:
// v_mfma_f32_16x16x32 with the one-row operand (the query over dims, then the probabilities over keys) as A and the LDS tiles
// as they are as B.
//   A: lane l holds row l & 15, k = 8 (l >> 4) + j. Even rows carry the hi half of the (hi, lo) pair and odd rows the lo half
//      (attn_a_frag: one ds_read_b128 from the packed pairs, eight distinct addresses per wave), so lane group g = l >> 4 finds
//      hi . B in result register 0 and lo . B in register 1 (and the same again in 2 and 3: the rows of a product are
//      independent, a spare row costs nothing and needs neither a zero piece nor a mask).
//   B of the scores, key block kb, k-step ks (32 dims): the piece kv_chunk_offset(blk, 4 ks + l / 16, 16 kb + l % 16) of the
//      blocked K. Four accumulators, one per 16-key block; lane group g takes acc[g][0] + acc[g][1], the score of key l.
//      A masked key's K row may hold anything: it reaches its own column only, and that column is set to -inf.
//   B of the output, dim block nb, k-step ks (32 keys): from the TRANSPOSED self-attention cache (VT: vblk = [8 (key/8)][64
//      dims][8 keys], this kernel's own layout) the piece kv_chunk_offset(blk, 4 ks + l / 16, 16 nb + l % 16); from a row-major
//      cross tile [64 keys][64 dims] (LDS-DMA in the HBM layout) two ds_read_b64_tr_b16 of keys 32 ks + 8 (l / 16) + {0..3},
//      {4..7}, dims 16 nb .. + 15. Lane group g takes oc[g][0] + oc[g][1] = o[l].
// The transposed reads and the MFMAs need EXEC all ones: every call site is wave-uniform (cw < nblk, a unit's waves).
// LDS banks of the transposed reads on 128-byte V rows ((a / 4) % 64 per 32-lane half): in the plain row-major image rows q and
// q + 2 of a 4-row block and the two blocks of a half (8 rows = 1 KiB apart) fall on the same eight banks, so a read is 4-way: 8
// LDS cycles instead of 2, 16 reads per block. The cross tiles therefore live in LDS with the chunks of every row permuted
// (attn_block<false, true>, layout::cross_v_swizzle; stage_cross_kv applies the map on the SOURCE side of the tile's DMA): every
// read is conflict-free, 32 LDS cycles per block instead of 128. The plain image stays for the A/B and the block's own tests.
__device__ __forceinline__ h16x8 attn_a_frag(const unsigned* xp, int ks, int lane) {
  return __builtin_bit_cast(h16x8, *reinterpret_cast<const u32x4*>(xp + 32 * (lane & 1) + 16 * ks + 4 * (lane >> 4)));
}
// lane group g = lane / 16 takes (hi + lo) of accumulator g
__device__ __forceinline__ float attn_pick(const f32x4 (&acc)[4], int lane) {
  const float s0 = acc[0][0] + acc[0][1], s1 = acc[1][0] + acc[1][1], s2 = acc[2][0] + acc[2][1], s3 = acc[3][0] + acc[3][1];
  const int g = lane >> 4;
  return g == 0 ? s0 : g == 1 ? s1 : g == 2 ? s2 : s3;
}
// this lane's h16 offset of B piece (blk kb or nb, k-step ks) in a blocked K or transposed V block
__device__ __forceinline__ int attn_b_offset(int nb, int ks, int lane) { return layout::kv_chunk_offset(0, 4 * ks + (lane >> 4), 16 * nb + (lane & 15)); }
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
// B piece (nb, ks) of a row-major V tile, plain or swizzled: two transposed reads (every lane of the wave active). base: the lane's
// layout::cross_v_read_base of the same image.
template <bool SWZ>
__device__ __forceinline__ h16x8 attn_b_rowmajor(const h16* vblk, int base, int nb, int ks) {
  struct { s16x4 lo, hi; } r;
  r.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(vblk + layout::cross_v_read_offset(base, nb, ks, 0, SWZ)));
  r.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(vblk + layout::cross_v_read_offset(base, nb, ks, 1, SWZ)));
  return __builtin_bit_cast(h16x8, r);
}
// scale, mask and softmax partial of the block (lane = key): returns the probability, m and l in every lane
__device__ __forceinline__ float attn_softmax(float s, bool valid, float* m_out, float* l_out) {
  s *= 0.125f;  // (64^-0.25)^2, export_onnx.py:116,124-126
  if (!valid) s = -INFINITY;
  const float m = wmax(s);  // -inf only for a block without a single valid key
  const float pk = m > -INFINITY ? __expf(s - m) : 0.f;
  *m_out = m;
  *l_out = wsum(pk);
  return pk;
}
// probabilities as packed (hi, lo) h16 in wave-private LDS: key k -> half-word k of ph (dwords 0..31) / pl (32..63)
__device__ __forceinline__ void attn_put_p(float pk, float* pw, int lane) {
  const h16 ph = (h16)pk, pl = (h16)(pk - (float)ph);
  reinterpret_cast<h16*>(pw)[lane] = ph;
  reinterpret_cast<h16*>(pw + 32)[lane] = pl;
  __builtin_amdgcn_wave_barrier();
}
// VT: the transposed V (true) or a row-major tile (false), which is plain unless SWZ
#if AXW_ATTN_MFMA
template <bool VT, bool SWZ = false>
__device__ __forceinline__ void attn_block(const h16* kblk, const h16* vblk, const unsigned* qp, bool valid, float* pw, float* part, int lane) {
#ifdef AXW_ATTN_SKIP  // timing-only build (wrong results): bounds what any speed-up of this block's arithmetic can buy
  if (lane == 0) { part[0] = 0.f; part[1] = 1.f; }
  part[2 + lane] = 0.f;
  return;
#endif
  f32x4 acc[4];
  {
    const h16x8 a0 = attn_a_frag(qp, 0, lane), a1 = attn_a_frag(qp, 1, lane);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const h16x8 b0 = *reinterpret_cast<const h16x8*>(kblk + attn_b_offset(kb, 0, lane)), b1 = *reinterpret_cast<const h16x8*>(kblk + attn_b_offset(kb, 1, lane));
      acc[kb] = AXW_MFMA_16x16x32(a0, b0, (f32x4{0.f, 0.f, 0.f, 0.f}));
      acc[kb] = AXW_MFMA_16x16x32(a1, b1, acc[kb]);
      if (kb == 1) __builtin_amdgcn_sched_barrier(0);  // two 16-key blocks' operands in flight at a time: the row producers hold weight rows here
    }
  }
  float m, lsum;
  const float pk = attn_softmax(attn_pick(acc, lane), valid, &m, &lsum);
  attn_put_p(pk, pw, lane);
  const unsigned* pwu = reinterpret_cast<const unsigned*>(pw);
  const h16x8 a0 = attn_a_frag(pwu, 0, lane), a1 = attn_a_frag(pwu, 1, lane);
  const int vbase = VT ? 0 : layout::cross_v_read_base(lane, SWZ);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    h16x8 b0, b1;
    if constexpr (VT) {
      b0 = *reinterpret_cast<const h16x8*>(vblk + attn_b_offset(nb, 0, lane));
      b1 = *reinterpret_cast<const h16x8*>(vblk + attn_b_offset(nb, 1, lane));
    } else {
      b0 = attn_b_rowmajor<SWZ>(vblk, vbase, nb, 0);
      b1 = attn_b_rowmajor<SWZ>(vblk, vbase, nb, 1);
    }
    acc[nb] = AXW_MFMA_16x16x32(a0, b0, (f32x4{0.f, 0.f, 0.f, 0.f}));
    acc[nb] = AXW_MFMA_16x16x32(a1, b1, acc[nb]);
    if (nb == 1) __builtin_amdgcn_sched_barrier(0);
  }
  if (lane == 0) { part[0] = m; part[1] = lsum; }
  part[2 + lane] = attn_pick(acc, lane);
}

// attn_block<true> on a block whose 16 pieces are already in registers, in the order the products consume them (kr[2 kb + ks],
// vr[2 nb + ks]: the pieces attn_b_offset(kb or nb, ks, lane) of the blocked K / the transposed V): the same operations in the
// same order, so a block gives the same bits from either home.
__device__ __forceinline__ int attn_regs_piece(int i, int lane) { return attn_b_offset(i >> 1, i & 1, lane); }
__device__ __forceinline__ void attn_block_regs(const u32x4 (&kr)[8], const u32x4 (&vr)[8], const unsigned* qp, bool valid, float* pw, float* part, int lane) {
  f32x4 acc[4];
  {
    const h16x8 a0 = attn_a_frag(qp, 0, lane), a1 = attn_a_frag(qp, 1, lane);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      acc[kb] = AXW_MFMA_16x16x32(a0, __builtin_bit_cast(h16x8, kr[2 * kb]), (f32x4{0.f, 0.f, 0.f, 0.f}));
      acc[kb] = AXW_MFMA_16x16x32(a1, __builtin_bit_cast(h16x8, kr[2 * kb + 1]), acc[kb]);
    }
  }
  float m, lsum;
  const float pk = attn_softmax(attn_pick(acc, lane), valid, &m, &lsum);
  attn_put_p(pk, pw, lane);
  const unsigned* pwu = reinterpret_cast<const unsigned*>(pw);
  const h16x8 a0 = attn_a_frag(pwu, 0, lane), a1 = attn_a_frag(pwu, 1, lane);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    acc[nb] = AXW_MFMA_16x16x32(a0, __builtin_bit_cast(h16x8, vr[2 * nb]), (f32x4{0.f, 0.f, 0.f, 0.f}));
    acc[nb] = AXW_MFMA_16x16x32(a1, __builtin_bit_cast(h16x8, vr[2 * nb + 1]), acc[nb]);
  }
  if (lane == 0) { part[0] = m; part[1] = lsum; }
  part[2 + lane] = attn_pick(acc, lane);
}
#else  // AXW_ATTN_MFMA == 0: the vector-pipe form
// The block as dot products on the vector pipe, written for instruction count: the scores are v_dot2c dot products of the
// packed K dwords with the packed query (2 instructions per 2 dims instead of 4); with the transposed V, lane = dim accumulates
// o[dim] with dot2 over key pairs against the packed probabilities; a row-major cross tile keeps the lane = (key row, dim chunk)
// form and sums over lane bits 3-5.
template <bool VT, bool SWZ = false>
__device__ __forceinline__ void attn_block(const h16* kblk, const h16* vblk, const unsigned* qp, bool valid, float* pw, float* part, int lane) {
#ifdef AXW_ATTN_SKIP  // timing-only build (wrong results): bounds what any speed-up of this block's arithmetic can buy
  if (lane == 0) { part[0] = 0.f; part[1] = 1.f; }
  if (lane < 8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) part[2 + lane * 8 + e] = 0.f;
  }
  return;
#endif
  float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int i = 0; i < 8; ++i) {
    const u32x4 kq = *reinterpret_cast<const u32x4*>(kblk + layout::kv_chunk_offset(0, i, lane));
    const u32x4 qh = *reinterpret_cast<const u32x4*>(qp + i * 4), ql = *reinterpret_cast<const u32x4*>(qp + 32 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[e] = h16dot2(kq[e], qh[e], sc[e]);
      sc[e] = h16dot2(kq[e], ql[e], sc[e]);
    }
  }
  float s = ((sc[0] + sc[1]) + (sc[2] + sc[3])) * 0.125f;  // (64^-0.25)^2, export_onnx.py:116,124-126
  if (!valid) s = -INFINITY;
  const float m = wmax(s);  // -inf only for a block without a single valid key
  const float pk = m > -INFINITY ? __expf(s - m) : 0.f;
  const float lsum = wsum(pk);
  if constexpr (VT) {
    // probabilities as packed (hi, lo) h16 in wave-private LDS: key k -> half-word k of ph (dwords 0..31) / pl (32..63)
    const h16 ph = (h16)pk, pl = (h16)(pk - (float)ph);
    reinterpret_cast<h16*>(pw)[lane] = ph;
    reinterpret_cast<h16*>(pw + 32)[lane] = pl;
    __builtin_amdgcn_wave_barrier();
    float o0 = 0.f, o1 = 0.f;
    const unsigned* pwu = reinterpret_cast<const unsigned*>(pw);
#pragma unroll 2
    for (int i = 0; i < 8; ++i) {  // keys 8i..8i+7 of dim `lane`
      const u32x4 vv = *reinterpret_cast<const u32x4*>(vblk + layout::kv_chunk_offset(0, i, lane));
      const u32x4 h4 = *reinterpret_cast<const u32x4*>(pwu + i * 4), l4 = *reinterpret_cast<const u32x4*>(pwu + 32 + i * 4);
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        o0 = h16dot2(vv[e], h4[e], o0);
        o0 = h16dot2(vv[e], l4[e], o0);
        o1 = h16dot2(vv[e + 1], h4[e + 1], o1);
        o1 = h16dot2(vv[e + 1], l4[e + 1], o1);
      }
    }
    if (lane == 0) { part[0] = m; part[1] = lsum; }
    part[2 + lane] = o0 + o1;
  } else {
    pw[(lane & 7) * 8 + (lane >> 3)] = pk;  // key k = 8i + r -> pw[r*8 + i]
    __builtin_amdgcn_wave_barrier();
    const float4 p0 = *reinterpret_cast<const float4*>(pw + (lane >> 3) * 8), p1 = *reinterpret_cast<const float4*>(pw + (lane >> 3) * 8 + 4);
    const float pr[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // V row of key 8i + (lane>>3), dims (lane&7)*8 .. +8
      const u32x4 vv = *reinterpret_cast<const u32x4*>(vblk + layout::cross_v_index(8 * i + (lane >> 3), (lane & 7) * 8, SWZ));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[2 * e] = fmaf(pr[i], h16lo(vv[e]), o[2 * e]);
        o[2 * e + 1] = fmaf(pr[i], h16hi(vv[e]), o[2 * e + 1]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = sum_hi3(o[e]);
    if (lane == 0) { part[0] = m; part[1] = lsum; }
    if (lane < 8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) part[2 + lane * 8 + e] = o[e];
    }
  }
}

// attn_block<true> on a block whose 16 pieces are already in registers (kr[i]: dims 8i..8i+7 of key `lane`; vr[i]: keys
// 8i..8i+7 of dim `lane`): the same operations in the same order, so a block gives the same bits from either home.
__device__ __forceinline__ int attn_regs_piece(int i, int lane) { return layout::kv_chunk_offset(0, i, lane); }
__device__ __forceinline__ void attn_block_regs(const u32x4 (&kr)[8], const u32x4 (&vr)[8], const unsigned* qp, bool valid, float* pw, float* part, int lane) {
  float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32x4 qh = *reinterpret_cast<const u32x4*>(qp + i * 4), ql = *reinterpret_cast<const u32x4*>(qp + 32 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[e] = h16dot2(kr[i][e], qh[e], sc[e]);
      sc[e] = h16dot2(kr[i][e], ql[e], sc[e]);
    }
    if (i & 1) __builtin_amdgcn_sched_barrier(0);  // the block's 64 registers leave room for two pieces of the query at a time
  }
  float s = ((sc[0] + sc[1]) + (sc[2] + sc[3])) * 0.125f;
  if (!valid) s = -INFINITY;
  const float m = wmax(s);
  const float pk = m > -INFINITY ? __expf(s - m) : 0.f;
  const float lsum = wsum(pk);
  const h16 ph = (h16)pk, pl = (h16)(pk - (float)ph);
  reinterpret_cast<h16*>(pw)[lane] = ph;
  reinterpret_cast<h16*>(pw + 32)[lane] = pl;
  __builtin_amdgcn_wave_barrier();
  float o0 = 0.f, o1 = 0.f;
  const unsigned* pwu = reinterpret_cast<const unsigned*>(pw);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32x4 h4 = *reinterpret_cast<const u32x4*>(pwu + i * 4), l4 = *reinterpret_cast<const u32x4*>(pwu + 32 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      o0 = h16dot2(vr[i][e], h4[e], o0);
      o0 = h16dot2(vr[i][e], l4[e], o0);
      o1 = h16dot2(vr[i][e + 1], h4[e + 1], o1);
      o1 = h16dot2(vr[i][e + 1], l4[e + 1], o1);
    }
    if (i & 1) __builtin_amdgcn_sched_barrier(0);
  }
  if (lane == 0) { part[0] = m; part[1] = lsum; }
  part[2 + lane] = o0 + o1;
}
#endif  // AXW_ATTN_MFMA

// merge nb (<= NCW) wave partials (m, l, o[64]) in LDS: returns (l, o[c]) rescaled to the common maximum *m_out.
// Unrolled over all NCW records with blocks >= nb masked: every LDS read goes out at once and the exponentials are
// independent (as a loop over a run-time nb this was nb dependent read -> exp -> FMA round trips on the one wave
// that every consumer of the attention output waits for).
__device__ __forceinline__ void merge_partials(const float* wpart, int nb, int c, float* m_out, float* l_out, float* o_out) {
  float mb[NCW], lb[NCW], ob[NCW];
#pragma unroll
  for (int b = 0; b < NCW; ++b) {
    const float mv = wpart[b * kPS], lv = wpart[b * kPS + 1], ov = wpart[b * kPS + 2 + c];
    const bool on = b < nb;
    mb[b] = on ? mv : -INFINITY;
    lb[b] = on ? lv : 0.f;
    ob[b] = on ? ov : 0.f;
  }
  float m = mb[0];
#pragma unroll
  for (int b = 1; b < NCW; ++b) m = fmaxf(m, mb[b]);
  float lt = 0.f, ov = 0.f;
#pragma unroll
  for (int b = 0; b < NCW; ++b) {
    const float f = mb[b] > -INFINITY ? __expf(mb[b] - m) : 0.f;
    lt = fmaf(f, lb[b], lt);
    ov = fmaf(f, ob[b], ov);
  }
  *m_out = m; *l_out = lt; *o_out = ov;
}


// ---------------------------------------------------------------------------------------- the query fold's pieces (decode_persistent.hip)
// fp32 weight rows of M: LPR lanes share a row, 2 * CH chunks of 4 floats per lane (element layout of rows_dot).
template <int LPR, int CH>
struct RowSetF32 {
  u32x4 w[2 * CH];
  float bias;
  __device__ __forceinline__ void prefetch(const float* W, const float* b, int K, int row, bool on, int ctid) {
    const int j = ctid % LPR;
    const float* wr = W + (long)row * K;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      w[2 * i] = *reinterpret_cast<const u32x4*>(wr + (j + LPR * i) * 8);
      w[2 * i + 1] = *reinterpret_cast<const u32x4*>(wr + (j + LPR * i) * 8 + 4);
    }
    bias = (on && j == 0) ? b[row] : 0.f;
  }
  __device__ __forceinline__ float run(const float* act, int ctid) const {
    const int j = ctid % LPR;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const float4 x0 = *reinterpret_cast<const float4*>(act + (j + LPR * i) * 8);
      const float4 x1 = *reinterpret_cast<const float4*>(act + (j + LPR * i) * 8 + 4);
      a0 = fmaf(__uint_as_float(w[2 * i][0]), x0.x, a0); a1 = fmaf(__uint_as_float(w[2 * i][1]), x0.y, a1);
      a0 = fmaf(__uint_as_float(w[2 * i][2]), x0.z, a0); a1 = fmaf(__uint_as_float(w[2 * i][3]), x0.w, a1);
      a0 = fmaf(__uint_as_float(w[2 * i + 1][0]), x1.x, a0); a1 = fmaf(__uint_as_float(w[2 * i + 1][1]), x1.y, a1);
      a0 = fmaf(__uint_as_float(w[2 * i + 1][2]), x1.z, a0); a1 = fmaf(__uint_as_float(w[2 * i + 1][3]), x1.w, a1);
    }
    return group_sum<LPR>(a0 + a1) + bias;
  }
};

// per-layer block of the fold arena (floats): M [D][D], then d, s, c [D] each, then the LayerNorm fold of the two LayerNorm-fed
// row phases (below): s_qkv, c_qkv [3D], s_fc1, c_fc1 [4D]
__host__ __device__ constexpr long qfold_stride(int d) { return (long)d * d + 17L * d; }
constexpr int QF_SQKV = 3, QF_CQKV = 6, QF_SFC1 = 9, QF_CFC1 = 13;  // vector offsets behind M, in units of D

// LDS-DMA of pieces i0..i1 of one wave's 64-key cross block (16 pieces of 1 KiB: 0-7 the K block, 8-15 the V block; 16 bytes per
// lane, the LDS destination of a piece is its base + lane * 16). gk, gv: the block in the cross caches (blocked K, row-major V);
// sKw, sVw: the wave's blocks in LDS. K lands as it is. A V piece is eight rows of the tile: lane = 8 (row % 8) + chunk, and with
// kCrossVSwizzle the lane fetches the chunk that layout::cross_v_source_piece gives its slot — the permutation is applied on the
// SOURCE address, inside the same eight 128-byte lines.
__device__ __forceinline__ void stage_cross_kv(const h16* gk, const h16* gv, h16* sKw, h16* sVw, int i0, int i1, int lane) {
  for (int i = i0; i < i1; ++i) {
    if (i < 8) {
      __builtin_amdgcn_global_load_lds((gptr_t)(gk + layout::kv_chunk_offset(0, i, lane)), (lds_ptr_t)(sKw + layout::kv_chunk_offset(0, i, 0)), 16, 0, kKvAux);
    } else {
      const int src = layout::cross_v_source_piece(64 * (i - 8) + lane, kCrossVSwizzle);
      __builtin_amdgcn_global_load_lds((gptr_t)(gv + 8 * src), (lds_ptr_t)(sVw + layout::kv_chunk_offset(0, i - 8, 0)), 16, 0, kKvAux);
    }
  }
}

// One cross-attention unit (a clip's head, one third of the 1536 padded keys) on the eight compute waves, behind the barrier that
// handed over the query: every wave runs its 64-key block from the LDS tiles (export_onnx.py:221-230: fp32 softmax, no mask but
// the padding), the wave that arrives last merges the eight partials and publishes the record — o[64] as four full lines, then
// (m, l). out: the record's granules; cnt: the LDS arrival counter.
__device__ __forceinline__ void cross_unit_block(const h16* sK, const h16* sV, const unsigned* qs, float* pscr, float* wpart, int* cnt, u64* out,
                                                 unsigned tag, int ca_split, int n_audio_ctx, int cw, int lane) {
  // this wave's own K/V tiles have landed. The builtin, not inline asm: behind an asm that may touch the counters the compiler
  // drains vmcnt at every following join (measured: +18 ms on Whisper-small for one such asm in a cold path)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  asm volatile("" ::: "memory");
  const int key = (ca_split * NCW + cw) * 64 + lane;
  attn_block<false, kCrossVSwizzle>(sK + cw * layout::kKvBlockElems, sV + cw * layout::kKvBlockElems, qs, key < n_audio_ctx, pscr + cw * 64, wpart + cw * kPS, lane);
  __builtin_amdgcn_wave_barrier();
  int old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
  old = __builtin_amdgcn_readfirstlane(old);
  if ((old + 1) % NCW == 0) {
    float m, lt, ov;
    merge_partials(wpart, NCW, lane, &m, &lt, &ov);
    gput(out + lane, tag, ov);
    if (lane < 2) gput(out + 64 + lane, tag, lane == 0 ? m : lt);
  }
}

// The row producers' merge of a head's kCrossSplit partial records into one element of the attention vector (softmax over the
// whole key range: rescale to the common maximum, then normalise), on values: ms, ls the records' m and l, os their o of the
// element. The one arithmetic of both forms below, so either gives the same bits.
__device__ __forceinline__ float merge_cross_values(const float (&ms)[kCrossSplit], const float (&ls)[kCrossSplit], const float (&os)[kCrossSplit]) {
  float m = ms[0];
#pragma unroll
  for (int sp = 1; sp < kCrossSplit; ++sp) m = fmaxf(m, ms[sp]);
  float lt = 0.f, ov = 0.f;
#pragma unroll
  for (int sp = 0; sp < kCrossSplit; ++sp) {
    const float f = ms[sp] > -INFINITY ? __expf(ms[sp] - m) : 0.f;
    lt = fmaf(f, ls[sp], lt);  // explicit fmaf: both call sites compile to the same operations
    ov = fmaf(f, os[sp], ov);
  }
  return ov / lt;
}
// The LDS form (the multi-clip launch; the one-clip launch with AXW_CO_MERGE_IN_GATHER=0): the records gathered into pbuf
// ([H][kCrossSplit][kPS] = o[64], m, l each) behind a workgroup barrier, element i of this lane.
__device__ __forceinline__ float merge_cross_records(const float* pbuf, int i) {
  const float* pp = pbuf + (i >> 6) * kCrossSplit * kPS;
  float ms[kCrossSplit], ls[kCrossSplit], os[kCrossSplit];
#pragma unroll
  for (int sp = 0; sp < kCrossSplit; ++sp) { ms[sp] = pp[sp * kPS + 64]; ls[sp] = pp[sp * kPS + 65]; os[sp] = pp[sp * kPS + (i & 63)]; }
  return merge_cross_values(ms, ls, os);
}
// The merge inside the gather (the one-clip launch with the query fold): lane task t < D / 2 = (head t / 32, dims 2 (t % 32), + 1)
// polls six pairs in one round trip — the dim pair of each of the head's kCrossSplit records (granules of the records at o_part,
// kRec apart), then each record's (m, l) pair — merges in registers and writes act[2 t], act[2 t + 1]. The tasks go to the compute
// waves, which idle here with little in their registers (the pollers hold the resident vocabulary rows: with half of the tasks they
// spill): ctid = thread index among the compute waves takes task ctid, the lanes beyond D / 2 none (they still take part in the
// give-up logic). Returns true on give-up; what it wrote then is discarded behind the caller's check barrier.
template <int D>
__device__ __forceinline__ bool co_gather_merge(__amdgpu_buffer_rsrc_t rs, unsigned tag, int o_part, int ctid, float* act, const unsigned* err, const int* ctl) {
  static_assert(D / 2 <= CT, "one merge task per compute lane");
  const int t = ctid < D / 2 ? ctid : -1;
  // All six pairs are reloaded until every tag matches: no per-pair state (gather2 keeps a flag, an index and two values per
  // pair, 24 registers more than the row producers have at this point), and two addresses with constant offsets.
  const int b_o = (o_part + (t >> 5) * kCrossSplit * kRec + 2 * (t & 31)) * 8, b_ml = (o_part + (t >> 5) * kCrossSplit * kRec + 64) * 8;
  u32x4 xo[kCrossSplit], xm[kCrossSplit];
  bool fail = false;
  long long t_start = 0;
  for (int spins = 0;; ++spins) {
    bool all = true;
    if (t >= 0) {
#pragma unroll
      for (int sp = 0; sp < kCrossSplit; ++sp) xo[sp] = __builtin_amdgcn_raw_buffer_load_b128(rs, b_o + sp * kRec * 8, 0, 16);  // aux 16 = sc1
#pragma unroll
      for (int sp = 0; sp < kCrossSplit; ++sp) xm[sp] = __builtin_amdgcn_raw_buffer_load_b128(rs, b_ml + sp * kRec * 8, 0, 16);
#pragma unroll
      for (int sp = 0; sp < kCrossSplit; ++sp) all &= xo[sp][1] == tag && xo[sp][3] == tag && xm[sp][1] == tag && xm[sp][3] == tag;
    }
    if (all) break;
    if ((spins & 63) == 63 && *(volatile const int*)ctl) { fail = true; break; }  // a wave of this workgroup gave up
    if ((spins & 255) == 255 && spins >= kSpinFree) {
      if (eget(err)) { fail = true; break; }                                      // another workgroup gave up: leave as well
      const long long now = wall_clock64();
      if (t_start == 0) t_start = now;
      else if (now - t_start > kSpinTicks) { fail = true; break; }
    }
  }
  if (t >= 0) {
    float ms[kCrossSplit], ls[kCrossSplit], o0[kCrossSplit], o1[kCrossSplit];
#pragma unroll
    for (int sp = 0; sp < kCrossSplit; ++sp) {
      o0[sp] = __uint_as_float(xo[sp][0]); o1[sp] = __uint_as_float(xo[sp][2]);
      ms[sp] = __uint_as_float(xm[sp][0]); ls[sp] = __uint_as_float(xm[sp][2]);
    }
    *reinterpret_cast<float2*>(act + 2 * t) = float2{merge_cross_values(ms, ls, o0), merge_cross_values(ms, ls, o1)};
  }
  return fail;
}

// A cross-attention unit's side of the query fold: wave 0 gathers the head's 64 T values (lanes 0-31, pairs at granule base_cq)
// and the row producers' statistics (lanes 32.., up to two producers each, one 16-granule line per producer at base_stat),
// derives mu / r of x1 = x0 + y1 (shift = the mean of x0, the same bits in every workgroup) and leaves the query
// cq_j = r (T_j - mu s_j) + c_j as packed (hi, lo) h16 pairs in qs. vec: the layer's fold vectors behind M (d, s, c at 0, D, 2D).
// Every wave of the pollers calls it (the gather's give-up logic is workgroup-wide); returns true on give-up.
template <int D, int NP_D>
__device__ __forceinline__ bool qfold_unit_query(__amdgpu_buffer_rsrc_t GR, unsigned tag, int tid, int base_cq, int base_stat, const float* vec,
                                                 int head, float shift, unsigned* qs, const unsigned* err, const int* ctl) {
  constexpr int SL = (NP_D + 1) / 2;  // lanes that hold statistics
  static_assert(32 + SL <= 64, "statistics lanes");
  float sj[2] = {0.f, 0.f}, cj[2] = {0.f, 0.f};
  if (tid < 32) {
    const float2 s2 = *reinterpret_cast<const float2*>(vec + D + head * 64 + 2 * tid);
    const float2 c2 = *reinterpret_cast<const float2*>(vec + 2 * D + head * 64 + 2 * tid);
    sj[0] = s2.x; sj[1] = s2.y; cj[0] = c2.x; cj[1] = c2.y;
  }
  unsigned v[4];
  const bool fail = gather2<2>(GR, tag, v, err, ctl, [&](int k2) {
    if (tid < 32) return k2 == 0 ? base_cq + head * 64 + 2 * tid : -1;
    const int pi = (tid - 32) + k2 * SL;
    return (tid < 32 + SL && pi < NP_D) ? base_stat + 16 * pi : -1;
  });
  if (tid < 64) {
    const bool st = tid >= 32;
    const float t1 = wsum(st ? __uint_as_float(v[0]) + __uint_as_float(v[2]) : 0.f);
    const float t2 = wsum(st ? __uint_as_float(v[1]) + __uint_as_float(v[3]) : 0.f);
    const float dm = t1 / D, var = fmaxf(t2 / D - dm * dm, 0.f);
    const float mu = shift + dm, r = rsqrtf(var + 1e-5f);
    if (tid < 32) {
      const float q0 = r * (__uint_as_float(v[0]) - mu * sj[0]) + cj[0], q1 = r * (__uint_as_float(v[1]) - mu * sj[1]) + cj[1];
      unsigned hi, lo;
      h16split2(q0, q1, hi, lo);
      qs[tid] = hi;
      qs[32 + tid] = lo;
    }
  }
  return fail;
}

// A row producer's side: the slot leaders have left y1 in pk[slot], T in pk[32 + slot] and x1 - shift in pscr[slot]; the compute
// wave that arrives last (LDS counter cnt) stores T, the two sums and y1 — three lines, one store instruction each, the ones
// the units wait for first. Gc: the clip's granule area; o_cq / o_stat / o_y1: buffer offsets; r0: first row, nrows <= 32.
__device__ __forceinline__ void qfold_publish(int lane, const float* pk, const float* pscr, int* cnt, u64* Gc, int o_cq, int o_stat, int o_y1,
                                              int r0, int nrows, int producer, unsigned tag) {
  __builtin_amdgcn_wave_barrier();
  int old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
  old = __builtin_amdgcn_readfirstlane(old);
  if ((old + 1) % NCW == 0) {
    const bool on = lane < nrows;
    const float tv = on ? pscr[lane] : 0.f;
    const float s1 = wsum(tv), s2 = wsum(tv * tv);
    if (on) gput(Gc + o_cq + r0 + lane, tag, pk[32 + lane]);
    if (lane < 2) gput(Gc + o_stat + 16 * producer + lane, tag, lane == 0 ? s1 : s2);
    if (on) gput(Gc + o_y1 + r0 + lane, tag, pk[lane]);
  }
}

// ---------------------------------------------------------------------------------------- kernel prologue (both launches)
// Macros, not functions: they name the kernel's own values (template arguments, tid, ctl, p, ...), and a helper that took
// them as arguments was measured to move the register allocation of the production kernels.
// The shapes: a poller lane owns PAIRS of adjacent vector elements: pair tid + j*PL (j < GPD) = elements 2*pair, 2*pair + 1;
// the cross-attention partial records travel as pairs, split between the roles (NPP1 by the pollers, the rest by the compute
// waves); NU cross-attention units per layer and clip. Granule buffers of a clip in u64 units: the statistics of row producer
// p (query fold) at O_STAT + 16 p, + 1 — a line of its own (packed, 8 producers' partial-line stores per line: units gather
// 0.4 us later, 108.7 -> 111.1 ms).
#define AXW_PERSIST_SHAPES                                                                                                   \
  constexpr int D = 8 * LD * CD, F = 8 * LF * CF, H = D / 64;                                                                \
  static_assert(F == 4 * D, "mlp width");                                                                                    \
  constexpr int GPD = (D / 2 + PL - 1) / PL, GD = 2 * GPD, NPART = H * kCrossSplit * kPS;                                    \
  constexpr int NPP = NPART / 2, NPP1 = (NPP + 1) / 2, GP1 = (NPP1 + PL - 1) / PL, GP2 = (NPP - NPP1 + CT - 1) / CT;         \
  static_assert(NPART % 2 == 0 && kPS % 2 == 0 && kRec % 2 == 0 && D % 2 == 0, "pair polls need even layouts");             \
  constexpr int NU = kCrossSplit * H;                                                                                        \
  constexpr int O_QKV = 0, O_ATT = 3 * D, O_Y1 = 4 * D, O_CQ = 5 * D, O_PART = 6 * D, O_Y2 = 10 * D, O_HID = 11 * D,          \
                O_Y3 = 15 * D, O_AMAX = 16 * D, O_STAT = 16 * D + 512;                                                       \
  static_assert(NPART <= 3 * D + D / 8 && NU * kRec <= 4 * D, "partial buffer");                                             \
  static_assert(kCrossSplit * NCW == 24, "cross-attention key blocks");

// The LDS both kernels carve the same way (persist_lds_bytes); QS_GAP: words between the LayerNorm sums and the query.
//   sK [8 blk][8][64 keys][8] (blocked, lane = key); sV: cross tiles [512 keys][64], self-attention cache per block
//   [8 (key/8)][64 dims][8 keys]; act [F + D/8]: input vector of the current rows phase; wpart [NCW][kPS]: per-wave attention
//   partials; red [2*NPW]: LayerNorm partial sums; qs [64]: query of the attention phase as packed h16 pairs ([32] hi, [32] lo);
//   am_v, am_i [16]: argmax scratch; ctl [16]: 0 give-up flag, 1 argmax of the step, 2.. LDS arrival counters; pk [64]: this
//   workgroup's rows of the phase, assembled for the one-instruction publish; pscr [NCW][64]: probability transpose scratch;
//   prof_acc [64]: per-phase time sums + one layer's absolute timeline (profiling runs only)
#define AXW_PERSIST_LDS(QS_GAP)                                                                                              \
  extern __shared__ __attribute__((aligned(16))) char smem[];                                                                \
  h16* sK = reinterpret_cast<h16*>(smem);                                                                                    \
  h16* sV = sK + NCW * layout::kKvBlockElems;                                                                                                 \
  float* act = reinterpret_cast<float*>(smem + kKvBytes);                                                                    \
  float* wpart = act + F + D / 8;                                                                                            \
  float* red = wpart + NCW * kPS;                                                                                            \
  unsigned* qs = reinterpret_cast<unsigned*>(red + 2 * NPW + QS_GAP);                                                        \
  float* am_v = reinterpret_cast<float*>(qs) + 64;                                                                           \
  int* am_i = reinterpret_cast<int*>(am_v + 16);                                                                             \
  int* ctl = am_i + 16;                                                                                                      \
  float* pk = reinterpret_cast<float*>(ctl + 16);                                                                            \
  float* pscr = pk + 64;                                                                                                     \
  long long* prof_acc = reinterpret_cast<long long*>(pscr + NCW * 64);

// tid is re-derived behind an opaque asm at the top of every layer: without it the compiler hoists every per-thread address
// of every phase out of the step loop and keeps >100 registers of loop invariants alive
#define AXW_PERSIST_IDS                                                                                                      \
  int tid = threadIdx.x;                                                                                                     \
  const bool poller = tid < PL; /* wave-uniform */                                                                           \
  const int P = gridDim.x, wg = blockIdx.x;                                                                                  \
  const int L = p.n_layer;                                                                                                   \
  u64* const G = p.gran;

// Self-attention ownership: unit (l, h) -> workgroup P-1-(l*H+h); the other NS workgroups take the cross-attention units
// (ca_unit_of). Producers of the d-row phases (one pass of CT/LD resp. CT/LF rows each): only they consume the attention
// outputs / cross-attention partials / mlp hidden vector; every other workgroup skips those three phases altogether (no polls,
// no barriers): a hand-off is the faster the fewer workgroups poll it (-5 % decode time). Row roles go by a ROTATED workgroup
// index (rwg 0 = the first self-attention owner): the d-wide layers' producers are then workgroups that own a head (busy with
// attention in one layer of twelve), not the ones that run a cross-attention unit in most layers — with several clips
// interleaved, a producer that is also a unit holder puts one clip's rows behind the other clip's attention block.
#define AXW_PERSIST_ROLES                                                                                                    \
  const int sa_unit = P - 1 - wg;                                                                                            \
  const int sa_layer = sa_unit < L * H ? sa_unit / H : -1, sa_head = sa_unit % H;                                            \
  const int NS = P - L * H;                                                                                                  \
  constexpr int NP_D = (D + CT / LD - 1) / (CT / LD), NP_F2 = (D + CT / LF - 1) / (CT / LF);                                 \
  const int rwg = (wg - NS + P) % P;                                                                                         \
  const bool in_o = rwg < NP_D, in_f2 = rwg < NP_F2;

// The fault hook (AX_WHISPER_PERSIST_FAULT: a workgroup that never publishes; everybody else must give up and drain), the
// zeroed K/V region (masked keys must be finite), the control words and the profile sums. Then kargs: launch parameters that
// are read once per STEP or less (token feedback, teacher forcing, dumps, results) are not kept in scalar registers for the
// whole launch; AXW_COLD re-reads them from the kernel-argument segment at their use, through a pointer the compiler cannot see
// through (so it can neither hoist the loads out of the step loop nor keep their results live). The d_model-768 instantiation
// was spilling 185 scalar registers into vector lanes.
#define AXW_PERSIST_INIT                                                                                                     \
  if (p.fault && wg == 0) return;                                                                                            \
  for (int i = tid; i < kKvBytes / 16; i += PT) reinterpret_cast<u32x4*>(smem)[i] = u32x4{0u, 0u, 0u, 0u};                   \
  if (tid < 16) ctl[tid] = 0;                                                                                                \
  if (PROF && tid < 64) prof_acc[tid] = 0;                                                                                   \
  __syncthreads();                                                                                                           \
  long long t_last = PROF ? wall_clock64() : 0;                                                                              \
  const __attribute__((address_space(4))) PersistParams* kargs =                                                             \
      (const __attribute__((address_space(4))) PersistParams*)__builtin_amdgcn_kernarg_segment_ptr();
#define AXW_COLD(FIELD) ([&] { auto* kp_ = kargs; asm volatile("" : "+s"(kp_)); return kp_->FIELD; }())

// profile stamps: pollers stamp slots 0..15 (thread 0), compute waves 16..31 (thread PL)
#define AXW_STAMP(IDX) \
  if (PROF && (tid == 0 || tid == PL)) { const long long t_now = wall_clock64(); prof_acc[IDX] += t_now - t_last; t_last = t_now; }
// first barrier of a phase: everybody learns whether a poller gave up
#define AXW_BARRIER_CHECK(CODE)                                                                                          \
  {                                                                                                                      \
    wg_barrier();                                                                                                        \
    if (ctl[0]) {                                                                                                        \
      if (tid == 0) __hip_atomic_store((gu32*)p.err, (unsigned)(CODE) | 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
      return;                                                                                                            \
    }                                                                                                                    \
  }

// The pollers' per-register-slot helpers: el(k) = vector element of register slot k; g2_prefetch (QF, row producers): the
// cross-attention LayerNorm's gain of the NEXT layer to run (A0 = W_cq (g . x0)), requested a stage ahead like lg / lb by
// ln_prefetch — a polling wave must have no load in flight.
#define AXW_POLLER_PREFETCH                                                                                                  \
  auto el = [&](int k) { return 2 * (tid + (k >> 1) * PL) + (k & 1); };                                                     \
  float g2[GD];                                                                                                              \
  auto g2_prefetch = [&](int layer) {                                                                                        \
    _Pragma("unroll") for (int k = 0; k < GD; ++k) {                                                                         \
      const int i = el(k);                                                                                                   \
      g2[k] = (QF && in_o && i < D) ? p.fl[(long)layer * DecArena::f_stride(D) + DecArena::F_CROSS_LN_W * D + i] : 0.f;      \
    }                                                                                                                        \
  };                                                                                                                         \
  g2_prefetch(0);                                                                                                            \
  auto ln_prefetch = [&](const float* g, const float* be) {                                                                  \
    _Pragma("unroll") for (int k = 0; k < GD; ++k) {                                                                         \
      const int i = el(k);                                                                                                   \
      lg[k] = i < D ? g[i] : 0.f;                                                                                            \
      lb[k] = i < D ? be[i] : 0.f;                                                                                           \
    }                                                                                                                        \
  };
// a clip's residual stream at the start of a step: x = token_embedding[TOK] + positional_embedding[step] (export_onnx.py:334-336)
#define AXW_EMBED(X, TOK)                                                                                                    \
  _Pragma("unroll") for (int k = 0; k < GD; ++k) {                                                                           \
    const int i = el(k);                                                                                                     \
    X[k] = i < D ? (float)AXW_COLD(tok_emb)[(long)(TOK) * D + i] + AXW_COLD(pos)[(long)step * D + i] : 0.f;                 \
  }
// the end of a launch: no LDS-DMA may still be in flight when the workgroup's LDS is released (vmcnt(0)); the profile sums out
#define AXW_PERSIST_DRAIN                                                                                                    \
  __builtin_amdgcn_s_waitcnt(0x0F70);                                                                                        \
  if (PROF) {                                                                                                                \
    __syncthreads();                                                                                                         \
    if (tid < 64) AXW_COLD(prof)[(long)wg * 64 + tid] = prof_acc[tid];                                                       \
  }

// Cross-attention unit of workgroup wg in the t-th layer of the LAUNCH (t = step * L + l), or -1; nu units per layer, ns
// workgroups without a self-attention head. The units of consecutive layers take consecutive ranges of nu workgroups modulo
// ns, counted over the whole launch and not per step: 2 * nu <= ns then keeps the two units of any workgroup at least two
// layers apart across the step boundary as well. (Counted per step, the last layer's range wrapped onto the first layer's of
// the next step whenever L * nu > ns — large-v3-turbo: 4 x 60 units on 176 workgroups — and a workgroup staged the next
// step's K tiles over the ones its last-layer unit had not used yet: logits off by 4e-2 at every step of that model.)
// (__host__ as well: persistent_decode_plan hands this very function to the host-side check of the assignment.)
__host__ __device__ __forceinline__ int ca_unit_of(int t, int nu, int wg, int ns) {
  if (wg >= ns) return -1;
  int r = (wg - (int)(((long)t * nu) % ns)) % ns;
  if (r < 0) r += ns;
  return r < nu ? r : -1;
}

// ---------------------------------------------------------------------------------------- host side
// LDS bytes of a launch with nc clips: the K/V region and the carve-up of both kernels (act [F + D/8], wpart, red, qs, am_v,
// am_i, ctl, pk, pscr, prof_acc), then per layout: one clip keeps 4 words behind the LayerNorm sums (the stage's mean and
// shift); several clips keep, per clip after the first, its d-wide input vector, query (64 words), argmax scratch (32) and the
// self-attention k, v rows of its current step (64), then the poller waves' attention scratch and the query fold's 68 words
// per clip
inline size_t persist_lds_bytes(int d, int nc) {
  const size_t common = (size_t)kKvBytes + ((size_t)4 * d + d / 8 + NCW * kPS + 2 * NPW + 64 + 16 + 16 + 16 + 64 + NCW * 64) * 4 + 64 * 8 + 64;
  if (nc == 1) return common + 4 * 4;
  return common + ((size_t)(nc - 1) * (d + 64 + 32 + 64) + NPW * kPS + NPW * 64 + (size_t)nc * 68) * 4;
}

// The supported shapes: d_model = 8*LD*CD (rows with K = d: LD lanes x CD 16-byte chunks), 4*d_model = 8*LF*CF.
// fn(PersistShape<...>{}) for d_model, hipErrorInvalidValue for any other width.
template <int LD_, int CD_, int LF_, int CF_>
struct PersistShape { static constexpr int LD = LD_, CD = CD_, LF = LF_, CF = CF_, D = 8 * LD_ * CD_; };
template <typename Fn>
hipError_t persist_dispatch(int d_model, Fn&& fn) {
  switch (d_model) {
    case 128: return fn(PersistShape<16, 1, 32, 2>{});
    case 256: return fn(PersistShape<32, 1, 64, 2>{});
    case 384: return fn(PersistShape<16, 3, 64, 3>{});
    case 512: return fn(PersistShape<32, 2, 64, 4>{});
    case 768: return fn(PersistShape<32, 3, 64, 6>{});
    case 1280: return fn(PersistShape<32, 5, 64, 10>{});
    default: return hipErrorInvalidValue;
  }
}

// one persistent kernel instantiation on `grid` workgroups with the LDS of nc clips
// (extra_lds: bytes behind the common carve-up, the rules instantiation's)
inline hipError_t launch_persistent(void (*kfn)(PersistParams), int d, int nc, const PersistParams& p, int grid, hipStream_t s, size_t extra_lds = 0) {
  const size_t lds = persist_lds_bytes(d, nc) + extra_lds;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(PT), lds, s, p);
  return hipGetLastError();
}

// two or three clips per launch (decode_persistent2.hip); launch_decode_persistent hands n_clip >= 2 on
hipError_t launch_decode_persistent2(const PersistParams& p, int d_model, int grid, hipStream_t s);

}  // inline namespace AXW_NS
}  // namespace axw
