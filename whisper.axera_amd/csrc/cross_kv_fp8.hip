// cross_kv_fp8.hip — opt-in FP8 storage of the cross-attention K/V for the batched decoder step (AX_WHISPER_CROSS_KV=fp8).
//
// At batch sizes a decoder step is bound by the cross K/V stream (B x 55.3 MB per step against 277.8 MB of weights), and
// decode_attention_kernel already reads it near the HBM rate: what is left is moving fewer bytes. The format — OCP e4m3fn codes, one
// power-of-two scale per (layer, slot, head, K or V, head dimension) — is defined once in decode_layout.hpp.
//
//   cross_kv_quantize_kernel            the h16 images the encoder's EPI_CROSS_KV epilogue left -> code images + scales; the h16
//                                       images stay (the persistent launches, the GEMV family, prefill, alignment and beam search
//                                       keep reading them)
//   decode_cross_attention_fp8_kernel   decode_attention_kernel's cross-attention over the code images: the K scales multiply the
//                                       query (after it is formed), the V scales the output (after the final 1 / l); both exact
#include <type_traits>

#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

using layout::kPartStride;
using layout::kAttnSplitMax;
using layout::kPartM;
using layout::kPartL;
using layout::kPartO;

// ------------------------------------------------------------------------------- quantise
// One workgroup per (layer, clip, head, K or V); a thread owns 16 dimensions of one key of every 64-key block. Pass 1 takes the
// per-dimension amax over the valid keys, pass 2 converts: the head's 196 KB comes from L2 the second time. x * 2^-e is exact, the
// conversion instruction rounds it to nearest even once.
__global__ __launch_bounds__(256) void cross_kv_quantize_kernel(CrossKvQuantParams p) {
  __shared__ unsigned s_amax[64];
  __shared__ float s_inv[64];
  const int tid = threadIdx.x;
  const int kv = blockIdx.x & 1, head = blockIdx.x >> 1, b = blockIdx.y, l = blockIdx.z;
  const int slot = p.slot_map ? p.slot_map[b] : b;
  if (slot < 0 || slot >= p.n_slots) return;  // (workgroup-uniform)
  const long hidx = ((long)l * p.n_slots + slot) * p.n_head + head;
  const h16* src = (kv ? p.v : p.k) + hidx * layout::kv_head_elems(p.keys_pad);
  unsigned char* dst = (kv ? p.v8 : p.k8) + hidx * layout::kv8_head_bytes(p.keys_pad);
  const int c16 = kv ? tid & 3 : tid >> 6, row = kv ? tid >> 2 : tid & 63;  // K: lane = key; V: four threads per row
  const int n_keys = min(p.n_keys, p.keys_pad), n_blk = p.keys_pad >> 6, n_blk_valid = (n_keys + 63) >> 6;
  auto load16 = [&](int key, float* x) {  // the 16 values of (key, dims 16 c16 ..)
    const u32x4 lo = *reinterpret_cast<const u32x4*>(src + (kv ? layout::v_index(key, c16 * 16) : layout::k_index(key, c16 * 16)));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(src + (kv ? layout::v_index(key, c16 * 16 + 8) : layout::k_index(key, c16 * 16 + 8)));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[2 * e] = h16lo(lo[e]); x[2 * e + 1] = h16hi(lo[e]);
      x[8 + 2 * e] = h16lo(hi[e]); x[8 + 2 * e + 1] = h16hi(hi[e]);
    }
  };
  if (tid < 64) s_amax[tid] = 0u;
  __syncthreads();
  float a[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = 0.f;
  for (int blk = 0; blk < n_blk_valid; ++blk) {
    const int key = blk * 64 + row;
    if (key < n_keys) {
      float x[16];
      load16(key, x);
#pragma unroll
      for (int e = 0; e < 16; ++e) a[e] = fmaxf(a[e], fabsf(x[e]));
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) atomicMax(&s_amax[c16 * 16 + e], __float_as_uint(a[e]));  // (magnitudes order as their bit patterns)
  __syncthreads();
  if (tid < 64) {
    const int e = layout::kv8_scale_exponent(s_amax[tid]);
    p.scales[hidx * layout::kKv8ScaleHead + kv * layout::kKvDim + tid] = __uint_as_float(layout::kv8_pow2_bits(e));
    s_inv[tid] = __uint_as_float(layout::kv8_pow2_bits(-e));
  }
  __syncthreads();
  float inv[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) inv[e] = s_inv[c16 * 16 + e];
  for (int blk = 0; blk < n_blk; ++blk) {
    const int key = blk * 64 + row;
    u32x4 out = {0u, 0u, 0u, 0u};  // keys at or beyond the key count: code 0
    if (key < n_keys) {
      float x[16];
      load16(key, x);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w] * inv[4 * w], x[4 * w + 1] * inv[4 * w + 1], 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * w + 2] * inv[4 * w + 2], x[4 * w + 3] * inv[4 * w + 3], c, true);
        out[w] = (unsigned)c;
      }
    }
    *reinterpret_cast<u32x4*>(dst + (kv ? layout::v8_index(key, c16 * 16) : layout::k8_chunk_offset(blk, c16, row))) = out;
  }
}

void launch_cross_kv_quantize(const CrossKvQuantParams& p, hipStream_t s) {
  if (p.clips < 1 || p.n_layer < 1 || p.n_head < 1 || p.keys_pad < 64 || p.keys_pad % 64 != 0 || p.n_keys < 0 || p.n_keys > p.keys_pad ||
      p.clips > p.n_slots) { fprintf(stderr, "[ax_whisper] cross_kv_quantize: %d clips, %d slots, %d of %d keys unsupported\n", p.clips, p.n_slots, p.n_keys, p.keys_pad); abort(); }
  hipLaunchKernelGGL(cross_kv_quantize_kernel, dim3(2 * p.n_head, p.clips, p.n_layer), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------- attention
// A 16-byte buffer load of a code image (non-temporal, as decode_attention_kernel's ld_kv); off in bytes.
__device__ __forceinline__ u32x4 ld_kv8(const unsigned char* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x27000);
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 2);  // aux 2 = nt
}

// decode_attention_kernel (decoder.hip) over the code images; QM and NCHL as there. What differs:
//  - a 64-key block is 4 + 4 sixteen-byte loads per lane instead of 8 + 8, so a wave takes TWO blocks per iteration (blk and blk + 4:
//    the waves interleave over the blocks as before) and keeps the h16 kernel's 8 + 8 loads in flight; the two blocks share one
//    maximum, one rescale and one pass of the wave reductions;
//  - V: four lanes per key row, a lane accumulates 16 output dimensions (lane % 4);
//  - the query is multiplied by the K scales once it is formed (every mode goes through s_q for that), the output by the V scales
//    after the final 1 / l.
// Lanes whose key is at or beyond the key count read the last valid key (K) / row (V), and a wave whose second block lies beyond its
// range reads its first block again: bytes beyond the keys are never loaded, so no code there — NaN included — reaches a result.
// `p` MUST stay the kernel's FIRST argument: the tail re-reads its fields at offset 0 of the kernel-argument segment (below).
template <int QM, int NCHL = 0>
__global__ __launch_bounds__(256) void decode_cross_attention_fp8_kernel(DecAttnFp8Params p, int cap_blocks) {
  static_assert(alignof(DecAttnFp8Params) <= 8 && std::is_trivially_copyable<DecAttnFp8Params>::value, "read back from the kernel-argument segment");
  constexpr bool FUSE_Q = QM == 1;
  __shared__ float s_part[4][kPartStride];
  __shared__ float s_q[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int clip_done = p.done[b];
  if (!p.done_late && clip_done) return;
  const int bps = (cap_blocks + p.n_split - 1) / p.n_split;
  const int blk_begin = split * bps, blk_cap_end = min(cap_blocks, blk_begin + bps);
  const int n_keys = p.n_keys;  // >= 1 (the launcher checks)
  const int blk_end = min((n_keys + 63) >> 6, blk_cap_end);

  const unsigned char* kb = p.k8 + (long)b * p.kv_batch_bytes + head * layout::kv8_head_bytes(cap_blocks * layout::kKvBlockKeys);
  const unsigned char* vb = p.v8 + (long)b * p.kv_batch_bytes + head * layout::kv8_head_bytes(cap_blocks * layout::kKvBlockKeys);
  const float* sc_head = p.scales + (long)b * p.scale_batch_stride + head * layout::kKv8ScaleHead;

  u32x4 kn[8], vn[8];  // [0, 4): block blk, [4, 8): block blk + 4
  int blk = blk_begin + wave;
  // bk0 < blk_end; the second block, where it lies beyond the range, is the first one again (masked below)
  auto load_k = [&](int bk0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int bk = (j && bk0 + 4 < blk_end) ? bk0 + 4 : bk0;
      const int lk = max(0, min(lane, n_keys - 1 - bk * 64));
#pragma unroll
      for (int i = 0; i < 4; ++i) kn[4 * j + i] = ld_kv8(kb, layout::k8_chunk_offset(bk, i, lk));
    }
  };
  auto load_v = [&](int bk0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int bk = (j && bk0 + 4 < blk_end) ? bk0 + 4 : bk0;
      const int last = max(bk * 64, n_keys - 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) vn[4 * j + i] = ld_kv8(vb, layout::v8_index(min(bk * 64 + 16 * i + (lane >> 2), last), (lane & 3) * 16));
    }
  };
  if (blk < blk_end) { load_k(blk); load_v(blk); }

  // the head's 64 query values, times the K scales, through s_q
  if constexpr (FUSE_Q) {
    __shared__ __attribute__((aligned(16))) float s_act[1024];
    __shared__ float s_red[8];
    const int d = p.d_model;  // <= 1024, multiple of 32
    const float* xr = p.x + (long)b * d;
    float xv[4], gg[4], bb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = tid + 256 * e;
      xv[e] = c < d ? xr[c] : 0.f;
      gg[e] = c < d ? p.ln_w[c] : 0.f;
      bb[e] = c < d ? p.ln_b[c] : 0.f;
    }
    const int qrow = tid >> 2, qj = tid & 3;
    const h16* wr = p.wq + (long)(head * 64 + qrow) * d;
    const int nch = d >> 3;
    constexpr int NWC = NCHL > 0 ? NCHL : 8;
    u32x4 wc[NWC];
#pragma unroll
    for (int i = 0; i < NWC; ++i) {
      const int c = qj + 4 * i;
      if constexpr (NCHL > 0) wc[i] = *reinterpret_cast<const u32x4*>(wr + c * 8);
      else wc[i] = c < nch ? *reinterpret_cast<const u32x4*>(wr + c * 8) : u32x4{0u, 0u, 0u, 0u};
    }
    const float bq = p.bq[head * 64 + qrow];
    const float ksc = sc_head[qrow];
    if (clip_done) return;  // (workgroup-uniform, in front of the first barrier)
    float s1 = (xv[0] + xv[1]) + (xv[2] + xv[3]);
    float s2 = (xv[0] * xv[0] + xv[1] * xv[1]) + (xv[2] * xv[2] + xv[3] * xv[3]);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) { s_red[wave] = s1; s_red[4 + wave] = s2; }
    __syncthreads();
    const float mean = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / d;
    const float rstd = rsqrtf(fmaxf(((s_red[4] + s_red[5]) + (s_red[6] + s_red[7])) / d - mean * mean, 0.f) + 1e-5f);
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int c = tid + 256 * e; if (c < d) s_act[c] = (xv[e] - mean) * rstd * gg[e] + bb[e]; }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f;
    if constexpr (NCHL > 0) {
      float b0 = 0.f, b1 = 0.f;
#pragma unroll
      for (int i = 0; i < NCHL; ++i) {
        const int c = qj + 4 * i;
        const float4 y0 = *reinterpret_cast<const float4*>(s_act + c * 8), y1 = *reinterpret_cast<const float4*>(s_act + c * 8 + 4);
        a0 = fmaf(h16lo(wc[i][0]), y0.x, a0);
        a1 = fmaf(h16hi(wc[i][0]), y0.y, a1);
        b0 = fmaf(h16lo(wc[i][1]), y0.z, b0);
        b1 = fmaf(h16hi(wc[i][1]), y0.w, b1);
        a0 = fmaf(h16lo(wc[i][2]), y1.x, a0);
        a1 = fmaf(h16hi(wc[i][2]), y1.y, a1);
        b0 = fmaf(h16lo(wc[i][3]), y1.z, b0);
        b1 = fmaf(h16hi(wc[i][3]), y1.w, b1);
      }
      a0 += b0; a1 += b1;
    }
    for (int c0 = 0; c0 < nch && NCHL == 0; c0 += 32) {
      u32x4 cur[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) cur[i] = wc[i];
#pragma unroll
      for (int i = 0; i < 8; ++i) { const int c = c0 + 32 + qj + 4 * i; wc[i] = c < nch ? *reinterpret_cast<const u32x4*>(wr + c * 8) : u32x4{0u, 0u, 0u, 0u}; }
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
    if (qj == 0) s_q[qrow] = (acc + bq) * ksc;
  } else if constexpr (QM == 2) {
    const int d = p.d_model, nst = d >> 4;  // nst <= 64
    float tq = 0.f, sj = 0.f, cj = 0.f, ksc = 0.f;
    f32x2_t sp = {0.f, 0.f};
    if (wave == 0) {
      tq = p.tq[(long)b * d + head * 64 + lane];
      sj = p.fold_s[head * 64 + lane];
      cj = p.fold_c[head * 64 + lane];
      ksc = sc_head[lane];
      if (lane < nst) sp = *reinterpret_cast<const f32x2_t*>(p.stat_part + ((long)b * nst + lane) * 2);
    }
    if (clip_done) return;  // (workgroup-uniform, in front of the barrier)
    if (wave == 0) {
      const float mean = wave_sum(sp[0]) / (float)d;
      const float dm = sp[0] * (1.f / 16.f) - mean;
      const float m2 = wave_sum(lane < nst ? sp[1] + 16.f * dm * dm : 0.f);
      const float rstd = rsqrtf(m2 / (float)d + 1e-5f);
      s_q[lane] = (rstd * (tq - mean * sj) + cj) * ksc;
    }
  } else {
    float qx = 0.f, ksc = 0.f;
    if (wave == 0) { qx = p.q[(long)b * p.d_model + head * 64 + lane]; ksc = sc_head[lane]; }
    if (clip_done) return;  // (workgroup-uniform, in front of the barrier)
    if (wave == 0) s_q[lane] = qx * ksc;
  }
  __syncthreads();
  // (pairs: a conversion yields the codes of two neighbouring dimensions, and one packed FMA takes them with the query pair)
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 qv[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    qv[c][0] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_q[2 * c])));
    qv[c][1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_q[2 * c + 1])));
  }

  // The workgroup's coordinates cross the block loop in vector registers: the scalar file is full with the 64 query values, the two
  // buffer descriptors and the loop's own state, and what does not fit the allocator spills.
  int v_b = b, v_head = head, v_split = split;
  asm volatile("" : "+v"(v_b), "+v"(v_head), "+v"(v_split));

  float m_w = -INFINITY, l_lane = 0.f;
  f2 o2[8];  // output dimensions 16 (lane % 4) + 2 e, + 1
#pragma unroll
  for (int e = 0; e < 8; ++e) o2[e] = f2{0.f, 0.f};

  auto two_blocks = [&](int cur, bool prefetch) {
    float sc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // lane = key (cur + 4 j) * 64 + lane: dot(q, k) over 64 dims
      f2 s = {0.f, 0.f};  // even and odd dimensions: two chains of 32
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)kn[4 * j + i][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)kn[4 * j + i][w], true);
          s = __builtin_elementwise_fma(qv[8 * i + 2 * w], lo, s);
          s = __builtin_elementwise_fma(qv[8 * i + 2 * w + 1], hi, s);
        }
      }
      sc[j] = (s[0] + s[1]) * 0.125f;  // (64^-0.25)^2
    }
    const bool two = cur + 4 < blk_end;
    if (prefetch) load_k(cur + 8);
    if (cur * 64 + lane >= n_keys) sc[0] = -INFINITY;
    if (!two || (cur + 4) * 64 + lane >= n_keys) sc[1] = -INFINITY;
    const float m_new = fmaxf(m_w, wave_max(fmaxf(sc[0], sc[1])));
    const float alpha = __expf(m_w - m_new);
    const float pk[2] = {__expf(sc[0] - m_new), __expf(sc[1] - m_new)};
    m_w = m_new;
    l_lane = l_lane * alpha + (pk[0] + pk[1]);
#pragma unroll
    for (int e = 0; e < 8; ++e) o2[e] *= alpha;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float w = __shfl(pk[j], 16 * i + (lane >> 2), 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vn[4 * j + i][u], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vn[4 * j + i][u], true);
          o2[2 * u] = __builtin_elementwise_fma(f2{w, w}, lo, o2[2 * u]);
          o2[2 * u + 1] = __builtin_elementwise_fma(f2{w, w}, hi, o2[2 * u + 1]);
        }
      }
    }
    if (prefetch) load_v(cur + 8);
  };
  for (; blk < blk_end; blk += 8) two_blocks(blk, blk + 8 < blk_end);

  // What the tail needs of the parameters is read from the kernel-argument segment again (p is the kernel's first argument), through
  // a pointer the compiler cannot trace back: held across the block loop beside the 64 query values, those ~20 scalar registers
  // push the kernel over the scalar file and the allocator spills.
  typedef const __attribute__((address_space(4))) DecAttnFp8Params* KernArgs;
  KernArgs pa = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(pa));
  const int n_split = pa->n_split, n_head = pa->n_head;
  const int tb = __builtin_amdgcn_readfirstlane(v_b), th = __builtin_amdgcn_readfirstlane(v_head), ts = __builtin_amdgcn_readfirstlane(v_split);
  // wave partial: sum o over the 16 key sub-rows (lanes with equal lane & 3), sum l over the wave
  const float l_w = wave_sum(l_lane);
  float o[16];
#pragma unroll
  for (int e = 0; e < 8; ++e) { o[2 * e] = o2[e][0]; o[2 * e + 1] = o2[e][1]; }
#pragma unroll
  for (int e = 0; e < 16; ++e) {  // lanes l, l^4, l^8 inside the 16-lane row (two DPP rotations), then the row swaps
    o[e] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(o[e]), 0x124, 0xf, 0xf, true));  // row_ror:4
    o[e] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(o[e]), 0x128, 0xf, 0xf, true));  // row_ror:8
    {
      auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[e]), __float_as_uint(o[e]), false, false);
      o[e] = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    }
    {
      auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[e]), __float_as_uint(o[e]), false, false);
      o[e] = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    }
  }
  if (lane == 0) { s_part[wave][kPartM] = m_w; s_part[wave][kPartL] = l_w; }
  if (lane < 4) {
#pragma unroll
    for (int e = 0; e < 16; ++e) s_part[wave][kPartO + lane * 16 + e] = o[e];
  }
  __syncthreads();
  if (tid < 64) {
    const float vsc = (pa->scales + (long)tb * pa->scale_batch_stride + th * layout::kKv8ScaleHead)[layout::kKvDim + tid];
    float m = fmaxf(fmaxf(s_part[0][kPartM], s_part[1][kPartM]), fmaxf(s_part[2][kPartM], s_part[3][kPartM]));
    float l = 0.f, ov = 0.f;
    if (m > -INFINITY) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float f = __expf(s_part[w][kPartM] - m);
        l += f * s_part[w][kPartL];
        ov += f * s_part[w][kPartO + tid];
      }
    }
    float y;
    if (n_split > 1) {
      // the splits of a (clip, head) meet as in decode_attention_kernel: write-through records, a drained store queue, one ticket
      // per workgroup; whoever draws the last one folds all records in split order
      float* base = pa->mpart + layout::part_offset(tb, th, 0, n_head, n_split);
      float* mine = base + ts * kPartStride;
      __hip_atomic_store(mine + kPartO + tid, ov, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (tid == 0) {
        __hip_atomic_store(mine + kPartM, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + kPartL, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      unsigned ticket = 0;
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      if (tid == 0) ticket = __hip_atomic_fetch_add(pa->mcnt + tb * n_head + th, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      ticket = __builtin_amdgcn_readfirstlane(ticket);
      if (ticket != (unsigned)n_split - 1u) return;
      float ms[kAttnSplitMax], ls[kAttnSplitMax], os[kAttnSplitMax];
#pragma unroll
      for (int s2 = 0; s2 < kAttnSplitMax; ++s2) {
        ms[s2] = m; ls[s2] = l; os[s2] = ov;
        if (s2 < n_split && s2 != ts) {
          const float* other = base + s2 * kPartStride;
          ms[s2] = __hip_atomic_load(other + kPartM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ls[s2] = __hip_atomic_load(other + kPartL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          os[s2] = __hip_atomic_load(other + kPartO + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      float M = -INFINITY, Ls = 0.f, O = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < kAttnSplitMax; ++s2) {
        if (s2 < n_split) {
          const float m2 = ms[s2], l2 = ls[s2], o2 = os[s2];
          const float mn = fmaxf(M, m2);
          const float f1 = M > -INFINITY ? __expf(M - mn) : 0.f, f2 = m2 > -INFINITY ? __expf(m2 - mn) : 0.f;
          Ls = f1 * Ls + f2 * l2;
          O = f1 * O + f2 * o2;
          M = mn;
        }
      }
      if (tid == 0) __hip_atomic_store(pa->mcnt + tb * n_head + th, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
      y = O / Ls;
    } else {
      y = ov / l;
    }
    y *= vsc;
    const h16 yh = (h16)y;
    const long i = layout::frag_index(tb, th * 64 + tid, pa->nbs);
    pa->out_hi[i] = yh;
    pa->out_lo[i] = (h16)(y - (float)yh);
  }
}

void launch_decode_cross_attention_fp8(const DecAttnFp8Params& p, hipStream_t s) {
  if (!p.k8 || !p.v8 || !p.scales || !p.done || !p.out_hi || !p.out_lo || p.n_keys < 1 || p.n_keys > p.cap_blocks * layout::kKvBlockKeys ||
      p.n_split < 1 || p.n_split > kAttnSplitMax || (p.n_split != 1 && !(p.mpart && p.mcnt))) {
    fprintf(stderr, "[ax_whisper] fp8 cross-attention: %d keys in %d blocks, n_split %d unsupported\n", p.n_keys, p.cap_blocks, p.n_split); abort();
  }
  const dim3 grid(p.n_split, p.n_head, p.batch);
  if (p.tq) {  // folded query
    if (p.d_model > 1024 || p.d_model % 64 != 0 || !p.stat_part || !p.fold_s || !p.fold_c) { fprintf(stderr, "[ax_whisper] fp8 cross-attention, folded query: d_model %d unsupported\n", p.d_model); abort(); }
    hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<2>), grid, dim3(256), 0, s, p, p.cap_blocks);
  } else if (p.wq) {
    if (p.d_model > 1024 || p.d_model % 32 != 0) { fprintf(stderr, "[ax_whisper] fp8 cross-attention, fused query projection: d_model %d unsupported\n", p.d_model); abort(); }
    if (p.d_model == 384) hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<1, 12>), grid, dim3(256), 0, s, p, p.cap_blocks);
    else if (p.d_model == 512) hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<1, 16>), grid, dim3(256), 0, s, p, p.cap_blocks);
    else if (p.d_model == 768) hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<1, 24>), grid, dim3(256), 0, s, p, p.cap_blocks);
    else if (p.d_model == 1024) hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<1, 32>), grid, dim3(256), 0, s, p, p.cap_blocks);
    else hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<1>), grid, dim3(256), 0, s, p, p.cap_blocks);
  } else {
    if (!p.q) { fprintf(stderr, "[ax_whisper] fp8 cross-attention: no query\n"); abort(); }
    hipLaunchKernelGGL((decode_cross_attention_fp8_kernel<0>), grid, dim3(256), 0, s, p, p.cap_blocks);
  }
}

}  // inline namespace AXW_NS
}  // namespace axw
