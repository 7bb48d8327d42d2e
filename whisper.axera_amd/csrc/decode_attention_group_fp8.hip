// decode_attention_group_fp8.hip — grouped single-query cross-attention over the FP8 code images, for beam search on a handle
// opened with AX_WHISPER_CROSS_KV=fp8 AND AX_WHISPER_BEAM_CROSS=shared (DESIGN.md "Shared cross K/V over FP8 codes").
//
// The work split is decode_cross_attention_group_kernel's (decode_attention_group.hip): one workgroup per (key split, head, clip)
// streams the clip's own K/V — here the e4m3fn codes of slot c, half the bytes of the h16 images — ONCE for all ranks of the clip
// inside the launch's slot range; four waves interleave over the 64-key blocks; G <= 8 ranks x the (hi, lo) h16 split of an fp32 row
// are the 16-row A operand of v_mfma_f32_16x16x32; fp32 online softmax per lane group. A code converts to the 16-bit operand type
// exactly (e4m3 has 4 significant bits and the exponent range 2^-9 .. 2^8), so the matrix cores multiply the code VALUES.
//
// K. The byte image is [blk][dim / 16][64 keys][16]: a 16-byte piece holds 16 dimensions of one key. The contraction order of an
//   MFMA is free as long as A and B agree, so lane l of the B operand of the 16-key block kb loads ONE piece, chunk l / 16 of key
//   16 kb + l % 16, and its bytes 0 .. 7 are the lane's B fragment of k-step 0, its bytes 8 .. 15 that of k-step 1:
//       k-slot (k-step ks, 8 (l / 16) + j)  <->  head dimension 16 (l / 16) + 8 ks + j,
//   i.e. dimension d sits at column qa_col(d) = 32 (d / 8 % 2) + 8 (d / 16) + d % 8 of the query image s_qa. Four 16-byte
//   non-temporal buffer loads per lane and block (the h16 kernel: eight), straight from global memory into registers.
// V. Row-major [key][64] bytes, 4 KB per 64-key tile. A lane loads the 8-byte piece (row 8 i + l / 8, dims 8 (l % 8) ..) — a wave's
//   load is 512 contiguous bytes — converts it in registers to the 16-byte h16 chunk the h16 kernel would have loaded, and writes
//   it to the SAME LDS slot of the layout::cross_v_swizzle image: the writes and the ds_read_b64_tr_b16 reads keep the h16 kernel's
//   proven conflict-free form, and nothing of the output product changes.
// Scales. V's per-dimension 2^e multiplies the fp32 output of that dimension behind the final 1 / l, exactly. K's per-dimension
//   2^e_d is folded into the query with one exponent shift s per rank: A_d = ldexp(q_d, e_d - s), s = max_d (ilogb(q_d) + e_d) - 14,
//   so the largest |A_d| of a rank lies in [2^14, 2^15) — inside fp16's range whatever q and the scales are — and the fp32 score
//   is ldexp(sum, s - 3) (the 1 / 8 of the head dimension with it). Every step but the (hi, lo) split of A_d is an exact power-of-two
//   scaling. What the form costs: where A_d falls below the 16-bit type's normal range its pair is no longer relative; the absolute
//   error 2^-25 (half) / 2^-126 (bfloat16) of the pair becomes 2^(s - e_d) times that in units of q_d (DESIGN.md derives the bound).
// Keys at or beyond n_keys are never loaded (the parents' clamp rule: such a lane reads the last valid key again, its score is -inf and
// its V row meets probability 0): no code there, 0x7f / 0xff included, reaches a result.
//
// Query modes, split record, ticket hand-off, output pair, done / done_late and the slot range that may cut a group: as in
// decode_attention_group.hip, through decode_attention_common.hpp. The three modes leave fp32 query values in LDS first (the fold
// above needs a rank's 64 values together).
#include "common.hpp"
#include "decode_attention_common.hpp"
#include "decode_attention_group_common.hpp"

namespace axw {
inline namespace AXW_NS {

using layout::kPartStride;
using layout::kAttnSplitMax;
using layout::kPartM;
using layout::kPartL;
using layout::kPartO;

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// base: wave-uniform pointer of this (clip, head)'s code image, off: this lane's byte offset (non-temporal, as ld_kv_nt)
__device__ __forceinline__ u32x4 ld_k8_nt(const unsigned char* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x27000);
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 2);  // aux 2 = nt
}
__device__ __forceinline__ u32x2 ld_v8_nt(const unsigned char* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x27000);
  return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 2);
}
// two fp32 values that h16 holds exactly -> one packed dword (element 0 in the low half)
__device__ __forceinline__ unsigned pack_exact(float a, float b) {
#if AXW_F16
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
#else
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);  // the upper halves of b : a
#endif
}
// eight codes (two dwords, ascending dimension / key order) -> eight h16, exactly
__device__ __forceinline__ h16x8 codes_to_h16(unsigned w0, unsigned w1) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  const u32x4 r = {pack_exact(a[0], a[1]), pack_exact(b[0], b[1]), pack_exact(c[0], c[1]), pack_exact(d[0], d[1])};
  return __builtin_bit_cast(h16x8, r);
}
// column of head dimension d in the query image (the K permutation of the file header)
__device__ __forceinline__ int qa_col(int d) { return 32 * ((d >> 3) & 1) + 8 * (d >> 4) + (d & 7); }

template <int QM>
__global__ __launch_bounds__(256) void decode_cross_attention_group_fp8_kernel(DecAttnGroupFp8Params p) {
  // the waves' h16 V tiles [4][64 keys][64 dims]; in front of the key loop the fused mode's LayerNormed rows [G][1024] fp32, behind it
  // the waves' records [4][8 ranks][66] fp32 (each wave's inside its own tile)
  __shared__ __attribute__((aligned(16))) h16 s_v[4 * layout::kKvBlockElems];
  // the waves' probability images; in front of the key loop the ranks' fp32 query values [8][64]
  __shared__ __attribute__((aligned(16))) h16 s_p[4 * kAImage];
  __shared__ __attribute__((aligned(16))) h16 s_qa[kAImage];
  __shared__ int s_shift[kGroupMax];
  __shared__ unsigned s_ticket;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x, head = blockIdx.y;
  const int clip = p.slot0 / p.group + blockIdx.z;
  const int r_lo = max(0, p.slot0 - clip * p.group), r_hi = min(p.group, p.slot0 + p.nslots - clip * p.group);
  const int G = r_hi - r_lo;                         // 1 .. 8 ranks of this clip inside the range
  const int rel0 = clip * p.group + r_lo - p.slot0;  // the first of them, counted from slot0
  unsigned live = 0;
  for (int g = 0; g < G; ++g) live |= (p.done[rel0 + g] ? 0u : 1u) << g;
  if (!p.done_late && !live) return;

  const int bps = (p.cap_blocks + p.n_split - 1) / p.n_split;
  const int blk_begin = split * bps;
  const int blk_end = min((p.n_keys + 63) >> 6, min(p.cap_blocks, blk_begin + bps));
  const long head_bytes = layout::kv8_head_bytes(p.cap_blocks * layout::kKvBlockKeys);
  const unsigned char* kb = p.k8 + (long)clip * p.kv_slot_bytes + head * head_bytes;
  const unsigned char* vb = p.v8 + (long)clip * p.kv_slot_bytes + head * head_bytes;
  const float* sc_head = p.scales + (long)clip * p.scale_slot_stride + head * layout::kKv8ScaleHead;  // the clip's own slot

  u32x4 kn[4];  // kn[kb]: chunk lane / 16 of key 16 kb + lane % 16: both k-steps' B fragments of the 16-key block
  u32x2 vn[8];  // vn[i]: row 8 i + lane / 8 of the V tile, dims 8 (lane % 8) ..
  auto load_k = [&](int bk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = max(0, min(16 * i + (lane & 15), p.n_keys - 1 - bk * 64));
      kn[i] = ld_k8_nt(kb, layout::k8_chunk_offset(bk, lane >> 4, key));
    }
  };
  auto load_v = [&](int bk) {
#pragma unroll
    for (int i = 0; i < 8; ++i) vn[i] = ld_v8_nt(vb, layout::v8_index(min(bk * 64 + 8 * i + (lane >> 3), p.n_keys - 1), (lane & 7) * 8));
  };
  int blk = blk_begin + wave;
  if (blk < blk_end) { load_k(blk); load_v(blk); }
  if (!live) return;  // (done_late: behind the first requests)

  // ---- the ranks' fp32 queries -> s_q
  float* s_q = reinterpret_cast<float*>(s_p);
  if constexpr (QM == 1) {
    float* s_act = reinterpret_cast<float*>(s_v);
    const int d = p.d_model;  // <= 1024, a multiple of 32
    for (int g = wave; g < G; g += 4) {  // LayerNorm of rank g's row by one wave, two passes over registers
      const float* xr = p.x + (long)(rel0 + g) * d;
      float xv[16];
      float s1 = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) { const int c = lane + 64 * e; xv[e] = c < d ? xr[c] : 0.f; s1 += xv[e]; }
      const float mean = wave_sum(s1) / (float)d;
      float s2 = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) { const float t = lane + 64 * e < d ? xv[e] - mean : 0.f; s2 = fmaf(t, t, s2); }
      const float rstd = rsqrtf(wave_sum(s2) / (float)d + 1e-5f);
#pragma unroll
      for (int e = 0; e < 16; ++e) { const int c = lane + 64 * e; if (c < d) s_act[g * kActStride + c] = (xv[e] - mean) * rstd * p.ln_w[c] + p.ln_b[c]; }
    }
    __syncthreads();
    // 4 lanes share a weight row, lane j takes the 16-byte chunks j, j + 4, ...; every chunk meets all G rows
    const int qrow = tid >> 2, qj = tid & 3;
    const h16* wr = p.wq + (long)(head * 64 + qrow) * d;
    const int nch = d >> 3;
    float acc[kGroupMax];
#pragma unroll
    for (int g = 0; g < kGroupMax; ++g) acc[g] = 0.f;
    u32x4 wc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int c = qj + 4 * i; wc[i] = c < nch ? *reinterpret_cast<const u32x4*>(wr + c * 8) : u32x4{0u, 0u, 0u, 0u}; }
    for (int c0 = 0; c0 < nch; c0 += 16) {
      u32x4 cur[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) cur[i] = wc[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int c = c0 + 16 + qj + 4 * i; wc[i] = c < nch ? *reinterpret_cast<const u32x4*>(wr + c * 8) : u32x4{0u, 0u, 0u, 0u}; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c0 + qj + 4 * i;
        if (c < nch) {
          const float w8[8] = {h16lo(cur[i][0]), h16hi(cur[i][0]), h16lo(cur[i][1]), h16hi(cur[i][1]),
                               h16lo(cur[i][2]), h16hi(cur[i][2]), h16lo(cur[i][3]), h16hi(cur[i][3])};
#pragma unroll
          for (int g = 0; g < kGroupMax; ++g) {
            if (g < G) {
              const float4 y0 = *reinterpret_cast<const float4*>(s_act + g * kActStride + c * 8), y1 = *reinterpret_cast<const float4*>(s_act + g * kActStride + c * 8 + 4);
              float a0 = fmaf(w8[0], y0.x, acc[g]), a1 = w8[1] * y0.y;
              a0 = fmaf(w8[2], y0.z, a0); a1 = fmaf(w8[3], y0.w, a1);
              a0 = fmaf(w8[4], y1.x, a0); a1 = fmaf(w8[5], y1.y, a1);
              a0 = fmaf(w8[6], y1.z, a0); a1 = fmaf(w8[7], y1.w, a1);
              acc[g] = a0 + a1;
            }
          }
        }
      }
    }
    const float bq = p.bq[head * 64 + qrow];
#pragma unroll
    for (int g = 0; g < kGroupMax; ++g) {
      const float qv = quad_sum(acc[g]) + bq;
      if (qj == 0) s_q[g * 64 + qrow] = g < G ? qv : 0.f;
    }
  } else if constexpr (QM == 2) {
    const int d = p.d_model, nst = d >> 4;  // nst <= 64
    for (int g = wave; g < kGroupMax; g += 4) {  // one wave per rank: lane = dimension, and one block statistic each
      float qv = 0.f;
      if (g < G) {
        const auto fq = attn::folded_query_request(p.tq, p.stat_part, p.fold_s, p.fold_c, rel0 + g, head, lane, d, nst);
        qv = attn::folded_query_value(fq, lane, d, nst);
      }
      s_q[g * 64 + lane] = qv;
    }
  } else {
    for (int g = wave; g < kGroupMax; g += 4) s_q[g * 64 + lane] = g < G ? p.q[(long)(rel0 + g) * p.d_model + head * 64 + lane] : 0.f;
  }
  __syncthreads();  // the fp32 queries are whole; nobody reads a LayerNormed row any more
  {
    // the K scales into the query (file header): one wave per rank, lane = dimension. A non-finite query value takes no part in the
    // shift and stays non-finite in the image, so it reaches the result as it does in the h16 kernels
    const int e_d = (int)(__float_as_uint(sc_head[layout::kKv8ScaleK * layout::kKvDim + lane]) >> 23) - 127;  // the scale is 2^e_d, normal
    for (int g = wave; g < kGroupMax; g += 4) {
      const float x = s_q[g * 64 + lane];
      const float top = wave_max(x != 0.f && isfinite(x) && g < G ? (float)(ilogbf(x) + e_d) : -1024.f);
      const int shift = top > -1024.f ? (int)top - 14 : 0;
      put_pair(s_qa, g, qa_col(lane), g < G ? ldexpf(x, e_d - shift) : 0.f);
      if (lane == 0) s_shift[g] = shift - 3;  // (with the 1 / 8 = (64^-0.25)^2 of the scores, export_onnx.py:116,124-126)
    }
  }
  __syncthreads();  // the query image is whole; the fp32 queries in s_p are dead
  const h16x8 qa0 = a_frag(s_qa, 0, lane), qa1 = a_frag(s_qa, 1, lane);
  const float vsc = sc_head[layout::kKv8ScaleV * layout::kKvDim + lane];  // of output dimension `lane`

  // ---- the key blocks of this wave
  h16* tile = s_v + wave * layout::kKvBlockElems;
  h16* pimg = s_p + wave * kAImage;
  const int vbase = layout::cross_v_read_base(lane, true);
  const int q4 = lane >> 4, col = lane & 15;
  const int sh[2] = {s_shift[2 * q4], s_shift[2 * q4 + 1]};
  float m_r[2] = {-INFINITY, -INFINITY}, l_r[2] = {0.f, 0.f};  // ranks 2 q4, 2 q4 + 1
  f32x4 o[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (; blk < blk_end; blk += 4) {
    const bool more = blk + 4 < blk_end;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<h16x8*>(tile + layout::cross_v_index(8 * i + (lane >> 3), (lane & 7) * 8, true)) = codes_to_h16(vn[i][0], vn[i][1]);
    if (more) load_v(blk + 4);
    f32x4 sc[4];
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      sc[kq] = AXW_MFMA_16x16x32(qa0, codes_to_h16(kn[kq][0], kn[kq][1]), (f32x4{0.f, 0.f, 0.f, 0.f}));
      sc[kq] = AXW_MFMA_16x16x32(qa1, codes_to_h16(kn[kq][2], kn[kq][3]), sc[kq]);
    }
    if (more) load_k(blk + 4);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float s[4], mx = -INFINITY;
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        s[kq] = ldexpf(sc[kq][2 * e] + sc[kq][2 * e + 1], sh[e]);
        if (blk * 64 + 16 * kq + col >= p.n_keys) s[kq] = -INFINITY;
        mx = fmaxf(mx, s[kq]);
      }
      const float m_new = fmaxf(m_r[e], row16_max(mx));  // (a block that is loaded has a key below n_keys)
      const float alpha = __expf(m_r[e] - m_new);
      m_r[e] = m_new;
      float l = l_r[e] * alpha;
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        const float pk = __expf(s[kq] - m_new);
        l += pk;
        put_pair(pimg, 2 * q4 + e, 16 * kq + col, pk);
      }
      l_r[e] = l;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) { o[nb][2 * e] *= alpha; o[nb][2 * e + 1] *= alpha; }
    }
    __builtin_amdgcn_wave_barrier();  // the wave's own LDS writes (tile, probabilities) precede its reads
    const h16x8 pa0 = a_frag(pimg, 0, lane), pa1 = a_frag(pimg, 1, lane);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      o[nb] = AXW_MFMA_16x16x32(pa0, v_frag(tile, vbase, nb, 0), o[nb]);
      o[nb] = AXW_MFMA_16x16x32(pa1, v_frag(tile, vbase, nb, 1), o[nb]);
    }
    __builtin_amdgcn_wave_barrier();  // ... and its reads the next block's writes
  }

  // ---- the wave's record per rank, into its own tile; then the four waves' records of a rank are merged by one wave
  float* wrec = reinterpret_cast<float*>(tile);
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    float* rec = wrec + (2 * q4 + e) * kPartStride;
    const float l = row16_sum(l_r[e]);
    if (col == 0) { rec[kPartM] = m_r[e]; rec[kPartL] = l; }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) rec[kPartO + 16 * nb + col] = o[nb][2 * e] + o[nb][2 * e + 1];
  }
  __syncthreads();
  const float* recs = reinterpret_cast<const float*>(s_v);
  constexpr int kWaveRec = layout::kKvBlockElems / 2;  // floats between the waves' records
  float m[2], l[2], ov[2];  // this thread's ranks wave and wave + 4, dimension `lane`
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int g = wave + 4 * j;
    m[j] = -INFINITY; l[j] = 0.f; ov[j] = 0.f;
    if (g < G) attn::merge_wave_records(recs + g * kPartStride, kWaveRec, lane, m[j], l[j], ov[j]);
  }
  // (the V scale behind the final 1 / l: exact)
  auto write_out = [&](int g, float y) { attn::store_out_pair(p.out_hi, p.out_lo, rel0 + g, head * 64 + lane, p.nbs, y * vsc); };
  if (p.n_split == 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int g = wave + 4 * j; if (g < G && (live >> g & 1)) write_out(g, ov[j] / l[j]); }
    return;
  }
  // Splits (decode_attention_common.hpp), as in decode_attention_group.hip: every wave publishes its ranks' records and drains them;
  // behind a barrier ONE lane draws the workgroup's ticket; whoever draws the last one folds every rank's records.
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int g = wave + 4 * j;
    if (!(g < G && (live >> g & 1))) continue;
    float* mine = p.mpart + layout::part_offset(rel0 + g, head, split, p.n_head, p.n_split);
    attn::publish_split_record(mine, lane, m[j], l[j], ov[j]);
  }
  attn::drain_split_stores();
  __syncthreads();
  unsigned* cnt = p.mcnt + (long)rel0 * p.n_head + head;
  const unsigned ticket = attn::draw_split_ticket(cnt, tid == 0);
  if (tid == 0) s_ticket = ticket;
  __syncthreads();
  if (s_ticket != (unsigned)p.n_split - 1u) return;
  if (tid == 0) attn::reset_split_counter(cnt);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int g = wave + 4 * j;
    if (!(g < G && (live >> g & 1))) continue;
    const float* base = p.mpart + layout::part_offset(rel0 + g, head, 0, p.n_head, p.n_split);
    write_out(g, attn::fold_split_records(base, split, p.n_split, lane, m[j], l[j], ov[j]));
  }
}

}  // namespace

void launch_decode_cross_attention_group_fp8(const DecAttnGroupFp8Params& p, hipStream_t s) {
  if (!(p.k8 && p.v8 && p.scales && p.group >= 1 && p.group <= kGroupMax && p.nslots >= 1 && p.slot0 >= 0 && p.slot0 % 16 == 0 && p.n_head >= 1 &&
        p.d_model == p.n_head * layout::kKvDim && p.cap_blocks >= 1 && p.n_keys >= 1 && p.n_keys <= p.cap_blocks * layout::kKvBlockKeys &&
        p.out_hi && p.out_lo)) {
    fprintf(stderr, "[ax_whisper] grouped fp8 cross-attention: group %d, slots %d + %d, d_model %d, n_head %d, n_keys %d unsupported\n",
            p.group, p.slot0, p.nslots, p.d_model, p.n_head, p.n_keys);
    abort();
  }
  const AttnQueryPlan plan = plan_attention_query(p, p, "grouped fp8 cross-attention");
  const dim3 grid(p.n_split, p.n_head, cross_group_clips(p.slot0, p.nslots, p.group));
  if (plan.mode == 2) hipLaunchKernelGGL((decode_cross_attention_group_fp8_kernel<2>), grid, dim3(256), 0, s, p);
  else if (plan.mode == 1) hipLaunchKernelGGL((decode_cross_attention_group_fp8_kernel<1>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((decode_cross_attention_group_fp8_kernel<0>), grid, dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
