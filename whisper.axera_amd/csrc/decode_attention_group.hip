// decode_attention_group.hip — grouped single-query cross-attention for beam search on gfx950 (DESIGN.md "Beam search",
// "Shared cross K/V").
//
// The K hypotheses ("ranks") of a clip sit in the slots [c K, c K + K) and all attend over the same 1500 encoder keys. The
// launch-per-phase step gives every slot its own copy of them (beam_spread_cross_kernel) and decode_attention_kernel streams each
// copy: K times the bytes. Here ONE workgroup per (key split, head, clip) streams the clip's own K/V, slot c's, once, and serves
// all ranks of the clip that lie inside the launch's slot range.
//
// Work split. 256 threads = 4 waves; wave w takes the 64-key blocks blk_begin + w, + 4, ... of the split, as
// decode_attention_kernel does. G <= 8 ranks x the (hi, lo) h16 split of an fp32 row are at most 16 rows: the A operand of
// v_mfma_f32_16x16x32 (rank g's hi half on row 2 g, its lo half on row 2 g + 1; rows from 2 G on are zero). A 64-key block is
// 8 MFMAs for the scores and 8 for the output, whatever G is.
//   scores   S[row][key] = sum_d A[row][d] K[key][d]. B piece (16-key block kb, k-step ks): lane l holds key 16 kb + l % 16, dims
//            32 ks + 8 (l / 16) .. + 7, which is the 16-byte piece kv_chunk_offset(blk, 4 ks + l / 16, 16 kb + l % 16) of the blocked
//            K: loaded straight from global memory into the operand registers (non-temporal buffer loads), never through LDS.
//            Result register i of lane l is row 4 (l / 16) + i, key 16 kb + l % 16: lane group q = l / 16 owns the ranks 2 q
//            (registers 0 + 1 = hi + lo) and 2 q + 1 (registers 2 + 3).
//   softmax  fp32, online: every lane keeps (max, sum) of its two ranks; the block maximum of a rank is a DPP reduction over the 16
//            lanes of its group, the sums stay per lane until the end.
//   output   O[row][dim] = sum_key P[row][key] V[key][dim]. The probabilities go through a wave-private LDS image [16 rows][64 keys]
//            (hi, lo) to become the A operand (rows of 72 elements: the four lane groups write four different bank groups). V is
//            row-major in memory and the B operand wants keys along k: the wave's V tile goes registers -> LDS in the image of
//            layout::cross_v_swizzle (16-byte chunks permuted inside every 128-byte row) and is read with ds_read_b64_tr_b16 at
//            layout::cross_v_read_offset, the conflict-free form of the persistent launches' cross tiles, kept as it is.
//            The result has the row layout of the scores, so a lane rescales its own two ranks' registers.
// One register set per operand (K 32 + V 32 VGPRs): the next block's V is requested as soon as the tile is in LDS, the next
// block's K as soon as the scores are formed; both land under the rest of the block.
// Keys at or beyond n_keys are never loaded (decode_attention_kernel's clamp rule: such a lane reads the last valid key of the
// block again, and its score is set to -inf / its V row meets probability 0).
//
// Query modes (QM), per rank: 0 from p.q; 1 the fused projection q = Wq[head rows] . LayerNorm(x[slot]) + bq, where a weight chunk
// is loaded once and multiplied with all G LayerNormed rows (they sit in the LDS of the V tiles, which are not in use yet);
// 2 the folded query r (T - mu s) + c.
// Behind the key loop: per rank the split record (m, l, o[64]), the ticket hand-off (one ticket per workgroup: the group's splits
// all serve the same ranks) and the last arriver's fold in split order, then the fragment-major (hi, lo) output pair — the shared
// pieces of decode_attention_common.hpp. A rank whose done flag is set gets no record and no output; a group whose ranks are all done returns
// before any K/V request (done_late == 0) or right behind the first ones (done_late == 1).
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

// base: wave-uniform pointer of this (clip, head)'s K or V, off: element offset of this lane (decoder.hip ld_kv)
__device__ __forceinline__ u32x4 ld_kv_nt(const h16* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x27000);
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off * 2, 0, 2);  // aux 2 = nt
}
template <int QM>
__global__ __launch_bounds__(256) void decode_cross_attention_group_kernel(DecAttnGroupParams p) {
  // the waves' V tiles [4][64 keys][64 dims]; in front of the key loop the fused mode's LayerNormed rows [G][1024] fp32, behind it the
  // waves' records [4][8 ranks][66] fp32 (each wave's inside its own tile)
  __shared__ __attribute__((aligned(16))) h16 s_v[4 * layout::kKvBlockElems];
  __shared__ __attribute__((aligned(16))) h16 s_p[4 * kAImage];
  __shared__ __attribute__((aligned(16))) h16 s_qa[kAImage];
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
  const long head_elems = layout::kv_head_elems(p.cap_blocks * layout::kKvBlockKeys);
  const h16* kb = p.k + (long)clip * p.kv_slot_stride + head * head_elems;
  const h16* vb = p.v + (long)clip * p.kv_slot_stride + head * head_elems;

  u32x4 kn[8], vn[8];  // kn[2 kb + ks]: the B pieces of the scores; vn[i]: rows 8 i + lane / 8 of the V tile, chunk lane % 8
  auto load_k = [&](int bk) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = max(0, min(16 * (i >> 1) + (lane & 15), p.n_keys - 1 - bk * 64));
      kn[i] = ld_kv_nt(kb, layout::kv_chunk_offset(bk, 4 * (i & 1) + (lane >> 4), key));
    }
  };
  auto load_v = [&](int bk) {
#pragma unroll
    for (int i = 0; i < 8; ++i) vn[i] = ld_kv_nt(vb, layout::v_index(min(bk * 64 + 8 * i + (lane >> 3), p.n_keys - 1), (lane & 7) * 8));
  };
  int blk = blk_begin + wave;
  if (blk < blk_end) { load_k(blk); load_v(blk); }
  if (!live) return;  // (done_late: behind the first requests)

  // ---- the ranks' queries -> s_qa
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
      if (qj == 0) put_pair(s_qa, g, qrow, g < G ? qv : 0.f);
    }
  } else if constexpr (QM == 2) {
    const int d = p.d_model, nst = d >> 4;  // nst <= 64
    for (int g = wave; g < kGroupMax; g += 4) {  // one wave per rank: lane = dimension, and one block statistic each
      float qv = 0.f;
      if (g < G) {
        const auto fq = attn::folded_query_request(p.tq, p.stat_part, p.fold_s, p.fold_c, rel0 + g, head, lane, d, nst);
        qv = attn::folded_query_value(fq, lane, d, nst);
      }
      put_pair(s_qa, g, lane, qv);
    }
  } else {
    for (int g = wave; g < kGroupMax; g += 4) put_pair(s_qa, g, lane, g < G ? p.q[(long)(rel0 + g) * p.d_model + head * 64 + lane] : 0.f);
  }
  __syncthreads();  // the query image is whole; nobody reads a LayerNormed row any more
  const h16x8 qa0 = a_frag(s_qa, 0, lane), qa1 = a_frag(s_qa, 1, lane);

  // ---- the key blocks of this wave
  h16* tile = s_v + wave * layout::kKvBlockElems;
  h16* pimg = s_p + wave * kAImage;
  const int vbase = layout::cross_v_read_base(lane, true);
  const int q4 = lane >> 4, col = lane & 15;
  float m_r[2] = {-INFINITY, -INFINITY}, l_r[2] = {0.f, 0.f};  // ranks 2 q4, 2 q4 + 1
  f32x4 o[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (; blk < blk_end; blk += 4) {
    const bool more = blk + 4 < blk_end;
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<u32x4*>(tile + layout::cross_v_index(8 * i + (lane >> 3), (lane & 7) * 8, true)) = vn[i];
    if (more) load_v(blk + 4);
    f32x4 sc[4];
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      sc[kq] = AXW_MFMA_16x16x32(qa0, __builtin_bit_cast(h16x8, kn[2 * kq]), (f32x4{0.f, 0.f, 0.f, 0.f}));
      sc[kq] = AXW_MFMA_16x16x32(qa1, __builtin_bit_cast(h16x8, kn[2 * kq + 1]), sc[kq]);
    }
    if (more) load_k(blk + 4);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float s[4], mx = -INFINITY;
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        s[kq] = (sc[kq][2 * e] + sc[kq][2 * e + 1]) * 0.125f;  // (64^-0.25)^2, export_onnx.py:116,124-126
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
  auto write_out = [&](int g, float y) { attn::store_out_pair(p.out_hi, p.out_lo, rel0 + g, head * 64 + lane, p.nbs, y); };
  if (p.n_split == 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int g = wave + 4 * j; if (g < G && (live >> g & 1)) write_out(g, ov[j] / l[j]); }
    return;
  }
  // Splits (decode_attention_common.hpp): every wave publishes its ranks' records and drains them; behind a barrier ONE lane draws
  // the workgroup's ticket (the group's splits all serve the same ranks); whoever draws the last one folds every rank's records.
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

void launch_decode_cross_attention_group(const DecAttnGroupParams& p, hipStream_t s) {
  if (!(p.group >= 1 && p.group <= kGroupMax && p.nslots >= 1 && p.slot0 >= 0 && p.slot0 % 16 == 0 && p.n_head >= 1 &&
        p.d_model == p.n_head * layout::kKvDim && p.cap_blocks >= 1 && p.n_keys >= 1 && p.n_keys <= p.cap_blocks * layout::kKvBlockKeys &&
        p.out_hi && p.out_lo)) {
    fprintf(stderr, "[ax_whisper] grouped cross-attention: group %d, slots %d + %d, d_model %d, n_head %d, n_keys %d unsupported\n",
            p.group, p.slot0, p.nslots, p.d_model, p.n_head, p.n_keys);
    abort();
  }
  const AttnQueryPlan plan = plan_attention_query(p, p, "grouped cross-attention");
  const dim3 grid(p.n_split, p.n_head, cross_group_clips(p.slot0, p.nslots, p.group));
  if (plan.mode == 2) hipLaunchKernelGGL((decode_cross_attention_group_kernel<2>), grid, dim3(256), 0, s, p);
  else if (plan.mode == 1) hipLaunchKernelGGL((decode_cross_attention_group_kernel<1>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((decode_cross_attention_group_kernel<0>), grid, dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
