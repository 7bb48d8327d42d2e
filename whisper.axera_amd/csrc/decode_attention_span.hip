// decode_attention_span.hip — opt-in cross-attention over each slot's own audio span (AX_WHISPER_CROSS_SPAN=audio).
//
// The batched step's cross-attention launches stream all 1500 encoder frames of every slot, whatever the clip's length: one key count
// per launch, the key splits chosen by the clip count. Here every slot has a span (engine: min(n_audio_ctx, ceil(samples / 320) +
// margin) frames) and the launch is a WORK LIST:
//
//   cross_span_plan_kernel                 the spans of a launch's slots -> items (slot, head, first block, block count, piece,
//                                          pieces, key count). A (slot, head) is cut into pieces of about total_blocks /
//                                          target_workgroups blocks, so a 1500-frame clip beside 300-frame clips becomes more
//                                          pieces instead of setting the pace of the launch. One workgroup per slot range, one
//                                          ordered prefix sum: the list does not depend on any arrival order. Rebuilt when spans
//                                          change (a call, an admission pass), never per step, and outside the captured step graph.
//   decode_cross_attention_span_kernel     one item per workgroup, read from device memory (a graph replay stays valid after a
//                                          refill); surplus workgroups exit on the item count. Wave w takes blocks first + w,
//                                          first + w + 4, ... of the piece; the tail of the span's last block is masked and no block
//                                          beyond the span is ever requested. The four waves' records merge through LDS, the pieces
//                                          of a (slot, head) through the write-through records and the ticket of
//                                          decode_attention_common.hpp, folded in piece order by the last arriver.
//                                          FP8 = false: blocked K / row-major V h16 images; FP8 = true: the e4m3fn code images and
//                                          their power-of-two scales (decode_layout.hpp). QM 0: the query from a buffer, QM 1: the
//                                          fused projection.
#include "common.hpp"
#include "decode_attention_common.hpp"

namespace axw {
inline namespace AXW_NS {

using layout::kPartStride;
using layout::kAttnSplitMax;
using layout::kPartM;
using layout::kPartL;
using layout::kPartO;
using layout::kKvBlockKeys;

// ------------------------------------------------------------------------------- plan
// One workgroup per slot range r: [b0[r], b0[r] + nb[r]). Slot indices in the items are relative to b0[r] (the origin of the
// launch's query, output, record and ticket pointers). List of range r: items + b0[r] * n_head * kAttnSplitMax, count: counts[b0[r] / 16].
__global__ __launch_bounds__(256) void cross_span_plan_kernel(CrossSpanPlanParams p) {
  __shared__ int s_red[256];
  __shared__ int s_base;
  const int tid = threadIdx.x, r = blockIdx.x;
  const int b0 = p.b0[r], nb = p.nb[r], H = p.n_head;
  const int max_blocks = (p.n_keys + kKvBlockKeys - 1) / kKvBlockKeys;
  auto keys_of = [&](int b) { return max(1, min(p.spans[b0 + b], p.n_keys)); };
  auto blocks_of = [&](int b) { return min(max_blocks, (keys_of(b) + kKvBlockKeys - 1) / kKvBlockKeys); };
  // blocks of the range (per head)
  int mine = 0;
  for (int b = tid; b < nb; b += 256) mine += blocks_of(b);
  s_red[tid] = mine;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {  // (integers: any order gives the same sum)
    if (tid < st) s_red[tid] += s_red[tid + st];
    __syncthreads();
  }
  const long total = (long)s_red[0] * H;
  __syncthreads();
  const int per = max(p.min_blocks, (int)((total + p.target[r] - 1) / max(1, p.target[r])));
  auto pieces_of = [&](int nblk) {
    const int want = min(p.max_pieces, (nblk + per - 1) / per);
    const int bpp = (nblk + want - 1) / want;  // blocks per piece
    return (nblk + bpp - 1) / bpp;             // every piece holds at least one block
  };
  CrossSpanItem* items = p.items + (long)b0 * H * kAttnSplitMax;
  if (tid == 0) s_base = 0;
  __syncthreads();
  // slots in chunks of 256, in slot order: an inclusive scan of the chunk's item counts, then every thread writes its slot's items
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int b = c0 + tid;
    const int nblk = b < nb ? blocks_of(b) : 0;
    const int np = b < nb ? pieces_of(nblk) : 0;
    s_red[tid] = np * H;
    __syncthreads();
    for (int st = 1; st < 256; st <<= 1) {
      const int v = tid >= st ? s_red[tid - st] : 0;
      __syncthreads();
      s_red[tid] += v;
      __syncthreads();
    }
    int at = s_base + s_red[tid] - np * H;
    if (b < nb) {
      const int bpp = (nblk + np - 1) / np, keys = keys_of(b);
      for (int h = 0; h < H; ++h)
        for (int pc = 0; pc < np; ++pc) {
          const int first = pc * bpp, cnt = min(bpp, nblk - first);
          items[at++] = CrossSpanItem{b | (h << 16), first | (cnt << 16), pc | (np << 16), keys};
        }
    }
    __syncthreads();
    if (tid == 255) s_base += s_red[255];
    __syncthreads();
  }
  if (tid == 0) p.counts[b0 >> 4] = s_base;
}

void launch_cross_span_plan(const CrossSpanPlanParams& p, hipStream_t s) {
  bool ok = p.spans && p.items && p.counts && p.n_keys >= 1 && p.n_head >= 1 && p.n_ranges >= 1 && p.n_ranges <= kSpanMaxRanges &&
            p.max_pieces >= 1 && p.max_pieces <= kAttnSplitMax && p.min_blocks >= 1;
  for (int r = 0; ok && r < p.n_ranges; ++r) ok = p.b0[r] >= 0 && p.b0[r] % 16 == 0 && p.nb[r] >= 1 && p.nb[r] < 65536 && p.target[r] >= 1;
  if (!ok) { fprintf(stderr, "[ax_whisper] cross-span plan: %d ranges, %d keys, %d pieces unsupported\n", p.n_ranges, p.n_keys, p.max_pieces); abort(); }
  hipLaunchKernelGGL(cross_span_plan_kernel, dim3(p.n_ranges), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------- attention
// 16-byte non-temporal buffer loads of a K/V image (the bytes are read once per step); off in bytes
__device__ __forceinline__ u32x4 ld_span(const void* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x27000);
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 2);  // aux 2 = nt
}

// Registers of one 64-key block in flight per wave.
//   h16: K 8 x 16 bytes (lane = key, chunk i = dims 8 i ..), V 8 x 16 bytes (row 8 i + lane / 8, dims 8 (lane % 8) ..): a lane
//        accumulates 8 output dimensions
//   FP8: K 4 x 16 bytes (lane = key, chunk i = dims 16 i ..), V 4 x 16 bytes (row 16 i + lane / 4, dims 16 (lane % 4) ..): a lane
//        accumulates 16 output dimensions; the K scales are in the query, the V scales multiply the output after the final 1 / l
// Lanes whose key is at or beyond the key count read the block's last valid key / row (the lines their neighbours read; no predicate
// around the loads): bytes beyond the span are never requested, so nothing there — a NaN code included — reaches a result.
template <bool FP8, int QM, int NCHL>
__global__ __launch_bounds__(256) void decode_cross_attention_span_kernel(DecAttnSpanParams p) {
  constexpr int NL = FP8 ? 4 : 8;     // 16-byte loads per operand and block
  constexpr int ND = FP8 ? 16 : 8;    // output dimensions per lane
  typedef float f2 __attribute__((ext_vector_type(2)));
  __shared__ float s_part[4][kPartStride];
  __shared__ float s_q[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if ((int)blockIdx.x >= *p.count) return;  // surplus workgroup
  const CrossSpanItem it = p.items[blockIdx.x];
  const int slot = it.slot_head & 0xffff, head = it.slot_head >> 16;
  if (slot >= p.batch || head >= p.n_head) return;  // (never: the plan kernel writes slots and heads of its own range)
  const int clip_done = p.done[slot];
  if (!p.done_late && clip_done) return;
  const int cap_blocks = p.cap_blocks;
  const int n_keys = max(1, min(it.n_keys, cap_blocks * kKvBlockKeys));
  const int blk_begin = it.blocks & 0xffff;
  const int blk_end = min(blk_begin + (it.blocks >> 16), (n_keys + kKvBlockKeys - 1) / kKvBlockKeys);

  const char* kb;
  const char* vb;
  if constexpr (FP8) {
    kb = reinterpret_cast<const char*>(p.k8) + (long)slot * p.kv_slot_bytes + head * layout::kv8_head_bytes(cap_blocks * kKvBlockKeys);
    vb = reinterpret_cast<const char*>(p.v8) + (long)slot * p.kv_slot_bytes + head * layout::kv8_head_bytes(cap_blocks * kKvBlockKeys);
  } else {
    kb = reinterpret_cast<const char*>(p.k + (long)slot * p.kv_slot_stride + head * layout::kv_head_elems(cap_blocks * kKvBlockKeys));
    vb = reinterpret_cast<const char*>(p.v + (long)slot * p.kv_slot_stride + head * layout::kv_head_elems(cap_blocks * kKvBlockKeys));
  }
  u32x4 kn[NL], vn[NL];
  auto load_k = [&](int bk) {
    const int lk = max(0, min(lane, n_keys - 1 - bk * kKvBlockKeys));
#pragma unroll
    for (int i = 0; i < NL; ++i) kn[i] = ld_span(kb, FP8 ? layout::k8_chunk_offset(bk, i, lk) : 2 * layout::kv_chunk_offset(bk, i, lk));
  };
  auto load_v = [&](int bk) {
    const int last = max(bk * kKvBlockKeys, n_keys - 1);
#pragma unroll
    for (int i = 0; i < NL; ++i)
      vn[i] = ld_span(vb, FP8 ? layout::v8_index(min(bk * kKvBlockKeys + 16 * i + (lane >> 2), last), (lane & 3) * 16)
                              : 2 * layout::v_index(min(bk * kKvBlockKeys + 8 * i + (lane >> 3), last), (lane & 7) * 8));
  };
  int blk = blk_begin + wave;
  if (blk < blk_end) { load_k(blk); load_v(blk); }  // in flight under the query prologue

  // the head's 64 query values (times the K scales over the code images) through s_q
  const float* sc_head = nullptr;
  if constexpr (FP8) sc_head = p.scales + (long)slot * p.scale_slot_stride + head * layout::kKv8ScaleHead;
  if constexpr (QM == 1) {
    __shared__ __attribute__((aligned(16))) float s_act[1024];
    __shared__ float s_red[8];
    const int d = p.d_model;  // <= 1024, multiple of 32
    auto fq = attn::fused_query_request<NCHL>(p.x, p.ln_w, p.ln_b, p.wq, p.bq, slot, head, d, tid);
    float ksc = 1.f;
    if constexpr (FP8) ksc = sc_head[tid >> 2];
    if (clip_done) return;  // (workgroup-uniform, in front of the first barrier)
    const float qx = attn::fused_query_finish(fq, s_act, s_red, d, tid, lane, wave, [] {});
    if ((tid & 3) == 0) s_q[tid >> 2] = qx * ksc;
  } else {
    float qx = 0.f, ksc = 1.f;
    if (wave == 0) {
      qx = p.q[(long)slot * p.d_model + head * 64 + lane];
      if constexpr (FP8) ksc = sc_head[lane];
    }
    if (clip_done) return;  // (workgroup-uniform, in front of the barrier)
    if (wave == 0) s_q[lane] = qx * ksc;
  }
  __syncthreads();
  float qv[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) qv[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_q[c])));

  // The item's coordinates cross the block loop in vector registers: the scalar file holds the 64 query values, the two buffer
  // descriptors and the loop's own state, and what does not fit the allocator spills (the generic projection's instantiations did).
  int v_slot = slot, v_head = head, v_piece = it.piece;
  asm volatile("" : "+v"(v_slot), "+v"(v_head), "+v"(v_piece));

  float m_w = -INFINITY, l_lane = 0.f;
  float o[ND];
#pragma unroll
  for (int e = 0; e < ND; ++e) o[e] = 0.f;

  // One register set per operand: the next block's K is requested once this block's scores are formed (it lands under the softmax
  // and the P.V arithmetic), the next V right after P.V.
  auto one_block = [&](int cur, bool prefetch) {
    float sc;
    if constexpr (FP8) {
      f2 s = {0.f, 0.f};  // even and odd dimensions
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)kn[i][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)kn[i][w], true);
          s = __builtin_elementwise_fma(f2{qv[16 * i + 4 * w], qv[16 * i + 4 * w + 1]}, lo, s);
          s = __builtin_elementwise_fma(f2{qv[16 * i + 4 * w + 2], qv[16 * i + 4 * w + 3]}, hi, s);
        }
      sc = s[0] + s[1];
    } else {
      sc = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sc = fmaf(qv[i * 8 + 2 * e], h16lo(kn[i][e]), sc);
          sc = fmaf(qv[i * 8 + 2 * e + 1], h16hi(kn[i][e]), sc);
        }
    }
    if (prefetch) load_k(cur + 4);
    sc *= 0.125f;  // (64^-0.25)^2
    if (cur * kKvBlockKeys + lane >= n_keys) sc = -INFINITY;  // the tail of the span's last block
    const float m_new = fmaxf(m_w, wave_max(sc));  // finite: a block that is loaded holds a key below n_keys
    const float alpha = __expf(m_w - m_new);
    const float pk = __expf(sc - m_new);
    m_w = m_new;
    l_lane = l_lane * alpha + pk;
#pragma unroll
    for (int e = 0; e < ND; ++e) o[e] *= alpha;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      if constexpr (FP8) {
        const float w = __shfl(pk, 16 * i + (lane >> 2), 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vn[i][u], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vn[i][u], true);
          o[4 * u] = fmaf(w, lo[0], o[4 * u]);
          o[4 * u + 1] = fmaf(w, lo[1], o[4 * u + 1]);
          o[4 * u + 2] = fmaf(w, hi[0], o[4 * u + 2]);
          o[4 * u + 3] = fmaf(w, hi[1], o[4 * u + 3]);
        }
      } else {
        const float w = __shfl(pk, 8 * i + (lane >> 3), 64);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[2 * e] = fmaf(w, h16lo(vn[i][e]), o[2 * e]);
          o[2 * e + 1] = fmaf(w, h16hi(vn[i][e]), o[2 * e + 1]);
        }
      }
    }
    if (prefetch) load_v(cur + 4);
  };
  for (; blk < blk_end; blk += 4) one_block(blk, blk + 4 < blk_end);

  const int t_slot = __builtin_amdgcn_readfirstlane(v_slot), t_head = __builtin_amdgcn_readfirstlane(v_head);
  const int t_piece = __builtin_amdgcn_readfirstlane(v_piece) & 0xffff, t_pieces = min(__builtin_amdgcn_readfirstlane(v_piece) >> 16, kAttnSplitMax);
  // wave record: o summed over the key sub-rows (lanes with equal lane % (64 / ND)), l over the wave
  const float l_w = wave_sum(l_lane);
#pragma unroll
  for (int e = 0; e < ND; ++e) {
    if constexpr (FP8) o[e] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(o[e]), 0x124, 0xf, 0xf, true));  // row_ror:4
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
  if (lane < 64 / ND) {
#pragma unroll
    for (int e = 0; e < ND; ++e) s_part[wave][kPartO + lane * ND + e] = o[e];
  }
  __syncthreads();
  if (tid < 64) {
    float m, l, ov, y;
    attn::merge_wave_records(&s_part[0][0], kPartStride, tid, m, l, ov);
    float vsc = 1.f;
    if constexpr (FP8) vsc = (p.scales + (long)t_slot * p.scale_slot_stride + t_head * layout::kKv8ScaleHead)[layout::kKvDim + tid];
    if (t_pieces > 1) {  // the pieces of a (slot, head) meet in this launch: the last one to arrive writes the output
      float* base = p.mpart + layout::part_offset(t_slot, t_head, 0, p.n_head, kAttnSplitMax);
      unsigned* cnt = p.mcnt + t_slot * p.n_head + t_head;
      if (!attn::split_publish_and_fold(base, cnt, t_piece, t_pieces, tid, m, l, ov, y, [](int) {})) return;
    } else {
      y = ov / l;
    }
    attn::store_out_pair(p.out_hi, p.out_lo, t_slot, t_head * 64 + tid, p.nbs, y * vsc);
  }
}

void launch_decode_cross_attention_span(const DecAttnSpanParams& p, hipStream_t s) {
  const bool fp8 = p.k8 != nullptr;
  const bool kv_ok = fp8 ? (p.v8 && p.scales) : (p.k && p.v);
  if (!kv_ok || !p.items || !p.count || !p.done || !p.out_hi || !p.out_lo || !p.mpart || !p.mcnt || p.batch < 1 || p.batch >= 65536 ||
      p.n_head < 1 || p.cap_blocks < 1 || p.grid < 1 || p.tq) {
    fprintf(stderr, "[ax_whisper] span cross-attention: %d slots, %d heads, %d blocks, %d workgroups unsupported\n", p.batch, p.n_head, p.cap_blocks, p.grid);
    abort();
  }
  const dim3 grid(p.grid);
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p); };
  if (p.wq) {  // fused query projection
    if (p.d_model > 1024 || p.d_model % 32 != 0 || !p.x || !p.ln_w || !p.ln_b || !p.bq) {
      fprintf(stderr, "[ax_whisper] span cross-attention, fused query projection: d_model %d unsupported\n", p.d_model); abort();
    }
    const int nchl = (p.d_model == 384 || p.d_model == 512 || p.d_model == 768 || p.d_model == 1024) ? p.d_model / 32 : 0;
    if (fp8) {
      if (nchl == 12) go(decode_cross_attention_span_kernel<true, 1, 12>);
      else if (nchl == 16) go(decode_cross_attention_span_kernel<true, 1, 16>);
      else if (nchl == 24) go(decode_cross_attention_span_kernel<true, 1, 24>);
      else if (nchl == 32) go(decode_cross_attention_span_kernel<true, 1, 32>);
      else go(decode_cross_attention_span_kernel<true, 1, 0>);
    } else {
      if (nchl == 12) go(decode_cross_attention_span_kernel<false, 1, 12>);
      else if (nchl == 16) go(decode_cross_attention_span_kernel<false, 1, 16>);
      else if (nchl == 24) go(decode_cross_attention_span_kernel<false, 1, 24>);
      else if (nchl == 32) go(decode_cross_attention_span_kernel<false, 1, 32>);
      else go(decode_cross_attention_span_kernel<false, 1, 0>);
    }
  } else {
    if (!p.q) { fprintf(stderr, "[ax_whisper] span cross-attention: no query\n"); abort(); }
    if (fp8) go(decode_cross_attention_span_kernel<true, 0, 0>);
    else go(decode_cross_attention_span_kernel<false, 0, 0>);
  }
}

// spans[slot_map ? slot_map[i] : i] = min(n_keys, ceil(samples[i] / 320) + margin); samples == nullptr: n_keys (length unknown)
__global__ void cross_span_set_kernel(const int* samples, const int* slot_map, int* spans, int count, int n_slots, int margin, int n_keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int slot = slot_map ? slot_map[i] : i;
  if (slot < 0 || slot >= n_slots) return;
  spans[slot] = samples ? cross_span_frames(samples[i], margin, n_keys) : n_keys;
}
void launch_cross_span_set(const int* samples, const int* slot_map, int* spans, int count, int n_slots, int margin, int n_keys, hipStream_t s) {
  hipLaunchKernelGGL(cross_span_set_kernel, dim3((count + 255) / 256), dim3(256), 0, s, samples, slot_map, spans, count, n_slots, margin, n_keys);
}

}  // inline namespace AXW_NS
}  // namespace axw
