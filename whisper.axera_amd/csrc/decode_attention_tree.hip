// decode_attention_tree.hip — beam search's self-attention over an ancestry table, on gfx950 (DESIGN.md "Beam search", "Tree
// self-attention"), and the table's update kernel.
//
// The K hypotheses ("ranks") of a clip sit in the slots [c K, c K + K). Position p of every slot's self K/V is written exactly once, at
// step p, and never changes; the copy path moves whole cache blocks between slots when a hypothesis changes its slot
// (beam_reorder_kernel) and decode_attention_kernel then streams every slot's whole history: K times nearly the same keys. Here the
// cache never moves. origin[slot][p] (uint8) says which of the clip's K slots holds the K/V row of position p of the hypothesis that
// lives in `slot` now; ONE workgroup per (head, clip) serves all ranks of the clip that lie inside the launch's slot range and loads
// every (slot, 64-key block) that any of them references once.
//
// Work split. 256 threads = 4 waves; wave w takes the 64-key blocks w, w + 4, ... of [0, max offset / 64] (the self cache holds at most
// eight blocks: no key split across workgroups). G <= 8 ranks x the (hi, lo) h16 split of the fp32 query are the 16-row A operand of
// v_mfma_f32_16x16x32, as in decode_attention_group.hip, whose operand movement this kernel takes as it is: K pieces of the blocked
// cache straight from global memory into the B registers (kv_chunk_offset), row-major V through the LDS image of
// layout::cross_v_swizzle read with ds_read_b64_tr_b16, fp32 online softmax with two ranks per lane group, the probability (hi, lo)
// image as the second A operand, the fragment-major output pair.
//
// The gather (what is new).
//   prologue  The workgroup brings its ranks' origin rows into LDS as s_org[rank][p]: the local slot rank g reads key p from —
//             origin[slot][p] below the rank's offset, the rank's OWN slot at its offset (the row this step's QKV launch wrote: the kernel
//             takes it as the slot's own whatever the table holds there), kNoSlot beyond it and for ranks that are done. Beside it
//             s_used[p]: bit s is set where some live rank reads key p from local slot s.
//   need      For its block a wave ORs s_used over the block's 64 keys (one vote per slot): the local slots to load.
//   scores    For every s in need: slot s's K block x all ranks' queries (8 MFMAs), then S[r][p] is TAKEN from that product where
//             s_org[r][p] == s — a select, not a multiply, so that whatever an unreferenced row holds (another slot's position `off`, which
//             a concurrent branch's QKV launch may be writing at this moment; NaN bits in a test) never reaches a score.
//   output    After the softmax update, for every s in need: O += P_s V_s with P_s[r][p] = P[r][p] where s_org[r][p] == s, else 0. 0 x NaN
//             is NaN on the matrix cores, so a V row (s, p) that no live rank reads is ZEROED on its way into the LDS tile (bit s of
//             s_used[p] clear): every row that reaches an accumulator is one that some rank of this launch attends over.
//   Keys beyond the largest offset are never loaded (the clamp rule of the other attention kernels: such a lane reads the block's last
//   valid key again).
// One register set per operand: the next (slot, block)'s V is requested as soon as the tile is in LDS, the next K as soon as the
// scores are formed — the next slot of this block's need, or the first slot of the wave's next block.
// A rank whose done flag is set gets no output; a group whose ranks are all done returns before any table or K/V request.
#include "common.hpp"
#include "decode_attention_common.hpp"
#include "decode_attention_group_common.hpp"

namespace axw {
inline namespace AXW_NS {

using layout::kPartStride;
using layout::kPartM;
using layout::kPartL;
using layout::kPartO;

namespace {

constexpr int kTreeKeysMax = kTreeBlocksMax * layout::kKvBlockKeys;  // keys per row of the LDS origin image
constexpr unsigned kNoSlot = 0xffu;

// base: wave-uniform pointer of this (slot, head)'s K or V, off: element offset of this lane (decoder.hip ld_kv)
__device__ __forceinline__ u32x4 ld_kv_nt(const h16* base, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x27000);
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off * 2, 0, 2);  // aux 2 = nt
}
__device__ __forceinline__ int first_slot(unsigned need) { return __builtin_ctz(need); }

__global__ __launch_bounds__(256) void decode_self_attention_tree_kernel(DecAttnTreeParams p) {
  // the waves' V tiles [4][64 keys][64 dims]; behind the key loop the waves' records [4][8 ranks][66] fp32 (each wave's inside its own tile)
  __shared__ __attribute__((aligned(16))) h16 s_v[4 * layout::kKvBlockElems];
  __shared__ __attribute__((aligned(16))) h16 s_p[4 * kAImage];
  __shared__ __attribute__((aligned(16))) h16 s_qa[kAImage];
  __shared__ unsigned char s_org[kGroupMax * kTreeKeysMax];
  __shared__ unsigned char s_used[kTreeKeysMax];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int head = blockIdx.x;
  const int clip = p.slot0 / p.group + blockIdx.y;
  const int r_lo = max(0, p.slot0 - clip * p.group), r_hi = min(p.group, p.slot0 + p.nslots - clip * p.group);
  const int G = r_hi - r_lo;                         // 1 .. 8 ranks of this clip inside the range
  const int rel0 = clip * p.group + r_lo - p.slot0;  // the first of them, counted from slot0
  unsigned live = 0;
  for (int g = 0; g < G; ++g) live |= (p.done[rel0 + g] ? 0u : 1u) << g;
  if (!live) return;

  // ---- offsets, origin rows and queries -> LDS
  const int cap_keys = p.cap_blocks * layout::kKvBlockKeys;
  int off_g[kGroupMax], max_off = 0;  // (an offset outside the cache is clamped: the launch never reads beyond a slot's allocation)
#pragma unroll
  for (int g = 0; g < kGroupMax; ++g) {
    off_g[g] = g < G && (live >> g & 1) ? max(0, min(p.off[rel0 + g], cap_keys - 1)) : -1;
    max_off = max(max_off, off_g[g]);
  }
  const int n_blk = (max_off >> 6) + 1;
  const unsigned char* org = p.origin + (long)(clip * p.group + r_lo) * p.origin_stride;
  for (int key = tid; key < n_blk * layout::kKvBlockKeys; key += 256) {
    unsigned used = 0;
#pragma unroll
    for (int g = 0; g < kGroupMax; ++g) {
      unsigned e = kNoSlot;
      if (key <= off_g[g]) {  // (a local slot beyond the clip's is clamped too, for the same reason)
        e = key == off_g[g] ? (unsigned)(r_lo + g) : min((unsigned)org[(long)g * p.origin_stride + key], (unsigned)(p.group - 1));
        used |= 1u << e;
      }
      s_org[g * kTreeKeysMax + key] = (unsigned char)e;
    }
    s_used[key] = (unsigned char)used;
  }
  for (int g = wave; g < kGroupMax; g += 4) put_pair(s_qa, g, lane, g < G ? p.q[(long)(rel0 + g) * p.d_model + head * 64 + lane] : 0.f);
  __syncthreads();

  const long head_elems = layout::kv_head_elems(cap_keys);
  const h16* kb = p.k + (long)clip * p.group * p.kv_slot_stride + head * head_elems;  // local slot 0 of the clip
  const h16* vb = p.v + (long)clip * p.group * p.kv_slot_stride + head * head_elems;
  u32x4 kn[8], vn[8];  // kn[2 kb + ks]: the B pieces of the scores; vn[i]: rows 8 i + lane / 8 of the V tile, chunk lane % 8
  auto load_k = [&](int s, int bk) {
    const h16* base = kb + (long)s * p.kv_slot_stride;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = min(16 * (i >> 1) + (lane & 15), max_off - bk * 64);
      kn[i] = ld_kv_nt(base, layout::kv_chunk_offset(bk, 4 * (i & 1) + (lane >> 4), key));
    }
  };
  auto load_v = [&](int s, int bk) {
    const h16* base = vb + (long)s * p.kv_slot_stride;
#pragma unroll
    for (int i = 0; i < 8; ++i) vn[i] = ld_kv_nt(base, layout::v_index(min(bk * 64 + 8 * i + (lane >> 3), max_off), (lane & 7) * 8));
  };
  // the local slots block bk is read from: wave-uniform
  auto need_of = [&](int bk) {
    const unsigned ub = s_used[bk * 64 + lane];
    unsigned need = 0;
#pragma unroll
    for (int s = 0; s < kGroupMax; ++s) need |= (__any((int)(ub >> s & 1u)) ? 1u : 0u) << s;
    return (unsigned)__builtin_amdgcn_readfirstlane((int)need);
  };
  int blk = wave;
  unsigned need = blk < n_blk ? need_of(blk) : 0u;  // (never empty: the rank with the largest offset reads every key of the block up to it)
  if (need) { load_k(first_slot(need), blk); load_v(first_slot(need), blk); }
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
  for (; blk < n_blk; blk += 4) {
    const unsigned need_next = blk + 4 < n_blk ? need_of(blk + 4) : 0u;
    unsigned og[2][4], vu[8];  // whom this lane's two ranks read its four keys from; who reads the V rows this lane stages
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) og[e][kq] = s_org[(2 * q4 + e) * kTreeKeysMax + blk * 64 + 16 * kq + col];
#pragma unroll
    for (int i = 0; i < 8; ++i) vu[i] = s_used[blk * 64 + 8 * i + (lane >> 3)];

    // scores: one K block per referenced slot, each rank keeps the columns it reads from that slot
    float sv[2][4];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) sv[e][kq] = -INFINITY;
    for (unsigned rem = need; rem;) {
      const unsigned s = first_slot(rem);
      rem &= rem - 1;
      f32x4 sc[4];
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        sc[kq] = AXW_MFMA_16x16x32(qa0, __builtin_bit_cast(h16x8, kn[2 * kq]), (f32x4{0.f, 0.f, 0.f, 0.f}));
        sc[kq] = AXW_MFMA_16x16x32(qa1, __builtin_bit_cast(h16x8, kn[2 * kq + 1]), sc[kq]);
      }
      if (rem) load_k(first_slot(rem), blk);
      else if (need_next) load_k(first_slot(need_next), blk + 4);
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int kq = 0; kq < 4; ++kq)
          if (og[e][kq] == s) sv[e][kq] = (sc[kq][2 * e] + sc[kq][2 * e + 1]) * 0.125f;  // (64^-0.25)^2, export_onnx.py:116,124-126
    }
    float pk[2][4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float mx = -INFINITY;
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) mx = fmaxf(mx, sv[e][kq]);
      const float m_new = fmaxf(m_r[e], row16_max(mx));
      // a rank that reads no key of any block so far (done, outside the range, or at an offset below this block): weights 0, not NaN
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __expf(m_r[e] - m_use);
      m_r[e] = m_new;
      float l = l_r[e] * alpha;
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        pk[e][kq] = __expf(sv[e][kq] - m_use);
        l += pk[e][kq];
      }
      l_r[e] = l;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) { o[nb][2 * e] *= alpha; o[nb][2 * e + 1] *= alpha; }
    }
    // output: one V block per referenced slot, rows nobody reads from that slot zeroed, each rank's weights on the rows it reads from it
    for (unsigned rem = need; rem;) {
      const unsigned s = first_slot(rem);
      rem &= rem - 1;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<u32x4*>(tile + layout::cross_v_index(8 * i + (lane >> 3), (lane & 7) * 8, true)) = (vu[i] >> s & 1u) ? vn[i] : u32x4{0u, 0u, 0u, 0u};
      if (rem) load_v(first_slot(rem), blk);
      else if (need_next) load_v(first_slot(need_next), blk + 4);
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) put_pair(pimg, 2 * q4 + e, 16 * kq + col, og[e][kq] == s ? pk[e][kq] : 0.f);
      __builtin_amdgcn_wave_barrier();  // the wave's own LDS writes (tile, probabilities) precede its reads
      const h16x8 pa0 = a_frag(pimg, 0, lane), pa1 = a_frag(pimg, 1, lane);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        o[nb] = AXW_MFMA_16x16x32(pa0, v_frag(tile, vbase, nb, 0), o[nb]);
        o[nb] = AXW_MFMA_16x16x32(pa1, v_frag(tile, vbase, nb, 1), o[nb]);
      }
      __builtin_amdgcn_wave_barrier();  // ... and its reads the next slot's writes
    }
    need = need_next;
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
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // this thread's ranks wave and wave + 4, dimension `lane`
    const int g = wave + 4 * j;
    if (!(g < G && (live >> g & 1))) continue;
    float m, l, ov;
    attn::merge_wave_records(recs + g * kPartStride, kWaveRec, lane, m, l, ov);
    attn::store_out_pair(p.out_hi, p.out_lo, rel0 + g, head * 64 + lane, p.nbs, ov / l);
  }
}

// grid (slots): a slot whose hypothesis came from another slot of its clip takes that slot's history [0, n) and origin row
// [0, n_origin); no K/V moves. No slot is both read and written in one launch (beam_select_kernel's slot assignment), rows included.
__global__ __launch_bounds__(256) void beam_ancestry_kernel(BeamAncestryParams p) {
  const int slot = blockIdx.x, from = p.src[slot];
  if (from == slot) return;  // it stays where it is, or its clip is complete
  const int tid = threadIdx.x;
  const int* hs = p.hist + (long)from * p.hist_stride;
  int* hd = p.hist + (long)slot * p.hist_stride;
  for (int i = tid; i < p.n; i += 256) hd[i] = hs[i];
  const unsigned char* os = p.origin + (long)from * p.origin_stride;
  unsigned char* od = p.origin + (long)slot * p.origin_stride;
  for (int i = tid; i < p.n_origin; i += 256) od[i] = os[i];
}

}  // namespace

void launch_decode_self_attention_tree(const DecAttnTreeParams& p, hipStream_t s) {
  if (!(p.group >= 1 && p.group <= kGroupMax && p.nslots >= 1 && p.slot0 >= 0 && p.slot0 % 16 == 0 && p.n_head >= 1 &&
        p.d_model == p.n_head * layout::kKvDim && p.cap_blocks >= 1 && p.cap_blocks <= kTreeBlocksMax && p.k && p.v && p.q && p.off && p.done &&
        p.origin && p.origin_stride >= p.cap_blocks * layout::kKvBlockKeys && p.out_hi && p.out_lo)) {
    fprintf(stderr, "[ax_whisper] tree self-attention: group %d, slots %d + %d, d_model %d, n_head %d, %d key blocks, origin rows of %d unsupported\n",
            p.group, p.slot0, p.nslots, p.d_model, p.n_head, p.cap_blocks, p.origin_stride);
    abort();
  }
  hipLaunchKernelGGL(decode_self_attention_tree_kernel, dim3(p.n_head, cross_group_clips(p.slot0, p.nslots, p.group)), dim3(256), 0, s, p);
}

void launch_beam_ancestry(const BeamAncestryParams& p, hipStream_t s) {
  if (!(p.n_slots >= 1 && p.n >= 0 && p.n <= p.hist_stride && p.n_origin >= 0 && p.n_origin <= p.origin_stride && p.src && p.hist && p.origin)) {
    fprintf(stderr, "[ax_whisper] launch_beam_ancestry: history length %d of %d / origin length %d of %d unsupported\n", p.n, p.hist_stride,
            p.n_origin, p.origin_stride);
    abort();
  }
  hipLaunchKernelGGL(beam_ancestry_kernel, dim3(p.n_slots), dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
