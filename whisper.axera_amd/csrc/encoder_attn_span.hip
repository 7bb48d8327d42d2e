// encoder_attn_span.hip — ragged self-attention of the audio encoder: clip b attends among its first span_b frames only
// (AX_WHISPER_CROSS_SPAN=encoder; DESIGN.md "Encoder spans"). The sibling of encoder_attn.hip with the same data path: K tile and V^T
// tile double-buffered in XOR-swizzled LDS, S^T = K Q^T with the query in registers, the exponentiated accumulator narrowed in place as
// the B operand of O^T = V^T P^T, the deferred rescale under `rescale_thr`. What is its own:
//
//   Ragged shape. Clips lie at the uniform row stride of the encoder's buffers (`rows` frames); each has its own span, read from a
//   device array. The key loop runs ceil(span / 64) tiles and the tail mask sits at `span`, inside whichever tile that is.
//
//   Nothing at or beyond the span is trusted. Q rows, K rows and V^T columns >= span may hold any bit pattern (stale activations of
//   an earlier, longer pass; memory never written), NaN and Inf included, and 0 * NaN = NaN, so a masked probability of 0 is not
//   enough. Queries: a lane whose row is >= span loads row span - 1 instead and stores zeros. K: the buffer resource ends behind row
//   span - 1, so the tail tile's rows beyond it read as zeros. V^T: the frames of a 16-group are stored permuted, so no range check
//   fits; the staging registers of the TAIL tile are masked by frame before they go to LDS (8 h16 per chunk, two chunks per thread,
//   once per workgroup). Full tiles run the parent's instructions.
//
//   Work list. One workgroup = one item (clip, head, query block) for the blocks below the span only. The host builds the list from
//   the spans alone (build_encoder_span_list; no atomics, no device-side plan): clips by falling span (the long items start first),
//   clip-major, then head, the query block fastest, so the blocks of one (clip, head) are neighbours. Workgroups are dealt round-robin
//   over the 8 XCDs, each with its own L2, and K / V^T of a (clip, head) should come through ONE L2 (encoder_attn.hip: dealt in launch
//   order they were fetched 4.6 times). So XCD x takes a contiguous chunk [chunk[x], chunk[x + 1]) of the list, workgroup 8 j + x its
//   j-th item. The chunks are cut on the prefix sums of the items' cost (key tiles + 1), not of their number: cut by number, the first
//   XCD would hold only long clips and the last only short ones. The grid is 8 x the longest chunk; surplus workgroups leave at once.
//
//   Two query-block heights. 128 rows: the parent's split, wave w = query rows 32 w .. 32 w + 31 over all keys. 64 rows, for passes
//   with too few items to fill the machine: wave w = query rows 32 (w & 1) .. + 31 over the 32-key half (w >> 1) of EVERY tile, so all
//   four waves still share each staged tile and each issues half of its MFMAs; waves 2 and 3 hand their (m, l, O) to waves 0 and 1
//   through the tile buffers at the end (one exchange per workgroup). A wave whose half of the tail tile is wholly masked skips it.
//
//   Output rows [span, rows_out) are written as zeros: a block's own rows beyond the span by their lanes, the blocks no item covers in
//   equal shares by the items of that (clip, head). Everything downstream of the attention is then finite by construction.
#include "common.hpp"
#include <algorithm>
#include <numeric>
#include <type_traits>

namespace axw {
inline namespace AXW_NS {

namespace {
__device__ __forceinline__ int swz128s(int row, int chunk) { return row * 128 + 16 * (chunk ^ ((row >> 1) & 7)); }
}  // namespace

template <int QROWS>
__global__ __launch_bounds__(256, 2) void encoder_attention_span_kernel(EncSpanAttnParams p) {
  __shared__ __attribute__((aligned(16))) char KVs[2][2][64 * 128];  // [buffer][K | V^T]; at the end of a 64-row block the exchange
  constexpr bool SPLIT = QROWS == 64;
  constexpr int NKB = SPLIT ? 1 : 2;  // 32-key halves of a tile one wave takes

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  int qblk, head, b;
  {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int c0 = p.chunk[xcd];
    if (j >= p.chunk[xcd + 1] - c0) return;
    const int item = p.items[c0 + j];
    qblk = item & 63;
    head = (item >> 6) & 63;
    b = item >> 12;
  }
  const int T = p.rows, d_model = p.d_model, t_pad = p.t_pad;
  const int span = min(max(p.spans[b], 1), T);
  const int qw = SPLIT ? (wave & 1) : wave;   // 32-row group of the block
  const int kb0 = SPLIT ? (wave >> 1) : 0;    // first 32-key half of a tile
  const int q_row = qblk * QROWS + qw * 32 + r;
  const int q_ld = min(q_row, span - 1);

  const h16* Qb = p.q + ((long)b * T) * d_model + head * 64;
  const h16* Kb = p.k + ((long)b * T) * d_model + head * 64;
  const h16* Vb = p.vt + ((long)b * p.n_head + head) * 64 * t_pad;

  h16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const h16x8*>(Qb + (long)q_ld * d_model + 16 * s + 8 * h);

  f32x16 oacc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[i][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int ld_row = tid >> 3, ld_c = tid & 7;
  const int nkt = (span + 63) >> 6;
  u32x4 rk[2], rv[2];
  // (encoder_attn.hip on the buffer loads) K's resource ends behind row span - 1: whatever lies beyond is never fetched
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (unsigned)(((long)span * d_model - head * 64) * 2), 0x27000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, (unsigned)(64 * t_pad * 2), 0x27000);
  int offk[2], offv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    offk[i] = ((ld_row + 32 * i) * d_model + ld_c * 8) * 2;
    offv[i] = ((ld_row + 32 * i) * t_pad + ld_c * 8) * 2;
  }
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rk[i] = __builtin_amdgcn_raw_buffer_load_b128(rsK, offk[i] + kt * 64 * d_model * 2, 0, 0);
      rv[i] = __builtin_amdgcn_raw_buffer_load_b128(rsV, offv[i], kt * 64 * 2, 0);
    }
  };
  // The staged V^T chunks of the tail tile, masked by frame: chunk ld_c holds positions 8 ld_c .. + 7 of the tile, which in the stored
  // order [0-3, 8-11 | 4-7, 12-15] of a 16-group are frames 16 (ld_c >> 1) + 4 (ld_c & 1) + {0 .. 3, 8 .. 11}; word w = frames f, f + 1.
  auto mask_tail_v = [&]() {
    const int f0 = (nkt - 1) * 64 + 16 * (ld_c >> 1) + 4 * (ld_c & 1);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int f = f0 + 2 * (w & 1) + 8 * (w >> 1);
      const unsigned keep = (f < span ? 0x0000ffffu : 0u) | (f + 1 < span ? 0xffff0000u : 0u);
      rv[0][w] &= keep;
      rv[1][w] &= keep;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(KVs[buf][0] + swz128s(ld_row + 32 * i, ld_c)) = rk[i];
      *reinterpret_cast<u32x4*>(KVs[buf][1] + swz128s(ld_row + 32 * i, ld_c)) = rv[i];
    }
  };

  load_tile(0);
  if (nkt == 1) mask_tail_v();
  store_tile(0);
  __syncthreads();

  const float sc = 0.125f * 1.44269504088896340736f;  // (64^-0.25)^2 * log2(e)

  // One 64-key tile out of LDS (encoder_attn.hip: process_tile), a wave's NKB halves of it from half kb0 on. TAIL masks the keys >=
  // span: the last tile only.
  auto process_tile = [&](int kt, auto tail_tag, const char* Ks, const char* Vs) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    if constexpr (TAIL && SPLIT) {
      if (kt * 64 + kb0 * 32 >= span) return;  // (wave-uniform) none of this wave's keys exists: m, l, O stay as they are
    }
    // ---- S^T = K Q^T : sacc[i][e] = score(key = kt*64 + (kb0+i)*32 + (e&3) + 8*(e>>2) + 4h, query = lane r)
    f32x16 sacc[NKB];
#pragma unroll
    for (int i = 0; i < NKB; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[i][e] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        h16x8 kf = *reinterpret_cast<const h16x8*>(Ks + swz128s((kb0 + i) * 32 + r, 2 * s + h));
        sacc[i] = AXW_MFMA_32x32x16(kf, qf[s], sacc[i]);
      }
    }
    // ---- online softmax (fp32, base-2)
    float mt = -INFINITY;
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if constexpr (TAIL) {
          const int key = kt * 64 + (kb0 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          if (key >= span) sacc[i][e] = -INFINITY;
        }
        mt = fmaxf(mt, sacc[i][e]);
      }
    {
      auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
      mt = fmaxf(__uint_as_float(r2[0]), __uint_as_float(r2[1]));
    }
    // raise the running maximum only if some row needs it (every tile a wave processes has at least one unmasked key of its own)
    if (__builtin_amdgcn_ballot_w64((mt - m_run) * sc > p.rescale_thr) != 0) {
      const float m_new = fmaxf(m_run, mt);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[i][e] *= alpha;
    }
    const float m_sc = m_run * sc;
    float ls = 0.f;
    h16x8 pf[NKB][2];
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float pv = __builtin_amdgcn_exp2f(fmaf(sacc[i][e], sc, -m_sc));
        ls += pv;
        pf[i][e >> 3][e & 7] = (h16)pv;
      }
    l_run += ls;
    // ---- O^T += V^T P^T (encoder_attn.hip: the 8 h16 at positions 8h .. 8h+7 of a 16-group in the stored frame order)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int i = 0; i < NKB; ++i)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const h16x8 vf = *reinterpret_cast<const h16x8*>(Vs + swz128s(db * 32 + r, 4 * (kb0 + i) + 2 * s2 + h));
          oacc[db] = AXW_MFMA_32x32x16(vf, pf[i][s2], oacc[db]);
        }
  };

  // Tile kt is in buffer kt & 1. The loop stores full tiles only (its staging registers are assigned unconditionally, two tiles per
  // iteration, the buffers compile-time constants as in the parent); the last one or two stores, the masked one among them, are peeled.
  int kt = 0;
  for (; kt + 3 < nkt; kt += 2) {
    load_tile(kt + 1);
    process_tile(kt, std::false_type{}, KVs[0][0], KVs[0][1]);
    store_tile(1);
    __syncthreads();
    load_tile(kt + 2);
    process_tile(kt + 1, std::false_type{}, KVs[1][0], KVs[1][1]);
    store_tile(0);
    __syncthreads();
  }
  int buf = 0;
  if (kt + 3 == nkt) {  // three tiles left: one more full store
    load_tile(kt + 1);
    process_tile(kt, std::false_type{}, KVs[0][0], KVs[0][1]);
    store_tile(1);
    __syncthreads();
    ++kt;
    buf = 1;
  }
  if (kt + 2 == nkt) {  // two left: the tail tile is staged, masked and stored while the last full one is read
    load_tile(kt + 1);
    process_tile(kt, std::false_type{}, KVs[buf][0], KVs[buf][1]);
    mask_tail_v();
    store_tile(buf ^ 1);
    __syncthreads();
    ++kt;
    buf ^= 1;
  }
  process_tile(kt, std::true_type{}, KVs[buf][0], KVs[buf][1]);

  if constexpr (SPLIT) {
    // waves 2, 3 -> waves 0, 1: [wave - 2][34 values][64 lanes] fp32 over the tile buffers (17 KB of 32), lane-contiguous
    float* xch = reinterpret_cast<float*>(&KVs[0][0][0]);
    __syncthreads();  // every wave is done with the tiles
    if (wave >= 2) {
      float* dst = xch + (wave - 2) * 34 * 64 + lane;
      dst[0] = m_run;
      dst[64] = l_run;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) dst[(2 + 16 * i + e) * 64] = oacc[i][e];
    }
    __syncthreads();
    if (wave < 2) {
      const float* src = xch + wave * 34 * 64 + lane;
      const float m2 = src[0], l2 = src[64];
      const float m_new = fmaxf(m_run, m2);  // finite: waves 0, 1 hold key 0 of every tile
      const float a1 = __builtin_amdgcn_exp2f((m_run - m_new) * sc), a2 = __builtin_amdgcn_exp2f((m2 - m_new) * sc);  // m2 = -inf: a2 = 0
      l_run = l_run * a1 + l2 * a2;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[i][e] = oacc[i][e] * a1 + src[(2 + 16 * i + e) * 64] * a2;
    }
  }

  h16* Ob = p.o + ((long)b * T) * d_model + head * 64;
  if (!SPLIT || wave < 2) {
    const float l = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = q_row < span ? 1.f / l : 0.f;  // a row beyond the span computed row span - 1 again: finite, stored as zeros
    if (q_row < p.rows_out) {
      h16* orow = Ob + (long)q_row * d_model;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          h16x4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = (h16)(oacc[db][4 * g + e] * inv);
          *reinterpret_cast<h16x4*>(orow + db * 32 + 8 * g + 4 * h) = pk;
        }
    }
  }
  // this item's share of the rows no item covers: [nqb * QROWS, rows_out) in nqb equal parts, 32 rows of 128 bytes per step
  {
    const int nqb = (span + QROWS - 1) / QROWS;
    const int z0 = nqb * QROWS;
    const int per = (max(p.rows_out - z0, 0) + nqb - 1) / nqb;
    const int lo = z0 + qblk * per, hi = min(lo + per, p.rows_out);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int row = lo + ld_row; row < hi; row += 32) *reinterpret_cast<u32x4*>(Ob + (long)row * d_model + ld_c * 8) = zero;
  }
}

// The work list of a launch from the clips' spans (clamped to 1 .. rows): list.chunk[9] and list.items as the kernel reads them, and
// the grid. Item = clip << 12 | head << 6 | query block. Cost of an item: its key tiles plus one (prologue, epilogue).
EncSpanList build_encoder_span_list(const int* spans, int n, int rows, int n_head, int block_rows) {
  EncSpanList L;
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  auto sp = [&](int b) { return std::min(std::max(spans[b], 1), rows); };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sp(a) > sp(b); });
  long total = 0;
  for (int b = 0; b < n; ++b) total += (long)n_head * ((sp(b) + block_rows - 1) / block_rows) * ((sp(b) + 63) / 64 + 1);
  long before = 0;  // cost of the items in front of the next one
  int x = 0;
  L.chunk[0] = 0;
  for (int b : order) {
    const int nqb = (sp(b) + block_rows - 1) / block_rows, cost = (sp(b) + 63) / 64 + 1;
    for (int hd = 0; hd < n_head; ++hd)
      for (int qb = 0; qb < nqb; ++qb) {
        // XCD x ends where the cost in front reaches (x + 1) / 8 of the total, measured at an item's middle
        while (x < 7 && (2 * before + cost) * 8 >= 2 * total * (x + 1)) L.chunk[++x] = (int)L.items.size();
        L.items.push_back(b << 12 | hd << 6 | qb);
        before += cost;
      }
  }
  while (x < 8) L.chunk[++x] = (int)L.items.size();
  int longest = 0;
  for (int i = 0; i < 8; ++i) longest = std::max(longest, L.chunk[i + 1] - L.chunk[i]);
  L.grid = 8 * longest;
  return L;
}

void launch_encoder_attention_span(const EncSpanAttnParams& p, int block_rows, int grid, hipStream_t s) {
  if (p.n_head > 64 || p.rows > 64 * 63 || p.rows > p.t_pad || p.rows_out > p.rows || p.d_model < p.n_head * 64)
    throw std::runtime_error("encoder span attention: shape outside the kernel's item encoding or buffers");
  if (grid < 1) return;
  if (block_rows == 64) hipLaunchKernelGGL(encoder_attention_span_kernel<64>, dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(encoder_attention_span_kernel<128>, dim3(grid), dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
