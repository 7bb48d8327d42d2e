// vocab_logprob.hip — the token probabilities of word-level timestamps without the logits (DESIGN.md "Word-level timestamps",
// "Fused vocabulary log-probabilities"): lp[r] = logit[r][id[r]] - logsumexp over columns [0, eot) of logit[r][.], where
// logit = LayerNorm(x) . W^T over the tied embedding W [n_vocab][d]. Three launches on one stream:
//   launch_layernorm_bf16     (gemm.hip) the fp32 rows, normalised in fp32, written once as the 16-bit B operand a [rows_pad][d]
//   vocab_logprob_kernel      grid = row tiles x vocabulary splits; one (max, sum) partial per (split, row), the target logit per row
//   vocab_logprob_merge_kernel  the partials of a row in split order -> lp[r]
// No workgroup waits for another and nothing is accumulated through atomics: every partial and every target has one owner, the merge
// walks the splits in a fixed order, so the output has the same bits every run.
//
// vocab_logprob_kernel: the operand arrangement of align_qk_softmax_kernel (decode_align.hip). Workgroup = 4 waves; the row tile
// (16 NR rows of a, NR = 4, 2 or 1 by d: vocab_logprob_plan) is staged once in LDS, rows 16 bytes apart from a multiple of the bank
// period, and read as 16-byte pieces. A wave owns 64 columns of every 256-column chunk of its split: logit^T = W a^T on
// v_mfma_f32_16x16x32 with A = 16 rows of W x 32 dims straight from global memory and B = 16 rows of the tile from LDS, so a lane has
// ONE row of x per row group and 4 columns per tile, and the fold of a tile into the row's online (max, sum) is one lse_add4 in the
// lane's own registers. Of every 64 dims lane group g takes dims [16 g, 16 g + 16) (the same bijection for A and B: a dot product
// does not care), so the four groups of a W row read one whole 128-byte line, each lane 32 consecutive bytes.
// Columns at or beyond eot enter the fold as -inf; the W row a lane reads is clamped to n_vocab - 1, so nothing beyond the table is
// touched. Rows at or beyond `rows` are the zeros the caller left in a; they are computed and never stored.
#include "decode_rules.hpp"

namespace axw {
inline namespace AXW_NS {

constexpr int kVlpLdPad = 8;  // h16 elements (16 bytes) between the LDS rows: row r starts at bank 4 r (mod 64) + a multiple of 64

template <int NR>
__global__ __launch_bounds__(256) void vocab_logprob_kernel(VocabLogProbParams p) {
  extern __shared__ __align__(16) unsigned char vlp_smem[];
  __shared__ float red[4][NR * 16][3];
  h16* xs = reinterpret_cast<h16*>(vlp_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, ldx = d + kVlpLdPad;
  const int r0 = blockIdx.x * (NR * 16), split = blockIdx.y;
  const int c_begin = split * p.split_cols, c_end = min(c_begin + p.split_cols, p.eot);

  // the row tile -> LDS (a holds whole row tiles)
  const int pieces = d >> 3;
  for (int i = tid; i < NR * 16 * pieces; i += 256) {
    const int r = i / pieces, q = i - r * pieces;
    *reinterpret_cast<u32x4*>(xs + r * ldx + q * 8) = *reinterpret_cast<const u32x4*>(p.a + (long)(r0 + r) * d + q * 8);
  }
  __syncthreads();

  float m[NR], s[NR], tg[NR];
  int idr[NR];
#pragma unroll
  for (int nr = 0; nr < NR; ++nr) {
    const int row = r0 + nr * 16 + col;
    m[nr] = -INFINITY; s[nr] = 0.f; tg[nr] = -INFINITY;
    idr[nr] = row < p.rows ? p.id[row] : -1;
  }

  for (int c0 = c_begin + wave * 64; c0 < c_end; c0 += 256) {
    f32x4 acc[4][NR];
    const h16* wrow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      wrow[t] = p.W + (long)min(c0 + t * 16 + col, p.n_vocab - 1) * d + g * 16;
#pragma unroll
      for (int nr = 0; nr < NR; ++nr) acc[t][nr] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const h16* xrow = xs + col * ldx + g * 16;
    for (int kp = 0; kp < d; kp += 64) {
      h16x8 wf[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) wf[t][hh] = *reinterpret_cast<const h16x8*>(wrow[t] + kp + hh * 8);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) {
          const h16x8 xf = *reinterpret_cast<const h16x8*>(xrow + nr * 16 * ldx + kp + hh * 8);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t][nr] = AXW_MFMA_16x16x32(wf[t][hh], xf, acc[t][nr]);
        }
    }
    // acc[t][nr][i] = logit(row r0 + 16 nr + col, column c0 + 16 t + 4 g + i): the tile into the row's (max, sum), the target out of it
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cb = c0 + t * 16 + 4 * g;
#pragma unroll
      for (int nr = 0; nr < NR; ++nr) {
        const float x0 = cb < c_end ? acc[t][nr][0] : -INFINITY, x1 = cb + 1 < c_end ? acc[t][nr][1] : -INFINITY;
        const float x2 = cb + 2 < c_end ? acc[t][nr][2] : -INFINITY, x3 = cb + 3 < c_end ? acc[t][nr][3] : -INFINITY;
        lse_add4(m[nr], s[nr], x0, x1, x2, x3);
        const int e = idr[nr] - cb;
        if (e >= 0 && e < 4) tg[nr] = e == 0 ? x0 : e == 1 ? x1 : e == 2 ? x2 : x3;
      }
    }
  }

  // the four lane groups of a row (fixed order: xor butterfly), then the four waves in wave order
#pragma unroll
  for (int nr = 0; nr < NR; ++nr) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float m2 = __shfl_xor(m[nr], o, 64), s2 = __shfl_xor(s[nr], o, 64);
      lse_merge(m[nr], s[nr], m2, s2);
      tg[nr] = fmaxf(tg[nr], __shfl_xor(tg[nr], o, 64));  // (one lane of the launch holds the target, the others -inf)
    }
    if (g == 0) {
      red[wave][nr * 16 + col][0] = m[nr];
      red[wave][nr * 16 + col][1] = s[nr];
      red[wave][nr * 16 + col][2] = tg[nr];
    }
  }
  __syncthreads();
  if (tid < NR * 16) {
    const int row = r0 + tid;
    if (row < p.rows) {
      float mm = red[0][tid][0], ss = red[0][tid][1], tt = red[0][tid][2];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        lse_merge(mm, ss, red[w][tid][0], red[w][tid][1]);
        tt = fmaxf(tt, red[w][tid][2]);
      }
      p.part_m[(long)split * p.rows + row] = mm;
      p.part_s[(long)split * p.rows + row] = ss;
      const int t = p.id[row];
      if (t >= c_begin && t < c_end) p.target[row] = tt;  // (the split that holds the id owns the row's target)
    }
  }
}

// lp[r] from the partials of row r, in split order; an id outside [0, eot) has no owner above: -inf
__global__ __launch_bounds__(256) void vocab_logprob_merge_kernel(VocabLogProbParams p) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= p.rows) return;
  float m = -INFINITY, s = 0.f;
  for (int sp = 0; sp < p.n_splits; ++sp) lse_merge(m, s, p.part_m[(long)sp * p.rows + row], p.part_s[(long)sp * p.rows + row]);
  const int t = p.id[row];
  p.out[row] = t >= 0 && t < p.eot ? logprob_of(p.target[row], m, s) : -INFINITY;
}

template <int NR>
static void launch_vocab_logprob_main(const VocabLogProbParams& p, hipStream_t s) {
  const size_t lds = (size_t)NR * 16 * (p.d + kVlpLdPad) * sizeof(h16);
  // (above 64 KB the dynamic LDS of a kernel has to be admitted, on every device that runs it)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&vocab_logprob_kernel<NR>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kVocabLogProbMaxLds);
  if (e != hipSuccess) {
    fprintf(stderr, "[ax_whisper] launch_vocab_logprob: hipFuncSetAttribute: %s\n", hipGetErrorString(e));
    abort();
  }
  const int tiles = (p.rows + NR * 16 - 1) / (NR * 16);
  hipLaunchKernelGGL(vocab_logprob_kernel<NR>, dim3(tiles, p.n_splits), dim3(256), lds, s, p);
}

void launch_vocab_logprob(const VocabLogProbParams& p, hipStream_t s) {
  if (p.rows < 1) return;
  int row_tile, n_splits, split_cols;
  const bool ok = vocab_logprob_plan(p.d, p.rows, p.eot, &row_tile, &n_splits, &split_cols);
  if (!ok || p.eot > p.n_vocab || row_tile != p.row_tile || n_splits != p.n_splits || split_cols != p.split_cols ||
      (size_t)row_tile * (p.d + kVlpLdPad) * sizeof(h16) > kVocabLogProbMaxLds) {
    fprintf(stderr, "[ax_whisper] launch_vocab_logprob: %d rows of %d, %d of %d ids, plan %d / %d / %d unsupported\n", p.rows, p.d, p.eot, p.n_vocab,
            p.row_tile, p.n_splits, p.split_cols);
    abort();
  }
  if (row_tile == 64) launch_vocab_logprob_main<4>(p, s);
  else if (row_tile == 32) launch_vocab_logprob_main<2>(p, s);
  else launch_vocab_logprob_main<1>(p, s);
  hipLaunchKernelGGL(vocab_logprob_merge_kernel, dim3((p.rows + 255) / 256), dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
