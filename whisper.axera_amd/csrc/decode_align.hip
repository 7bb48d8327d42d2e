// decode_align.hip — word-level timestamps (DESIGN.md "Word-level timestamps"): from the cross-attention queries of a teacher-forced
// context to the frame at which every text token begins. openai-whisper timing.py's find_alignment, on the GPU:
//   align_qk_softmax_kernel   P = softmax over the clip's own F keys of q . k / 8, per alignment head, fp32        [clip][head][row][F_pad]
//   align_normalize_kernel    per head and frame: z = (P - mean) / std over the clip's rows, median of 7 along the frames
//                             (reflect padding), matrix += z / n_heads_total                                        [clip][row][frame]
//   align_dtw_kernel          dynamic time warping on -matrix[3 : L-1], anti-diagonal wavefront, the walk back over the trace in the
//                             same launch                                                                           jump [clip][N]
//
// align_qk_softmax_kernel: the operand arrangement of prefill_attention_kernel (decode_prefill.hip). Workgroup = 4 waves = 64 rows of
// one (clip, alignment head), 16 rows per wave; S^T = K Q^T on v_mfma_f32_16x16x32 with A = 16 keys x 32 dims straight from the
// blocked cross K (one 16-byte piece per lane) and B = the wave's query rows in registers, so a lane has ONE row and 4 keys per tile.
// Two sweeps over the clip's key blocks: the row maximum and sum (fp32, online), then P = exp2((s - m) / 8 * log2 e) / sum, written
// as 16-byte pieces. The key-count mask is applied in the last block only. Keys at or beyond the clip's count and rows at or
// beyond its length may hold anything (NaN included): a key's score depends on that key alone and a row's on that row alone.
//
// align_normalize_kernel: workgroup = 256 threads = 4 row groups x 64 frame columns, the columns being a tile of 58 frames with a
// halo of 3 on either side (with reflect padding every frame a tile's medians need lies inside its halo). Per head: column mean
// (pass 1) and centred squares (pass 2) over the clip's rows, the four row groups folded through LDS; then every thread of the tile's
// own 58 columns walks its rows: seven normalised neighbours, their median, one add into the matrix. An element of the matrix has one
// owner and the launches of successive layers are ordered on the stream: no atomics, the same bits every run.
//
// align_dtw_kernel: one workgroup of 512 threads per clip, thread i owns row i of the cost table. Diagonal d holds the cells
// i + j = d; three diagonals live in LDS, indexed by row, and a step is one barrier. One fp32 add per cell, x + the chosen
// predecessor (align_path.hpp: dtw_choice), so the accumulated cost is that of a numpy float32 evaluation whatever the lane order.
// A thread reads its row of the matrix in 16-byte pieces, one piece ahead of the cell it computes. One trace byte per cell goes to
// global memory ([N + 1][F + 1]); after the last diagonal one lane walks it back (dtw_backtrace) and writes jump[0, N).
#include "align_path.hpp"
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

__global__ __launch_bounds__(256) void align_qk_softmax_kernel(AlignQKParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.z, ah = blockIdx.y, qb = blockIdx.x;
  const int L = p.len[c];
  if (qb * 64 >= L) return;  // (the whole workgroup: clips of one launch differ in length)
  const int n_keys = p.n_keys[c];
  if (n_keys < 1) return;
  const int head = p.heads[ah];
  const int n_blocks = (n_keys + 63) / 64;
  const int col = lane & 15, g = lane >> 4;
  const int qpos = qb * 64 + wave * 16 + col;  // this lane's row: column of the B operand and of every accumulator
  const h16* qrow = p.q + (long)(p.row0[c] + min(qpos, L - 1)) * p.ldq + head * 64;
  h16x8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const h16x8*>(qrow + ks * 32 + g * 8);
  const h16* Kh = p.k + (long)p.slot[c] * p.kv_slot_stride + head * layout::kv_head_elems(p.keys_pad);
  const float sc = 0.125f * 1.44269504088896340736f;  // (64^-0.25)^2 * log2(e)

  // s[t][i] = score(key = kb*64 + t*16 + 4g + i, row = qpos), unscaled; masked keys -inf
  auto scores = [&](int kb, f32x4 (&s)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const h16x8 kf = *reinterpret_cast<const h16x8*>(Kh + layout::kv_chunk_offset(kb, ks * 4 + g, t * 16 + col));
        s[t] = AXW_MFMA_16x16x32(kf, qf[ks], s[t]);
      }
    }
    if (kb == n_blocks - 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (kb * 64 + t * 16 + 4 * g + i >= n_keys) s[t][i] = -INFINITY;
    }
  };

  // sweep 1: the row maximum and sum, online, base 2 (every block holds at least one key of the clip: the running maximum is finite)
  float m_run = -INFINITY, l_run = 0.f;
  for (int kb = 0; kb < n_blocks; ++kb) {
    f32x4 s[4];
    scores(kb, s);
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) mt = fmaxf(mt, s[t][i]);
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);
    m_run = m_new;
    const float m_sc = m_new * sc;
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) ls += __builtin_amdgcn_exp2f(fmaf(s[t][i], sc, -m_sc));
    l_run = l_run * alpha + ls;  // this lane's 16 keys of every block; the four groups are added below
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = 1.f / l_run, m_sc = m_run * sc;

  // sweep 2: P, a 16-byte piece per tile and lane (pieces of the last block may reach into [n_keys, f_pad): zeros)
  float* prow = p.P + (((long)c * p.n_align + ah) * p.rows_pad + qpos) * p.f_pad;
  for (int kb = 0; kb < n_blocks; ++kb) {
    f32x4 s[4];
    scores(kb, s);
    if (qpos < L) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 pv;
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = __builtin_amdgcn_exp2f(fmaf(s[t][i], sc, -m_sc)) * inv;
        *reinterpret_cast<f32x4*>(prow + kb * 64 + t * 16 + 4 * g) = pv;
      }
    }
  }
}

void launch_align_qk_softmax(const AlignQKParams& p, hipStream_t s) {
  if (p.n_clips < 1 || p.max_len < 1 || p.n_align < 1) return;
  if (p.f_pad % 64 != 0 || p.max_len > p.rows_pad) {
    fprintf(stderr, "[ax_whisper] launch_align_qk_softmax: scratch of %d rows x %d frames does not hold %d rows in whole key blocks\n", p.rows_pad,
            p.f_pad, p.max_len);
    abort();
  }
  hipLaunchKernelGGL(align_qk_softmax_kernel, dim3((p.max_len + 63) / 64, p.n_align, p.n_clips), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------ normalise + median + head mean
constexpr int kNormTile = 58, kNormHalo = 3;  // 58 + 2 * 3 = 64 columns

// the median of seven: the fourth smallest (min / max exchanges select, they do not round)
__device__ __forceinline__ float median7(float a, float b, float c, float d, float e, float f, float g) {
#define AXW_SORT2(x, y) { const float lo_ = fminf(x, y), hi_ = fmaxf(x, y); x = lo_; y = hi_; }
  // (13 exchanges; correct on all 128 inputs of zeros and ones, hence on every input)
  AXW_SORT2(a, f) AXW_SORT2(a, d) AXW_SORT2(b, g) AXW_SORT2(c, e) AXW_SORT2(a, b) AXW_SORT2(d, f) AXW_SORT2(c, g)
  AXW_SORT2(c, d) AXW_SORT2(d, g) AXW_SORT2(e, f) AXW_SORT2(b, e) AXW_SORT2(b, d) AXW_SORT2(d, e)
#undef AXW_SORT2
  return d;
}

__global__ __launch_bounds__(256) void align_normalize_kernel(AlignNormParams p) {
  __shared__ float part[4][64], mean[64], sd[64];
  const int tid = threadIdx.x, j = tid & 63, rg = tid >> 6;
  const int c = blockIdx.y, c0 = blockIdx.x * kNormTile;
  const int L = p.len[c], F = p.n_keys[c];
  if (c0 >= F || L < 1) return;  // (the whole workgroup)
  const int colj = c0 - kNormHalo + j;  // this thread's column of the window
  const bool live = colj >= 0 && colj < F;
  const bool own = live && j >= kNormHalo && j < kNormHalo + kNormTile;
  const bool filter = F > kNormHalo;
  // window positions of the seven neighbours of column colj, reflected at both ends of [0, F)
  int nb[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    int q = colj + k - kNormHalo;
    if (q < 0) q = -q;
    if (q >= F) q = 2 * (F - 1) - q;
    nb[k] = q - (c0 - kNormHalo);
  }
  for (int h = 0; h < p.n_align; ++h) {
    const float* P = p.P + ((long)c * p.n_align + h) * p.rows_pad * p.f_pad;
    float s = 0.f;
    if (live)
      for (int r = rg; r < L; r += 4) s += P[(long)r * p.f_pad + colj];
    part[rg][j] = s;
    __syncthreads();
    if (rg == 0) mean[j] = (part[0][j] + part[1][j] + part[2][j] + part[3][j]) / (float)L;
    __syncthreads();
    const float mu = mean[j];
    s = 0.f;
    if (live)
      for (int r = rg; r < L; r += 4) {
        const float dlt = P[(long)r * p.f_pad + colj] - mu;
        s = fmaf(dlt, dlt, s);
      }
    part[rg][j] = s;
    __syncthreads();
    if (rg == 0) sd[j] = sqrtf((part[0][j] + part[1][j] + part[2][j] + part[3][j]) / (float)L);
    __syncthreads();
    if (own) {
      const long col0 = c0 - kNormHalo;
      for (int r = rg; r < L; r += 4) {
        const float* row = P + (long)r * p.f_pad + col0;
        float z;
        if (filter) {
          float v[7];
#pragma unroll
          for (int k = 0; k < 7; ++k) v[k] = (row[nb[k]] - mean[nb[k]]) / sd[nb[k]];
          z = median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
        } else {
          z = (row[j] - mu) / sd[j];
        }
        float* out = p.matrix + ((long)c * p.m_rows + r) * p.m_ld + colj;
        *out = fmaf(z, p.inv_heads, *out);
      }
    }
    __syncthreads();  // (mean and sd are rewritten for the next head)
  }
}

void launch_align_normalize(const AlignNormParams& p, hipStream_t s) {
  if (p.n_clips < 1 || p.max_keys < 1 || p.n_align < 1) return;
  hipLaunchKernelGGL(align_normalize_kernel, dim3((p.max_keys + kNormTile - 1) / kNormTile, p.n_clips), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------------------ DTW
__global__ __launch_bounds__(kAlignDtwThreads) void align_dtw_kernel(AlignDtwParams p) {
  __shared__ float diag[3][kAlignDtwThreads];  // diag[d % 3][i] = cost[i][d - i]
  const int c = blockIdx.x, i = threadIdx.x;
  const int N = p.len[c] - 4, F = p.n_keys[c];  // rows 3 .. L-2 of the matrix
  if (N < 1 || F < 1 || N >= kAlignDtwThreads) return;  // (the whole workgroup; the launcher refuses longer clips)
  uint8_t* trace = p.trace + (long)c * p.trace_clip_stride;
  const long W = (long)F + 1;
  // row i of the table reads matrix row 3 + (i - 1), in pieces of four floats (m_ld is a multiple of 4, F <= m_ld)
  const float* xrow = p.matrix + ((long)c * p.m_rows + 3 + max(i - 1, 0)) * p.m_ld;
  const bool has_row = i >= 1 && i <= N;
  f32x4 cur = {0.f, 0.f, 0.f, 0.f}, nxt = {0.f, 0.f, 0.f, 0.f};
  if (has_row) nxt = *reinterpret_cast<const f32x4*>(xrow);
  const float inf = INFINITY;
  diag[0][i] = i == 0 ? 0.f : inf;  // d = 0: cost[0][0] = 0; cells with j < 0 read as border
  diag[1][i] = inf;                 // d = 1: cost[0][1] and cost[1][0]
  __syncthreads();
  for (int d = 2; d <= N + F; ++d) {
    const float* d1 = diag[(d - 1) % 3];
    const float* d2 = diag[(d - 2) % 3];
    const int j = d - i;
    float v = inf;  // row 0, column 0 and the cells this diagonal does not have
    if (has_row && j >= 1 && j <= F) {
      const int e = (j - 1) & 3;
      if (e == 0) {
        cur = nxt;
        if (j - 1 + 4 < F) nxt = *reinterpret_cast<const f32x4*>(xrow + j - 1 + 4);
      }
      const float x = -(e == 0 ? cur[0] : e == 1 ? cur[1] : e == 2 ? cur[2] : cur[3]);
      const float c0 = d2[i - 1], c1 = d1[i - 1], c2 = d1[i];
      const uint8_t t = dtw_choice(c0, c1, c2);
      v = x + (t == kTraceDiag ? c0 : t == kTraceUp ? c1 : c2);
      trace[(long)i * W + j] = t;
    }
    diag[d % 3][i] = v;
    __syncthreads();
  }
  // (the barrier above orders every trace byte of the workgroup before this lane's loads)
  if (i == 0) dtw_backtrace(trace, N, F, p.jump + (long)c * p.jump_ld);
}

void launch_align_dtw(const AlignDtwParams& p, hipStream_t s) {
  if (p.n_clips < 1) return;
  if (p.max_len - 4 >= kAlignDtwThreads || p.m_ld % 4 != 0) {
    fprintf(stderr, "[ax_whisper] launch_align_dtw: %d rows / a row stride of %d floats unsupported\n", p.max_len, p.m_ld);
    abort();
  }
  hipLaunchKernelGGL(align_dtw_kernel, dim3(p.n_clips), dim3(kAlignDtwThreads), 0, s, p);
}

// ------------------------------------------------------------------------------ word probabilities
// out[r] = logits[r][id[r]] - logsumexp(logits[r][0 .. n_ids)), one workgroup per row
__global__ __launch_bounds__(256) void row_id_logprob_kernel(const float* __restrict__ logits, long stride, int n_ids, const int* __restrict__ id,
                                                             float* __restrict__ out) {
  __shared__ float sh_m[4], sh_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (long)blockIdx.x * stride;
  float m = -INFINITY;
  for (int k = tid; k < n_ids; k += 256) m = fmaxf(m, row[k]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) sh_m[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
  float s = 0.f;
  for (int k = tid; k < n_ids; k += 256) s += expf(row[k] - m);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) sh_s[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const int t = id[blockIdx.x];
    out[blockIdx.x] = t >= 0 && t < n_ids ? row[t] - (m + logf(sh_s[0] + sh_s[1] + sh_s[2] + sh_s[3])) : -INFINITY;
  }
}

void launch_row_id_logprob(const float* logits, long stride, int n_ids, const int* id, int rows, float* out, hipStream_t s) {
  if (rows < 1) return;
  hipLaunchKernelGGL(row_id_logprob_kernel, dim3(rows), dim3(256), 0, s, logits, stride, n_ids, id, out);
}

}  // inline namespace AXW_NS
}  // namespace axw
