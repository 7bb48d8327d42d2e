// resample.hip — polyphase sample-rate conversion to 16 kHz (DESIGN.md "Sample rates"; resample.hpp: the definition, the filter
// table and its constants; common.hpp: ResampleParams).
//
// resample_kernel: grid (tiles of the longest clip, clips), one workgroup of four waves per tile of kResampleTile consecutive
// outputs of one clip; workgroups beyond a clip's last tile leave at once.
//   1. the tile's input span [i0(first) - K + 1, i0(last) + K] goes to LDS: thread t loads samples t, t + 256, ... of the span
//      (consecutive lanes, consecutive addresses), zeros outside the clip. The span of every accepted rate fits kResampleSpan
//      (common.hpp); a descriptor whose span would not is skipped, never staged.
//   2. a table of up to kResampleLdsTable entries with more than one phase (8, 12, 24 kHz: 272 .. 544 entries) goes to LDS as well.
//   3. thread t computes output j = first + t: the 2 K products in tap order, fused multiply-adds in fp32, x from LDS at
//      (i0(j) - i0 of the span) + i. The coefficient row: L == 1 (32, 48, 96 kHz) is one row for every lane, read through a
//      wave-uniform pointer (scalar loads, the coefficient is an SGPR operand of the multiply-add); a small table from LDS
//      (lanes of equal phase read one address: a broadcast); a large one (44.1, 22.05, 11.025 kHz: 239 .. 348 KB) from global memory,
//      which the 4 MB L2 of an XCD holds. A large table is stored tap-major, [2 K][L] (resample_table_tap_major): at tap i the 64
//      lanes of a wave read 64 of the L entries of ONE row of 4 L bytes (640 bytes at 44.1 kHz), where the phase-major layout
//      has every lane on a cache line of its own, 1496 bytes apart. Measured at 44.1 kHz, 30 s clips: 5.12 ms against 5.81 ms per
//      64 clips, 0.087 ms against 0.064 ms for one clip (profiles/resample_bench.txt): the per-lane coefficient load itself, not
//      its layout, is what this path pays for (DESIGN.md "Sample rates" says what would remove it).
//   4. the output goes where the front-end reads it (row placement with the overflow rule, or packed).
// LDS banks of the x reads (32 banks of 4 bytes per 32-lane half): lanes step by M / L samples, so an odd M at L == 1 (48 kHz: 3)
// is conflict-free, an even one (32 kHz: 2, 96 kHz: 6) two-way; not measured with counters.
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

template <class H>
__device__ __forceinline__ float resample_dot(const float* x, H h, int T) {
  float acc = 0.f;
  int i = 0;
  for (; i + 4 <= T; i += 4) {
    acc = fmaf(x[i], h[i], acc);
    acc = fmaf(x[i + 1], h[i + 1], acc);
    acc = fmaf(x[i + 2], h[i + 2], acc);
    acc = fmaf(x[i + 3], h[i + 3], acc);
  }
  for (; i < T; ++i) acc = fmaf(x[i], h[i], acc);
  return acc;
}

// the same sum with the coefficients `stride` floats apart (a tap-major table: h = the phase's column)
__device__ __forceinline__ float resample_dot_strided(const float* x, const float* h, int T, int stride) {
  float acc = 0.f;
  int i = 0;
  for (; i + 4 <= T; i += 4) {
    const float h0 = h[(long)i * stride], h1 = h[(long)(i + 1) * stride], h2 = h[(long)(i + 2) * stride], h3 = h[(long)(i + 3) * stride];
    acc = fmaf(x[i], h0, acc);
    acc = fmaf(x[i + 1], h1, acc);
    acc = fmaf(x[i + 2], h2, acc);
    acc = fmaf(x[i + 3], h3, acc);
  }
  for (; i < T; ++i) acc = fmaf(x[i], h[(long)i * stride], acc);
  return acc;
}

__global__ __launch_bounds__(kResampleTile) void resample_kernel(const ResampleParams p) {
  __shared__ float xs[kResampleSpan];
  __shared__ float hs[kResampleLdsTable];
  const int b = blockIdx.y, tid = threadIdx.x;
  const ResampleClip c = p.clips[b];
  const long j0 = (long)blockIdx.x * kResampleTile;
  if (j0 >= c.n_out) return;
  const int nj = min((long)kResampleTile, (long)c.n_out - j0);
  const int L = c.L, M = c.M, K = c.K, T = 2 * K;
  // j < 2^29 and M <= 384: j M fits 64 bits with room; j M >= 0, so / and % are floor and mod
  const long base0 = (j0 * M) / L;
  const long first = base0 - K + 1;
  const long last = ((j0 + nj - 1) * M) / L + K;
  const long span = last - first + 1;
  if (span > kResampleSpan) return;
  const float* in = p.in + c.in_off;
  for (long i = tid; i < span; i += kResampleTile) {
    const long g = first + i;
    xs[i] = (g >= 0 && g < c.n_in) ? in[g] : 0.f;
  }
  const float* tab = p.tables + c.tab_off;
  const bool tab_lds = L > 1 && L * T <= kResampleLdsTable;
  if (tab_lds)
    for (int i = tid; i < L * T; i += kResampleTile) hs[i] = tab[i];
  __syncthreads();
  if (tid >= nj) return;
  const long j = j0 + tid;
  const long jm = j * M;
  const int r = (int)(jm % L);
  const float* x = xs + (int)(jm / L - base0);  // = (i0(j) - K + 1) - first
  float y;
  if (L == 1) y = resample_dot(x, tab, T);
  else if (tab_lds) y = resample_dot(x, hs + r * T, T);
  else y = resample_dot_strided(x, tab + r, T, L);
  if (p.stride > 0) {
    if (j < p.stride) p.out[(long)c.row * p.stride + j] = y;
    else p.overflow[p.over_off[c.row] + j - p.stride] = y;
  } else {
    p.out[c.out_off + j] = y;
  }
}

void launch_resample(const ResampleParams& p, hipStream_t s) {
  if (p.batch < 1 || p.max_out < 1) return;
  if (!p.in || !p.tables || !p.clips || !p.out || p.stride < 0 || p.batch > 65535) {
    fprintf(stderr, "[ax_whisper] launch_resample: bad parameters (batch %d, stride %d)\n", p.batch, p.stride);
    abort();  // fail loudly: there is no fallback path
  }
  const int tiles = (p.max_out + kResampleTile - 1) / kResampleTile;
  hipLaunchKernelGGL(resample_kernel, dim3(tiles, p.batch), dim3(kResampleTile), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
