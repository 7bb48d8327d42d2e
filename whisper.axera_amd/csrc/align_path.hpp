// align_path.hpp — the path rule of word-level timestamps (DESIGN.md "Word-level timestamps"), defined ONCE for the host route
// (words.hpp: align_path) and the DTW kernel (decode_align.hip): which predecessor a cell of the cost table takes, and the walk
// back over the trace bytes. openai-whisper timing.py's dtw_cpu and backtrace. Plain C++: no HIP include, `__host__ __device__`
// only where the compiler is hipcc.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define AXW_ALIGN_FN __host__ __device__ inline
#else
#define AXW_ALIGN_FN inline
#endif

namespace axw {

// one trace byte per cell of the (rows + 1) x (frames + 1) table
constexpr uint8_t kTraceDiag = 0, kTraceUp = 1, kTraceLeft = 2;

// c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]; strict comparisons, so every tie (and every NaN) goes left
AXW_ALIGN_FN uint8_t dtw_choice(float c0, float c1, float c2) {
  if (c0 < c1 && c0 < c2) return kTraceDiag;
  if (c1 < c0 && c1 < c2) return kTraceUp;
  return kTraceLeft;
}

// trace [(n_rows + 1)][(n_frames + 1)] -> jump[i] = the frame of the first path point of row i. The border counts as left in row 0
// and up in column 0 whatever the array holds there, and a byte that is none of the three counts as left: the walk ends within
// n_rows + n_frames steps and writes inside jump whatever the bytes are.
AXW_ALIGN_FN void dtw_backtrace(const uint8_t* trace, int n_rows, int n_frames, int* jump) {
  const long W = (long)n_frames + 1;
  for (int i = 0; i < n_rows; ++i) jump[i] = 0;
  int i = n_rows, j = n_frames;
  while (i > 0 || j > 0) {
    if (i >= 1 && j >= 1) jump[i - 1] = j - 1;
    const uint8_t t = i == 0 ? kTraceLeft : j == 0 ? kTraceUp : trace[(long)i * W + j];
    if (t == kTraceDiag) { --i; --j; }
    else if (t == kTraceUp) --i;
    else --j;
  }
}

}  // namespace axw
