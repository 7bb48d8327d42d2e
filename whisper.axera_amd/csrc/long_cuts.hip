// long_cuts.hip — chunked long-form on gfx950 (DESIGN "Chunked long-form"; long_cuts.hpp: the definitions): where to cut a long file
// into windows of at most 30 s, chosen on the device from the file's own log-mel store, and the window kernel that ends a window at
// its cut. No model is involved: a cut goes to the quietest frame of a search range.
//
//   long_levels_kernel       store rows -> frame level e (mean over the mels of what the encoder will see) and smoothed level s
//                            (box of 2 R + 1 frames, index clamped to the file). One launch over a ragged batch of files.
//   long_cut_plan_kernel     the cut rule, one workgroup per file: per window a strided scan of the <= 1501 even candidates and a
//                            block arg-min on (value, frame); the next seek depends on it.
//   long_cut_compact_kernel  the files' windows -> one flat list in the order file-then-seek.
//   mel_window_cut_kernel    mel_window_kernel (mel_window.inc) with a length per window: zero from frame len on.
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

__device__ __forceinline__ float ordered_to_float(unsigned u) {  // FrontendParams::gmax's encoding (frontend.hip)
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// ---- levels. A workgroup owns kLevelTile frames of one file plus R frames on each side. LDS slot i holds e of frame
// clamp(t0 - R + i, 0, n_frames - 1), so the box sum of tile frame k is slots k .. k + 2 R and the clamp needs no second thought.
// A frame's row is read by the 16 lanes of a DPP row, 16 B per lane (a row of 128 mels in two steps of 256 B, four frames per wave
// instruction), and reduced inside that row. Store traffic is 1 + 2 R / 256 times the store: 1.2 at the default R = 25.
// The order of the fp32 sums (tests/long_cuts_reference.py derives its bound from it): a lane adds (x0 + x1) + (x2 + x3) of each of its
// 16-byte pieces in ascending order, the 16 lanes are added by a four-step butterfly, the sum is divided by n_mels; s adds its
// 2 R + 1 values of e in ascending frame order and divides by 2 R + 1.
constexpr int kLevelHalo = 64;
constexpr int kLevelSlots = kLevelTile + 2 * kLevelHalo;

__global__ __launch_bounds__(256) void long_levels_kernel(LongLevelsParams p) {
  __shared__ float lev[kLevelSlots];
  const int file = blockIdx.y, tid = threadIdx.x;
  const int n_frames = p.n_frames[file];
  const int t0 = blockIdx.x * kLevelTile;
  if (t0 >= n_frames) return;  // (uniform: a shorter file of the launch)
  const int R = p.smooth, nm = p.n_mels;
  const int n_tile = min(kLevelTile, n_frames - t0);
  const int n_slots = n_tile + 2 * R;
  const float floor_v = ordered_to_float(p.gmax[file]) - 8.0f;
  const long row0 = (long)p.frame_off[file];
  const int lane = tid & 15, group = tid >> 4;
  const int pieces = nm >> 2;  // 16-byte pieces of a row
  // two frames per 16-lane group and step: their loads are independent, so a lane has two to four 16-byte loads in flight
  for (int i0 = 0; i0 < n_slots; i0 += 32) {
    const int slot_a = i0 + group, slot_b = slot_a + 16;
    // always a row of the file, also for a slot beyond n_slots
    const float* row_a = p.store + (row0 + min(max(t0 - R + slot_a, 0), n_frames - 1)) * nm;
    const float* row_b = p.store + (row0 + min(max(t0 - R + slot_b, 0), n_frames - 1)) * nm;
    float acc_a = 0.f, acc_b = 0.f;
    for (int v = lane; v < pieces; v += 16) {
      f32x4 xa = *reinterpret_cast<const f32x4*>(row_a + 4 * v);
      f32x4 xb = *reinterpret_cast<const f32x4*>(row_b + 4 * v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xa[k] = (fmaxf(xa[k], floor_v) + 4.0f) * 0.25f;
        xb[k] = (fmaxf(xb[k], floor_v) + 4.0f) * 0.25f;
      }
      acc_a += (xa[0] + xa[1]) + (xa[2] + xa[3]);
      acc_b += (xb[0] + xb[1]) + (xb[2] + xb[3]);
    }
    acc_a = row16_sum(acc_a);
    acc_b = row16_sum(acc_b);
    if (lane == 0 && slot_a < n_slots) lev[slot_a] = acc_a / (float)nm;
    if (lane == 0 && slot_b < n_slots) lev[slot_b] = acc_b / (float)nm;
  }
  __syncthreads();
  if (tid < n_tile) {
    float sum = lev[tid];
    for (int j = 1; j <= 2 * R; ++j) sum += lev[tid + j];
    const long o = row0 + t0 + tid;
    p.s[o] = sum / (float)(2 * R + 1);
    if (p.e) p.e[o] = lev[tid + R];
  }
}

void launch_long_levels(const LongLevelsParams& p, hipStream_t s) {
  if (p.n_files < 1 || p.max_frames < 1 || p.smooth < 0 || p.smooth > kLevelHalo || p.n_mels < 8 || p.n_mels % 8 != 0) {
    fprintf(stderr, "[ax_whisper] launch_long_levels: bad parameters (files %d, frames %d, smooth %d, mels %d)\n", p.n_files, p.max_frames, p.smooth,
            p.n_mels);
    abort();
  }
  hipLaunchKernelGGL(long_levels_kernel, dim3((p.max_frames + kLevelTile - 1) / kLevelTile, p.n_files), dim3(256), 0, s, p);
}

// ---- the cut rule. (value, frame) pairs are ordered by value ascending, then frame descending: the smallest level wins, a tie goes
// to the latest frame. Levels are finite (long_cuts.hpp), so the order is total and the result does not depend on how the scan is
// split over the threads.
__device__ __forceinline__ void cut_better(float& bv, int& bi, float ov, int oi) {
  if (ov < bv || (ov == bv && oi > bi)) { bv = ov; bi = oi; }
}

__global__ __launch_bounds__(256) void long_cut_plan_kernel(LongCutPlanParams p) {
  __shared__ float wave_v[4];
  __shared__ int wave_i[4];
  const int file = blockIdx.x, tid = threadIdx.x;
  const int content = p.n_samples[file] / kHop;
  const float* s = p.s + p.frame_off[file];
  const int base = p.seg_off[file], room = p.seg_off[file + 1] - base;
  int seek = 0, count = 0;
  while (content - seek > p.w_max && count < room) {  // (uniform)
    const int lo = seek + p.w_min, hi = seek + p.w_max;  // hi <= content - 1: inside the file's levels
    float bv = __builtin_inff();
    int bi = -1;
    for (int f = lo + 2 * tid; f <= hi; f += 512) cut_better(bv, bi, s[f], f);
    for (int d = 32; d >= 1; d >>= 1) cut_better(bv, bi, __shfl_xor(bv, d), __shfl_xor(bi, d));
    if ((tid & 63) == 0) { wave_v[tid >> 6] = bv; wave_i[tid >> 6] = bi; }
    __syncthreads();
    bv = wave_v[0]; bi = wave_i[0];
    for (int k = 1; k < 4; ++k) cut_better(bv, bi, wave_v[k], wave_i[k]);
    __syncthreads();  // (the next window writes wave_v again)
    if (bi < lo) bi = hi;  // not reached with finite levels: whatever the input, the walk moves on and stays inside the file
    if (tid == 0) { p.seg_seek[base + count] = seek; p.seg_len[base + count] = bi - seek; }
    seek = bi;
    ++count;
  }
  if (tid == 0) {
    if (content > 0 && count < room) { p.seg_seek[base + count] = seek; p.seg_len[base + count] = content - seek; ++count; }
    p.n_windows[file] = count;
  }
}

__global__ __launch_bounds__(64) void long_cut_compact_kernel(LongCutPlanParams p) {
  const int file = blockIdx.x, tid = threadIdx.x;
  int before = 0;
  for (int g = tid; g < file; g += 64) before += p.n_windows[g];
  for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d);
  const int n = p.n_windows[file], base = p.seg_off[file];
  for (int k = tid; k < n; k += 64) {
    p.win_file[before + k] = file;
    p.win_seek[before + k] = p.seg_seek[base + k];
    p.win_len[before + k] = p.seg_len[base + k];
  }
}

void launch_long_cut_plan(const LongCutPlanParams& p, hipStream_t s) {
  if (p.n_files < 1 || p.w_min < 2 || p.w_max < p.w_min || p.w_max > kFramesOut || ((p.w_min | p.w_max) & 1)) {
    fprintf(stderr, "[ax_whisper] launch_long_cut_plan: bad parameters (files %d, window %d .. %d)\n", p.n_files, p.w_min, p.w_max);
    abort();
  }
  hipLaunchKernelGGL(long_cut_plan_kernel, dim3(p.n_files), dim3(256), 0, s, p);
  hipLaunchKernelGGL(long_cut_compact_kernel, dim3(p.n_files), dim3(64), 0, s, p);
}

// ---- the window that ends at its cut
constexpr int WF = 64;  // frames per workgroup, as in frontend.hip
#define AXW_MEL_WINDOW_KERNEL mel_window_cut_kernel
#define AXW_MEL_WINDOW_CUT 1
#include "mel_window.inc"
#undef AXW_MEL_WINDOW_KERNEL
#undef AXW_MEL_WINDOW_CUT

void launch_mel_window_cut(const MelWindowParams& p, const int* win_len, hipStream_t s) {
  const int lds = p.mel_ref ? WF * (p.n_mels + 1) * 4 : 0;
  hipLaunchKernelGGL(mel_window_cut_kernel, dim3((kFramesOut + WF - 1) / WF, p.n_windows), dim3(256), lds, s, p, win_len);
}

}  // inline namespace AXW_NS
}  // namespace axw
