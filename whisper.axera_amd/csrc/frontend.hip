// frontend.hip — log-mel front-end on gfx950 (K1/K2 of SURVEY §8a).
//
// Replaces librosa::Feature::melspectrogram (cpp/src/librosa/librosa.h:46-155) and the
// clamp/normalise/pad of Whisper::preprocess (cpp/src/Whisper.cpp:151-184):
//   reflect pad 200 | periodic Hann | 400-pt DFT bins 0..200 | re^2+im^2 | Slaney mel GEMM |
//   log10(max(.,1e-10)) | global max over ALL frames | max(., gmax-8) | (.+4)/4 | zero-fill to 3000
// "ALL frames" means all frames of the input however long it is (Whisper.cpp:158-172 takes the maximum before it
// truncates to 3000 frames): the grid covers every frame of the longest clip, frames past 3000 only feed the maximum.
//
// Kernel 1 (stft_mel_kernel): one workgroup = 32 consecutive frames of one clip. The windowed frames are staged in
// LDS ([32][401] f32, 51 KB) and the 400-point DFT runs on the matrix cores as an exact-fp32 GEMM
//   [32 frames x 400 samples] . [400 x (cos | sin) of 224 bins]     (v_mfma_f32_32x32x2_f32, fp32 in, fp32 accumulate:
// the arithmetic class of the FMA loop it replaces — rounds 1-3 evaluated the DFT with 64 scalar accumulators per lane at
// 0.18 of the fp32 vector peak); the twiddle operand is never materialised: a lane walks a 400-entry (cos, sin) table in
// LDS with its own stride (k * bin mod 400). The power spectrum goes back to LDS and the mel projection + log10 + clip
// maximum are fused in.
// Kernel 2 (mel_normalize_kernel): clamp/scale/zero-fill and layout: time-major h16 rows for the
// encoder's conv-as-GEMM (and the reference's [n_mels][3000] f32 layout when a caller asks for it).
// HBM traffic per clip: 1.92 MB PCM in, 0.96 MB log-mel scratch out+in, 0.48 MB h16 out.
// Long-form (whole files, DESIGN "Long-form"): stft_mel_long_kernel keeps every frame's row in a per-file store, and
// mel_window_kernel cuts the 30 s window at a file's seek out of it into an encoder slot.
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

constexpr int FR = 32;        // frames per workgroup = rows of one MFMA tile
constexpr int PW_LD = 209;    // power row stride in LDS: odd (column reads of the mel GEMM), >= 202 (bins padded to an even count)
constexpr int XS = kNFFT + 1; // row stride of the staged frames: odd, so a column read (32 frames, one sample) hits 32 banks
constexpr int kBinGroups = (kBins + 31) / 32;  // 7 groups of 32 bins

__device__ __forceinline__ unsigned float_to_ordered(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_float(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// the kernel's text lives in frontend_stft.inc: once for clips, once for whole files
#define AXW_STFT_KERNEL stft_mel_kernel
#define AXW_STFT_LONG 0
#include "frontend_stft.inc"
#undef AXW_STFT_KERNEL
#undef AXW_STFT_LONG
#define AXW_STFT_KERNEL stft_mel_long_kernel
#define AXW_STFT_LONG 1
#include "frontend_stft.inc"
#undef AXW_STFT_KERNEL
#undef AXW_STFT_LONG

// Whisper.cpp:169-181: max(., mmax-8), (.+4)/4, rows resized to 3000 with zero fill.
__global__ __launch_bounds__(256) void mel_normalize_kernel(FrontendParams p) {
  const int b = blockIdx.y;
  const int nm = p.n_mels;
  const int n_frames = p.openai ? kFramesOut : min(1 + p.n_samples[b] / kHop, kFramesOut);
  const float floor_v = ordered_to_float(p.gmax[b]) - 8.0f;
  const long total = (long)kFramesOut * nm;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int f = (int)(i / nm), m = (int)(i - (long)f * nm);
    float v = 0.f;
    if (f < n_frames) v = (fmaxf(p.logmel[(long)b * total + i], floor_v) + 4.0f) * 0.25f;
    if (p.mel_ref) p.mel_ref[((long)b * nm + m) * kFramesOut + f] = v;
    if (p.mel_tm) p.mel_tm[((long)b * p.mel_rows + f + 1) * nm + m] = (h16)v;  // row 0 = conv left pad
  }
}

// host-supplied mel [B][n_mels][3000] f32 -> encoder input layout (used by AX_WHISPER_EncodeMel)
__global__ __launch_bounds__(256) void mel_to_tm_kernel(const float* __restrict__ mel_ref, h16* __restrict__ mel_tm, int n_mels,
                                                        int mel_rows) {
  const int b = blockIdx.y;
  const long total = (long)kFramesOut * n_mels;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int f = (int)(i / n_mels), m = (int)(i - (long)f * n_mels);
    mel_tm[((long)b * mel_rows + f + 1) * n_mels + m] = (h16)mel_ref[((long)b * n_mels + m) * kFramesOut + f];
  }
}

__global__ void gmax_reset_kernel(unsigned* gmax, int batch) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < batch) gmax[i] = 0u;  // below every ordered-encoded float
}

void launch_frontend(const FrontendParams& p, hipStream_t s) {
  hipLaunchKernelGGL(gmax_reset_kernel, dim3((p.batch + 63) / 64), dim3(64), 0, s, p.gmax, p.batch);
  const int lds = FR * XS * 4 + kNFFT * 8;
  dim3 grid((p.max_frames + FR - 1) / FR, p.batch);
  // basis is passed transposed ([201][n_mels]) by the engine in p.mel_basis
  hipLaunchKernelGGL(stft_mel_kernel, grid, dim3(256), lds, s, p, p.mel_basis);
  hipLaunchKernelGGL(mel_normalize_kernel, dim3(64, p.batch), dim3(256), 0, s, p);
}

// ---- long-form: one 30 s window of a file's log-mel store -> encoder slot a (DESIGN "Long-form"). The kernel's text lives in
// mel_window.inc: once here, once in long_cuts.hip for a window that ends at a cut.
constexpr int WF = 64;  // frames per workgroup
#define AXW_MEL_WINDOW_KERNEL mel_window_kernel
#define AXW_MEL_WINDOW_CUT 0
#include "mel_window.inc"
#undef AXW_MEL_WINDOW_KERNEL
#undef AXW_MEL_WINDOW_CUT

void launch_frontend_long(const FrontendParams& p, const LongStoreParams& ls, hipStream_t s) {
  hipLaunchKernelGGL(gmax_reset_kernel, dim3((p.batch + 63) / 64), dim3(64), 0, s, p.gmax, p.batch);
  const int lds = FR * XS * 4 + kNFFT * 8;
  dim3 grid((p.max_frames + FR - 1) / FR, p.batch);
  hipLaunchKernelGGL(stft_mel_long_kernel, grid, dim3(256), lds, s, p, p.mel_basis, ls);
}

void launch_mel_window(const MelWindowParams& p, hipStream_t s) {
  const int lds = p.mel_ref ? WF * (p.n_mels + 1) * 4 : 0;
  hipLaunchKernelGGL(mel_window_kernel, dim3((kFramesOut + WF - 1) / WF, p.n_windows), dim3(256), lds, s, p);
}

void launch_mel_to_tm(const float* mel_ref, h16* mel_tm, int batch, int n_mels, int mel_rows, hipStream_t s) {
  hipLaunchKernelGGL(mel_to_tm_kernel, dim3(64, batch), dim3(256), 0, s, mel_ref, mel_tm, n_mels, mel_rows);
}

}  // inline namespace AXW_NS
}  // namespace axw
