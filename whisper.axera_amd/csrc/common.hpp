// common.hpp — shared device helpers and the launch interface of the HIP kernels (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_layout.hpp"
#include "vocab_logprob_plan.hpp"

// ------------------------------------------------------------------ the 16-bit storage / MFMA operand type
// Every kernel file and the engine are compiled TWICE (Makefile): -DAXW_F16=0 -> bfloat16 (the default; what
// BASELINE configs[1], [2], [4] name), -DAXW_F16=1 -> IEEE half (configs[3]: "Whisper-turbo fp16"; also the dtype
// OpenAI's and HF's checkpoints are published in, so their weights load without a rounding step). Everything that
// depends on the type lives in the inline namespace axw::bf / axw::hf — same source, two sets of symbols — and the C ABI
// (api.cpp) picks one per model from the dtype of its weights file. `h16` is that type: weights, MFMA operands,
// K/V caches and the (hi, lo) activation pairs of the batched decoder. Accumulation, LayerNorm, softmax, GELU, the
// residual stream and the logits are fp32 in both builds.
#ifndef AXW_F16
#define AXW_F16 0
#endif
#if AXW_F16
#define AXW_NS hf
#else
#define AXW_NS bf
#endif

namespace axw {
inline namespace AXW_NS {

#if AXW_F16
typedef _Float16 h16;
constexpr const char* kDtypeName = "fp16";
#else
typedef __bf16 h16;
constexpr const char* kDtypeName = "bf16";
#endif
typedef h16 h16x4 __attribute__((ext_vector_type(4)));
typedef h16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // 16-byte staging register (HIP's uint4 struct can end up in scratch)
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kNFFT = 400;
constexpr int kHop = 160;
constexpr int kBins = 201;
constexpr int kFramesOut = 3000;   // Whisper.cpp:172 resize(3000)

// ------------------------------------------------------------------ device helpers
#ifdef __HIPCC__
// the two h16 values packed in one dword (element 2i in the low half), widened to fp32: one shift / one mask for
// bfloat16; v_cvt_f32_f16 (folded into v_fma_mix_f32 where the value feeds an FMA) for half
#if AXW_F16
typedef _Float16 axw_half2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float h16lo(unsigned u) { return (float)__builtin_bit_cast(axw_half2, u)[0]; }
__device__ __forceinline__ float h16hi(unsigned u) { return (float)__builtin_bit_cast(axw_half2, u)[1]; }
#define AXW_MFMA_32x32x16(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B, C, 0, 0, 0)
#define AXW_MFMA_16x16x32(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, C, 0, 0, 0)
#else
__device__ __forceinline__ float h16lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float h16hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
#define AXW_MFMA_32x32x16(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, C, 0, 0, 0)
#define AXW_MFMA_16x16x32(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, C, 0, 0, 0)
#endif
// fp32 accumulate of a 2-element dot product of packed h16 pairs (v_dot2c_f32_bf16 / v_dot2c_f32_f16), and the split of
// two fp32 values into packed (hi, lo) h16 pairs: x = hi + lo to 16 (bfloat16) / 22 (half) significant bits
#if AXW_F16
__device__ __forceinline__ float h16dot2(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(axw_half2, a), __builtin_bit_cast(axw_half2, b), c, false);
}
#else
typedef __bf16 axw_bf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float h16dot2(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(axw_bf2, a), __builtin_bit_cast(axw_bf2, b), c, false);
}
#endif
__device__ __forceinline__ void h16split2(float x0, float x1, unsigned& hi, unsigned& lo) {
  const h16 h0 = (h16)x0, h1 = (h16)x1;
  const h16 l0 = (h16)(x0 - (float)h0), l1 = (h16)(x1 - (float)h1);
  hi = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
  lo = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
}
// sum / maximum over the wave in every lane (all 64 lanes active): DPP butterflies inside a 16-lane row, then
// v_permlane{16,32}_swap across rows — ~8 short vector instructions; the __shfl_xor form compiles to six dependent
// ds_bpermute round trips (~700 cycles of latency per call, which bounded the K/V block loop of decode_attention_kernel)
#define AXW_DPP_F(CTRL, X) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(X), CTRL, 0xf, 0xf, true))
// sum over the 16 lanes of a DPP row (equal lane >> 4), in every lane of the row: the four butterfly steps
__device__ __forceinline__ float row16_sum(float v) {
  v += AXW_DPP_F(0xB1, v);   // quad_perm [1,0,3,2]
  v += AXW_DPP_F(0x4E, v);   // quad_perm [2,3,0,1]
  v += AXW_DPP_F(0x141, v);  // row_half_mirror
  v += AXW_DPP_F(0x140, v);  // row_mirror
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, AXW_DPP_F(0xB1, v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, AXW_DPP_F(0x4E, v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, AXW_DPP_F(0x141, v));  // row_half_mirror
  v = fmaxf(v, AXW_DPP_F(0x140, v));  // row_mirror
#undef AXW_DPP_F
  {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  return v;
}
// THE argmax tie rule, "first maximum wins" (std::max_element, Whisper.cpp:42-45): candidate (ov, oi) replaces (v, i) when it is
// greater, or equal with the lower index. A NaN candidate never wins. Every merge of argmax candidates goes through here.
__device__ __forceinline__ void argmax_take(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// (value, index) maximum over the 16 lanes of a DPP row in every lane of the row: the four butterfly steps
__device__ __forceinline__ void row16_argmax(float& v, int& idx) {
#define AXW_DPP_I(CTRL, X) __builtin_amdgcn_update_dpp(0, X, CTRL, 0xf, 0xf, true)
#define AXW_ARGMAX_STEP(CTRL) { const float ov = __int_as_float(AXW_DPP_I(CTRL, __float_as_int(v))); const int oi = AXW_DPP_I(CTRL, idx); argmax_take(v, idx, ov, oi); }
  AXW_ARGMAX_STEP(0xB1)   // quad_perm [1,0,3,2]
  AXW_ARGMAX_STEP(0x4E)   // quad_perm [2,3,0,1]
  AXW_ARGMAX_STEP(0x141)  // row_half_mirror
  AXW_ARGMAX_STEP(0x140)  // row_mirror
#undef AXW_ARGMAX_STEP
#undef AXW_DPP_I
}
// (value, index) maximum over the wave in every lane, lower index on equal values; DPP butterflies inside a 16-lane row,
// v_permlane{16,32}_swap across rows (the __shfl_xor form: twelve dependent ds_bpermute round trips)
__device__ __forceinline__ void wave_argmax(float& v, int& idx) {
  row16_argmax(v, idx);
  {
    auto rv = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    auto ri = __builtin_amdgcn_permlane16_swap((unsigned)idx, (unsigned)idx, false, false);
    v = __uint_as_float(rv[0]); idx = (int)ri[0];
    argmax_take(v, idx, __uint_as_float(rv[1]), (int)ri[1]);
  }
  {
    auto rv = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    auto ri = __builtin_amdgcn_permlane32_swap((unsigned)idx, (unsigned)idx, false, false);
    v = __uint_as_float(rv[0]); idx = (int)ri[0];
    argmax_take(v, idx, __uint_as_float(rv[1]), (int)ri[1]);
  }
}
// GEPI_QKV_CACHE, one output y of row n for the clip with index b among the launch's per-clip pointers: the q row, or the
// self-attention K (blocked) / V (row-major) cache append at row `key` = the clip's own offset (export_onnx.py:245-247,
// Whisper.cpp:328-342). P: GemvParams, DecGemmParams or DecCGemmParams (rows n < 3 d_model; `key` is not used for n < d_model).
template <class P>
__device__ __forceinline__ void store_qkv_cache(const P& p, int b, int n, float y, int key) {
  const int d = p.d_model;
  if (n < d) {
    p.out[(long)b * d + n] = y;
  } else {
    const int c = (n < 2 * d) ? n - d : n - 2 * d;
    const int head = c >> 6, dd = c & 63;
    const long base = (long)b * p.kv_batch_stride + head * layout::kv_head_elems(p.n_ctx_pad);
    if (n < 2 * d) p.k_cache[base + layout::k_index(key, dd)] = (h16)y;
    else p.v_cache[base + layout::v_index(key, dd)] = (h16)y;
  }
}

// exact-erf GELU (nn.GELU default; export_onnx.py:158-159 F.gelu)
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
// The same GELU with erf from Abramowitz-Stegun 7.1.26 (|erf error| <= 1.5e-7, i.e. far below one h16 ulp of the
// result): 1 rcp + 1 exp + 6 FMA instead of libm erff's ~60 instructions. Used where the result is narrowed to h16.
__device__ __forceinline__ float gelu_erf_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __frcp_rn(fmaf(0.3275911f, z, 1.f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float e = 1.f - poly * __expf(-z * z);
  return 0.5f * x * (1.f + copysignf(e, x));
}
#endif

// Two values at once with packed fp32 arithmetic (v_pk_fma_f32 / v_pk_mul_f32) and the hardware reciprocal (1 ulp; the
// correctly rounded __frcp_rn above expands to a division sequence of ~10 instructions): 2 rcp + 2 exp + ~12 packed ops
// per PAIR. In the mlp.0 epilogue of the encoder the GELU arithmetic is comparable to the tile's MFMA time.
#ifdef __HIPCC__
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t gelu_erf_fast2(f32x2_t x) {
  // 0.5 x (1 + erf(x / sqrt 2)) = 0.5 x + |x| (0.5 - 0.5 poly(t) exp(-x^2 / 2)),  t = 1 / (1 + p |x| / sqrt 2): erf is odd, so
  // the sign needs no copysign; 1/sqrt 2, the 0.5 and log2(e) are folded into the constants (17 instructions per pair)
  const f32x2_t ax = {fabsf(x[0]), fabsf(x[1])};
  const f32x2_t den = ax * (0.3275911f * 0.70710678118654752440f) + 1.f;
  const f32x2_t t = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  f32x2_t poly = t * (0.5f * 1.061405429f) + (0.5f * -1.453152027f);
  poly = poly * t + (0.5f * 1.421413741f);
  poly = poly * t + (0.5f * -0.284496736f);
  poly = poly * t + (0.5f * 0.254829592f);
  poly = poly * t;
  const f32x2_t u = ax * 0.84932180028801904272f;  // sqrt(0.5 log2 e): exp(-x^2 / 2) = exp2(-u^2)
  const f32x2_t mu2 = -u * u;
  const f32x2_t ex = {__builtin_amdgcn_exp2f(mu2[0]), __builtin_amdgcn_exp2f(mu2[1])};
  const f32x2_t e = 0.5f - poly * ex;
  return ax * e + x * 0.5f;
}
#endif

// ------------------------------------------------------------------ GEMM (encoder)
// C[M,N] = A[M,K] (h16, row stride lda, rows may overlap) * W[N,K]^T (h16) with a fused epilogue.
enum GemmEpilogue : int {
  EPI_BIAS_BF16 = 0,       // C h16 = acc + bias
  EPI_BIAS_GELU_BF16 = 1,  // C h16 = gelu(acc + bias)
  EPI_GELU_POS_F32 = 2,    // C f32  = gelu(acc + bias) + aux[m][n]      (conv2 + positional embedding)
  EPI_RESID_F32 = 3,       // C f32 += acc + bias                        (out-proj / FFN2 residual)
  EPI_QKV = 4,             // n<d: Q h16 [m][d]; d<=n<2d: K h16 [m][d]; else V^T h16 [h][64][Tp]
  EPI_CROSS_KV = 5,        // decode layouts: K blocked [l][b][h][blk][8][64][8], V [l][b][h][Tp][64]
  EPI_PARTIAL_F32 = 6,     // split-K: part[split][batch*M + m][n] f32 = acc over this split's k range (no bias); the
                           // LayerNorm that follows folds the partials (+ bias) into the residual stream, in fixed order
};

struct GemmParams {
  const h16* A; long lda; long a_batch_stride;
  const h16* W;                     // [N][K]
  const float* bias;                 // [N] fp32
  void* C; long ldc; long c_batch_stride;
  const float* aux;                  // EPI_GELU_POS_F32: pos [M][N]
  void* C2; void* C3;                // EPI_QKV: K, V^T ; EPI_CROSS_KV: C=K blocked, C2=V
  long c2_batch_stride, c3_batch_stride;
  int M, N, K, batch;
  int d_model;                       // EPI_QKV / EPI_CROSS_KV
  int t_pad;                         // padded key count (multiple of 64)
  int n_batch_total;                 // EPI_CROSS_KV: slot count B in [l][B][h]...
  const int* kv_slot_map;            // EPI_CROSS_KV: clip b of this launch -> slot kv_slot_map[b] (device), nullptr: slot b
  int n_layer;                       // EPI_CROSS_KV: decoder layers (weight rows: all K, then all V)
  int n_begin;                       // set by launch_gemm: first output column of this launch
  int n_tiles;                       // set by launch_gemm: 128-column tiles of this launch
  int epilogue;
  int qkv_part;                      // EPI_QKV: 0 both launches, 1 only Q,K columns, 2 only V columns (run side by side on two streams)
  int ksplit;                        // EPI_PARTIAL_F32: K slices (grid.y), K / 64 divisible by it
  float* part; long part_stride;     // EPI_PARTIAL_F32: partial sums, one [batch*M][N] slab per slice
};
void launch_gemm(const GemmParams& p, hipStream_t s);

// fp32 [rows][d] -> h16 [rows][d] LayerNorm (eps 1e-5)
// n_part > 0: first x[row] += bias + part[0][row] + ... + part[n_part-1][row] (split-K partials of the GEMM before, slab
// stride part_stride), written back to x
void launch_layernorm_bf16(float* x, const float* g, const float* b, h16* y, long rows, int d, hipStream_t s,
                           const float* part = nullptr, int n_part = 0, long part_stride = 0, const float* part_bias = nullptr);

// encoder self-attention (non-causal, T keys), Q/K h16 [B][T][d], V^T h16 [B][H][64][Tp] (frames of every 16-group in
// the order [0-3, 8-11, 4-7, 12-15], as EPI_QKV writes them) -> O h16 [B][T][d]. rescale_thr: how far (log2 units) a
// tile's row maximum may exceed the running one before the accumulators are rescaled; 0 = on every increase.
void launch_encoder_attention(const h16* q, const h16* k, const h16* vt, h16* o, int batch, int T, int t_pad,
                              int d_model, int n_head, hipStream_t s, float rescale_thr = 8.f);

// ------------------------------------------------------------------ front-end
struct FrontendParams {
  const float* pcm;        // device [batch][stride]
  int stride;
  const int* n_samples;    // device [batch]
  int batch, n_mels;
  const float* twiddle;    // device [400][2] cos,sin
  const float* window;     // device [400]
  const float* mel_basis;  // device [n_mels][201]
  float* power;            // unused: read by no kernel, set by no caller (the power spectrum stays in LDS)
  float* logmel;           // device scratch [batch][3000][n_mels]: log10 of the mel sums, before clamp and scale
  unsigned* gmax;          // device [batch] (float bits, ordered-int encoded)
  float* mel_ref;          // device [batch][n_mels][3000] f32 (reference layout) or nullptr
  h16* mel_tm;            // device [batch][mel_rows][n_mels] h16 time-major, row 0 = left pad, or nullptr
  int mel_rows;
  int max_frames;          // frames computed per clip (<= 3001)
  const float* overflow;   // samples beyond `stride` of clips longer than the staging row (device, packed), or nullptr:
  const long long* over_off;  //   sample j >= stride of clip b is overflow[over_off[b] + j - stride] (device [batch])
  int openai;              // 1: the fp32 ONNX lineage's front-end (SURVEY A.1 column 3, generate_data.py:162-176): clip
                           // zero-padded / trimmed to 30 s before the STFT, last frame dropped, no zero fill
};
void launch_frontend(const FrontendParams& p, hipStream_t s);
void launch_mel_to_tm(const float* mel_ref, h16* mel_tm, int batch, int n_mels, int mel_rows, hipStream_t s);

// long-form (DESIGN "Long-form"): the front-end over whole files. FrontendParams carries pcm (the base the offsets below count
// from), n_samples / gmax [n_files], batch = n_files, max_frames = frames of the longest file, the constants; stride, logmel,
// mel_*, overflow and openai are not read.
struct LongStoreParams {
  const long long* pcm_off;    // device [n_files]: file b's samples are pcm[pcm_off[b] ...]
  const long long* frame_off;  // device [n_files]: file b's rows are store[frame_off[b] ...]
  float* store;                // device [sum of 1 + n_samples / 160][n_mels] fp32 log-mel, before clamp and scale
};
void launch_frontend_long(const FrontendParams& p, const LongStoreParams& ls, hipStream_t s);
// window a of a pass = rows [win_seek[a], win_seek[a] + 3000) of file win_file[a] -> encoder slot a
struct MelWindowParams {
  const float* store;
  const long long* frame_off;  // device [n_files]
  const int* n_frames;         // device [n_files]: rows the file has in the store
  const unsigned* gmax;        // device [n_files] (ordered-int encoded, as FrontendParams::gmax)
  const int* win_file;         // device [n_windows]
  const int* win_seek;         // device [n_windows], 0 <= seek
  h16* mel_tm;                 // device [n_windows][mel_rows][n_mels] or nullptr
  float* mel_ref;              // device [n_windows][n_mels][3000] or nullptr
  int mel_rows, n_mels, n_windows;
};
void launch_mel_window(const MelWindowParams& p, hipStream_t s);

// ------------------------------------------------------------------ chunked long-form (long_cuts.hip; long_cuts.hpp: the definitions)
constexpr int kLevelTile = 256;  // frames of one file per workgroup of the levels kernel; its LDS holds the tile + 64 frames each side
// One launch over a ragged batch of files: e[f] = mean over the mels of what the encoder will see of store row f, s[f] = the mean of
// e over [f - R, f + R] with the index clamped to the file. Both are written at frame_off[file] + f, as the store's rows are.
struct LongLevelsParams {
  const float* store;
  const long long* frame_off;  // device [n_files]
  const int* n_frames;         // device [n_files]
  const unsigned* gmax;        // device [n_files] (ordered-int encoded)
  float* s;                    // device [sum of n_frames]
  float* e;                    // device [sum of n_frames] or nullptr
  int n_mels, n_files, smooth; // smooth = R, 0 .. 64; n_mels a multiple of 8
  int max_frames;              // frames of the longest file (grid.x = its tiles)
};
void launch_long_levels(const LongLevelsParams& p, hipStream_t s);
// The cut rule on the device, one workgroup per file, then the compaction into the flat order file-then-seek. File b's windows are
// first written to seg_seek / seg_len [seg_off[b] ...) (room for cut_plan_capacity of them), its count to n_windows[b]; the second
// kernel moves them to win_file / win_seek / win_len [sum of the counts], which mel_window_cut_kernel reads.
struct LongCutPlanParams {
  const float* s;              // device: the smoothed levels, file b's at frame_off[b] ...
  const long long* frame_off;  // device [n_files]
  const int* n_samples;        // device [n_files]: content = n_samples / 160
  const int* seg_off;          // device [n_files + 1]: file b's room is seg_off[b + 1] - seg_off[b] windows
  int *seg_seek, *seg_len;     // device [seg_off[n_files]]
  int* n_windows;              // device [n_files]
  int *win_file, *win_seek, *win_len;  // device [seg_off[n_files]]
  int n_files, w_min, w_max;
};
void launch_long_cut_plan(const LongCutPlanParams& p, hipStream_t s);
// launch_mel_window for windows that end at a cut: window a holds win_len[a] frames, zero from there on
void launch_mel_window_cut(const MelWindowParams& p, const int* win_len, hipStream_t s);

// ------------------------------------------------------------------ sample-rate conversion (resample.hip; DESIGN.md "Sample rates")
// One launch over a ragged batch of clips, each at its own rate: y_j = sum over i < 2 K of x[i0 + i - K + 1] H[r][i] with
// i0 = floor(j M / L), r = (j M) mod L, x zero outside the clip (resample.hpp: the definition and the table H [L][2 K]).
constexpr int kResampleTile = 256;        // consecutive outputs of one clip per workgroup, one per thread
// LDS floats for a tile's input span [i0(first) - K + 1, i0(last) + K]: at most ceil(255 M / L) + 2 K, and M / L <= 24 (384 kHz),
// K <= ceil(64 * 24 / ROLLOFF) = 1621 for every accepted rate, so 6120 + 3242 = 9362 is the widest: one staging pass always fits
constexpr int kResampleSpan = 9472;
constexpr int kResampleLdsTable = 2048;   // tables of up to this many entries (8, 12, 24 kHz) are read from LDS, larger ones through L2
// A table on the device is H [L][2 K] as resample.hpp defines it, except a table with more than one phase that does not fit
// kResampleLdsTable: that one is stored tap-major, [2 K][L] (lanes of a wave then read neighbouring entries; resample.hip)
inline bool resample_table_tap_major(int L, int K) { return L > 1 && (long)L * 2 * K > kResampleLdsTable; }
struct ResampleClip {       // device, one per clip of the launch
  long long in_off;         // the clip's samples are in[in_off ... in_off + n_in)
  long long out_off;        // packed placement: output j goes to out[out_off + j]
  long long tab_off;        // the clip's table is tables[tab_off ... tab_off + L * 2 K), in the layout resample_table_tap_major says
  int n_in, n_out;          // 1 <= n_in, n_out = ceil(n_in L / M)
  int L, M, K;
  int row;                  // row placement: the clip's staging row
};
struct ResampleParams {
  const float* in; const float* tables;
  const ResampleClip* clips;  // device [batch]
  int batch;
  float* out;
  // stride > 0, row placement (the engine's staging rows, FrontendParams::overflow / over_off): output j of a clip goes to
  // out[row * stride + j] for j < stride, else to overflow[over_off[row] + j - stride]; stride == 0: packed placement
  int stride;
  float* overflow; const long long* over_off;
  int max_out;                // the largest n_out of the launch (grid.x = its tiles)
};
inline bool resample_shape_ok(int L, int M, int K) {  // what the kernel takes: the widest span of a tile fits its LDS
  return L >= 1 && M >= 1 && K >= 1 && ((long)(kResampleTile - 1) * M + L - 1) / L + 2L * K <= kResampleSpan;
}
void launch_resample(const ResampleParams& p, hipStream_t s);

// ------------------------------------------------------------------ decoder
struct DecState {          // device-resident loop state, one per engine
  int step;                // decoder steps run since the last reset (bookkeeping; no kernel derives a position from it)
  int n_done;
  int pad0, pad1;
};
// Every utterance slot has its OWN offset (`off[b]`: the position fed to this step = number of cached self-attention keys
// = the `offset` input of the reference's decoder graph, export_onnx.py:312-336 / Whisper.cpp:207-222, which handles one
// utterance at a time and so has one): slots of one batch may be at different positions, a finished slot stops
// advancing, and a new clip can be admitted into it while the others decode on (Engine::stream_*). Kernel parameter
// structs carry `off` with the same clip origin as their other per-clip pointers.

struct DecLayerW {
  const float *attn_ln_w, *attn_ln_b, *cross_ln_w, *cross_ln_b, *mlp_ln_w, *mlp_ln_b;
  const h16 *w_qkv, *w_o, *w_cq, *w_co, *w_fc1, *w_fc2;
  const float *b_qkv, *b_o, *b_cq, *b_co, *b_fc1, *b_fc2;
};

// Layout of the decoder-layer weight arenas (engine.cpp load_weights): layer l's h16 matrices start at
// w_base + l * w_stride(d), in units of d*d elements; its fp32 vectors at f_base + l * f_stride(d), in units of d.
struct DecArena {
  enum : int { W_QKV = 0, W_O = 3, W_CQ = 4, W_CO = 5, W_FC1 = 6, W_FC2 = 10, W_UNITS = 14 };
  enum : int { F_ATTN_LN_W = 0, F_ATTN_LN_B = 1, F_B_QKV = 2, F_B_O = 5, F_CROSS_LN_W = 6, F_CROSS_LN_B = 7, F_B_CQ = 8, F_B_CO = 9,
               F_MLP_LN_W = 10, F_MLP_LN_B = 11, F_B_FC1 = 12, F_B_FC2 = 16, F_UNITS = 17 };
  static constexpr __host__ __device__ long w_stride(int d) { return (long)W_UNITS * d * d; }
  static constexpr __host__ __device__ long f_stride(int d) { return (long)F_UNITS * d; }
};

enum GemvPrologue : int { PRO_PLAIN = 0, PRO_LAYERNORM = 1, PRO_ATTN_COMBINE = 2 };
enum GemvEpilogue : int {
  GEPI_STORE = 0,      // out[b][n] = y + bias
  GEPI_GELU = 1,       // out[b][n] = gelu(y + bias)
  GEPI_RESID = 2,      // out[b][n] += y + bias
  GEPI_QKV_CACHE = 3,  // n<d: q; then self-K (blocked) / self-V cache rows at `step`
  GEPI_LOGITS = 4,     // per-WG argmax partials (+ optional full logits dump)
  GEPI_PARTIAL = 5,    // batched path only: split-K partial sums [ksplit][part_batch][N], folded by the consumer
};

struct GemvParams {
  const h16* W; const float* bias; int N, K, batch;
  // prologue
  int prologue;
  const float* in;            // PRO_PLAIN: [B][K]; PRO_LAYERNORM: x [B][K]
  const float* ln_w; const float* ln_b;
  const float* part; int n_split; int n_head;   // PRO_ATTN_COMBINE: partials [B][H][n_split] of layout::kPartStride floats
  // epilogue
  int epilogue;
  float* out;                 // [B][N]
  h16* k_cache; h16* v_cache; long kv_batch_stride; int d_model; int n_ctx_pad;  // GEPI_QKV_CACHE (this layer)
  const DecState* state;
  const int* off;                  // per-clip offsets [batch] (GEPI_QKV_CACHE: cache row; GEPI_LOGITS: skip while every clip is below skip_before_step)
  float* amax_val; int* amax_idx; int amax_stride;  // GEPI_LOGITS: partials [clip][amax_stride], one per workgroup
  float* logits_dump;              // optional logits row of this step for clip b at logits_dump + b*logits_dump_stride
  long logits_dump_stride;
  int skip_before_step;            // GEPI_LOGITS: do nothing while state->step < this (SOT steps)
};
void launch_gemv(const GemvParams& p, hipStream_t s);
int gemv_grid(const GemvParams& p);  // number of workgroups launch_gemv will use

// x[b] = tok_emb[tok[b]] + pos[off[b]]
void launch_embed(const h16* tok_emb, const float* pos, const int* tok, const int* off, float* x, int batch, int d,
                  hipStream_t s);

// single-query attention over blocked K / row-major V, writes split partials [B][H][n_split][66]
struct DecAttnParams {
  const float* q;             // [B][d]
  const h16* k; const h16* v; long kv_batch_stride;   // this layer, slot 0
  float* part; int n_split;
  int batch, n_head, d_model;
  int n_keys;                 // fixed key count (cross) or -1: off[b] + 1 (self)
  int cap_blocks;             // allocated 64-key blocks per (slot, head): 24 cross, 7 self
  const DecState* state;
  const int* off;             // per-clip offsets [B]
  const int* done;            // device [B], never null: clips whose flag is set are skipped (greedy loop past their eot); all zero where nobody stops
  int done_late;              // few clips (a launch is one dependent chain): the flag is looked at BEHIND the first requests, not before them
  h16* out_hi; h16* out_lo; int nbs; // normalised output as a fragment-major h16 pair instead of partials; with n_split > 1
                                     // the splits of a (clip, head) meet through mpart / mcnt and the last one to arrive writes it
  float* mpart; unsigned* mcnt;      // [B][H][n_split][66] / [B][H] (zero between launches), same clip origin as q / out
  // fused query projection (batched cross-attention): q = Wq[head rows] . LayerNorm(x[b]) + bq computed by the
  // (clip, head) workgroup itself while its first K/V block is in flight; wq == nullptr: q is read from `q`
  const float* x; const float* ln_w; const float* ln_b; const h16* wq; const float* bq;
  // folded query (decode_gemm.hip "QUERY FOLD"; tq != nullptr): q[j] = rstd (tq[b][j] - mean fold_s[j]) + fold_c[j], mean / rstd of
  // the clip's residual row from its stat_part[b][d_model / 16][2] block statistics
  const float* tq; const float* stat_part; const float* fold_s; const float* fold_c;
  // measurement only (Engine::bench "attn_stamp"): [workgroups][2] = {begin, end} of every workgroup of this launch in
  // 100 MHz wall-clock ticks, written by the kernel itself (a separate template instantiation: the production kernel
  // carries no stamp code)
  unsigned long long* stamp;
};
void launch_decode_attention(const DecAttnParams& p, hipStream_t s);

// ---- FP8 cross K/V (cross_kv_fp8.hip; decode_layout.hpp "FP8 cross K/V"): opt-in storage of the batched step's cross-attention
// h16 cross K (blocked) and V (row-major) of `clips` clips -> e4m3fn code images and power-of-two scales, one workgroup per
// (layer, clip, head, K or V). Clip b's images are those of slot slot_map[b] (device; nullptr: slot b), as EPI_CROSS_KV wrote them.
struct CrossKvQuantParams {
  const h16* k; const h16* v;              // [layer][n_slots][head] images of keys_pad keys
  unsigned char* k8; unsigned char* v8;    // the code images, same order
  float* scales;                           // [layer][n_slots][head][2][64]
  const int* slot_map;
  int n_layer, n_slots, n_head, clips;
  int n_keys, keys_pad;                    // valid keys (<= keys_pad) and allocated keys (a multiple of 64) per (slot, head)
};
void launch_cross_kv_quantize(const CrossKvQuantParams& p, hipStream_t s);

// single-query cross-attention over the code images: decode_attention_kernel's three query modes, split record, ticket hand-off and
// fragment-major (hi, lo) output pair (the fields below mean what their namesakes in DecAttnParams mean)
struct DecAttnFp8Params {
  const float* q;
  const unsigned char* k8; const unsigned char* v8; long kv_batch_bytes;  // this layer, the launch's first slot
  const float* scales; long scale_batch_stride;                          // this layer, the launch's first slot: [head][2][64] per slot
  int n_split;
  int batch, n_head, d_model;
  int n_keys, cap_blocks;
  const int* done; int done_late;
  h16* out_hi; h16* out_lo; int nbs;
  float* mpart; unsigned* mcnt;
  const float* x; const float* ln_w; const float* ln_b; const h16* wq; const float* bq;
  const float* tq; const float* stat_part; const float* fold_s; const float* fold_c;
};
void launch_decode_cross_attention_fp8(const DecAttnFp8Params& p, hipStream_t s);

// ---- batched decode (3..64 clips per launch): activations as h16 (hi, lo) pairs, MFMA GEMM (decode_gemm.hip)
struct DecGemmParams {
  const h16* W;                           // fragment-major packed weights
  const float* bias; int N, K, batch;
  const h16* a_hi; const h16* a_lo;      // fragment-major h16 pair (decode_gemm.hip), this launch's first clip block
  int nbs;                                 // allocated clip blocks (stride of the activation layout)
  int epilogue;                            // GemvEpilogue
  int rt;                                  // weight-row tiles per wave: 1 (16 rows/WG) or 4 (64 rows/WG, vocabulary)
  float* out;                              // fp32 [batch][N] (STORE / RESID / q of QKV_CACHE)
  h16* out_hi; h16* out_lo;              // GEPI_GELU: h16 pair [batch][N]
  h16* k_cache; h16* v_cache; long kv_batch_stride; int d_model; int n_ctx_pad;
  const DecState* state;
  const int* off;                          // per-clip offsets [batch]
  float* amax_val; int* amax_idx; int amax_stride;
  float* logits_dump; long logits_dump_stride;
  int skip_before_step;
  int ksplit; int part_batch;              // GEPI_PARTIAL: K slices (grid.y) and the clip stride of the partial buffer
};
void launch_decode_gemm(const DecGemmParams& p, hipStream_t s);

// Clip-block form of the batched linear layer: one workgroup = 16 clips x 16*rt weight rows over the whole K, so the
// activations of a workgroup are 16 rows instead of 64, LayerNorm of the residual stream can be the prologue (no
// separate preparation launch, no activation round trip through memory) and the residual add can be the epilogue
// (every output element has exactly one owner: no split-K partials to fold).
struct DecCGemmParams {
  const h16* W;                           // fragment-major packed weights
  const float* bias; int N, K, batch;
  const float* x; const float* ln_w; const float* ln_b;   // ln_w != nullptr: input = LayerNorm(x [batch][K] fp32)
  const h16* a_hi; const h16* a_lo;      // else: fragment-major h16 pair
  int nbs;                                 // allocated clip blocks (stride of the pair layouts)
  int epilogue;                            // GEPI_STORE / GEPI_GELU / GEPI_RESID / GEPI_QKV_CACHE
  int rt;                                  // 1 or 2
  float* out;                              // fp32 [batch][N] (STORE, RESID: out += y; q of QKV_CACHE)
  h16* out_hi; h16* out_lo;              // GEPI_GELU: h16 pair
  h16* k_cache; h16* v_cache; long kv_batch_stride; int d_model; int n_ctx_pad;
  const DecState* state;
  const int* off;                          // per-clip offsets [batch]
  // query fold of the clip-block step (decode_gemm.hip "QUERY FOLD"); fold_row0 == 0: none
  int fold_row0;                           // rows >= fold_row0 are fold rows (QKV launch: 3 d_model; o launch: d_model)
  const float* ln_w2;                      // LayerNorm-prologue launch: the fold rows' input is ln_w2 . x (no statistics, no shift)
  const h16* W_lo;                         // pair-input launch: lo halves of the fold rows' weights (fragment-major, row block 0 = fold_row0)
  float* out2;                             // the fold rows' output / residual target [batch][N - fold_row0]
  float* stat_part;                        // GEPI_RESID: [batch][fold_row0 / 16][2] = (sum, squares about the block mean) of the new rows
  // measurement only (Engine::bench "attn_stamp"): [workgroups][2] = {begin, time at stamp_point} of every workgroup, 100 MHz ticks;
  // a separate template instantiation (the production kernel carries no stamp code)
  unsigned long long* stamp; int stamp_point;
};
void launch_decode_cgemm(const DecCGemmParams& p, hipStream_t s);
int decode_gemm_grid(int N, int rt);
bool decode_logits_resident_ok(int K, int batch);  // rt == 0 (one workgroup per CU, activations in registers) supports this shape
void launch_act_prep(float* x, const float* g, const float* be, h16* hi, h16* lo, int batch, int K, bool do_ln, int nbs,
                     const float* part, int n_part, int part_batch, const float* part_bias, hipStream_t s);
void launch_pack_weight_frag(const h16* w, h16* wp, int N, int K, hipStream_t s);
void launch_pack_weight_frag_split(const float* w, h16* hi, h16* lo, int N, int K, hipStream_t s);  // fp32 -> (hi, lo) h16 pair

struct AdvanceArgs {  // what advance_kernel itself takes
  const float* amax_val; const int* amax_idx; int n_part; int amax_stride;
  DecState* state; int* off; int* tok; int* done; int* n_out; int* out_ids; int batch;
  int* done_host;             // optional host-mapped [batch]: set (behind a system-scope fence) when a clip finishes, so that the
                              // host sees it without a copy or a synchronisation (Engine::stream_step)
  int n_ctx, eot, max_new, n_vocab;
  const int* max_new_clip;    // optional device [B]: per-clip id budget (a ragged batch), capped by max_new
  const int* sot;             // device [4]
  const int* forced; int n_forced;   // teacher forcing (device [B][n_forced]) or nullptr
  int* argmax_dump;           // optional [B][n_forced+1]
  const h16* tok_emb; const float* pos; float* x; int d_model;  // fused embedding of the next step
  int n_prefix;               // prefix tokens fed before the first sampled step (sot[0 .. n_prefix)); 0 means 4
  const int* base;            // optional device [B], forced mode: positions in front of the prefix (a prompted clip's L - 2); nullptr: none
};
// What callers fill in. sot_clip stands behind AdvanceArgs, not inside it: advance_kernel's argument block, and with it the code of
// every call that sets no sot_clip, stays what it was before the field existed.
struct AdvanceParams : AdvanceArgs {
  const int* sot_clip;        // optional device [B][4]: a prefix per clip (slot stream in timestamp mode); the token fed behind offset s
                              // is sot_clip[4 b + s + 1] instead of sot[s + 1]. Set: the second instantiation of the kernel runs
};
void launch_advance(const AdvanceParams& p, hipStream_t s);

// ---- timestamp rules (decode_timestamps.hip): one argmax partial per clip that samples at this step, chosen under
// Whisper's timestamp rules from the clip's dumped logits row and its history
struct TsRulesArgs {
  const float* logits; long stride;  // fp32 rows [batch][stride], stride a multiple of 4
  int batch, n_vocab, eot, ts_begin;  // ts_begin = no_timestamps + 1: id of 0.00 s
  const int* off;                    // device [batch] or nullptr (every clip samples); clips with off < n_prefix - 1 are skipped
  int n_prefix;
  const int* done;                   // device [batch] or nullptr: finished clips are skipped
  const int* out_ids; const int* n_out; int n_ctx;   // greedy history: [batch][n_ctx] ids, [batch] counts
  const int* forced; int n_forced;   // teacher-forced history [batch][n_forced] (n = off - n_prefix + 1 - base), or nullptr
  const int* base;                   // optional device [batch], forced mode: a prompted clip's L - 2; nullptr: none
  float* amax_val; int* amax_idx; int amax_stride;   // out: partial 0 of clip b at b * amax_stride
};
// What callers fill in. suppress stands behind TsRulesArgs, not inside it: the argument block of the rules kernels, and with it the
// code of every launch without a set, is what it was before there were sets; a launch with one runs the kernels' second instantiation.
struct TsRulesParams : TsRulesArgs {
  const unsigned* suppress;          // token suppression (suppress.hpp: the mask of the handle's set), or nullptr: no set
};
void launch_timestamp_rules(const TsRulesParams& p, hipStream_t s);
// Scored form (DESIGN.md "Confidence"): the rules kernel that also writes, for every clip that samples at this step, the
// log-probability of the chosen id under the final allowed set and the decision id, both at index n = the clip's history length.
// With `off` and `no_speech` set, clips at decode offset 0 get log p(no_speech_id) over their whole row instead.
struct TsScoreParams {
  float* logprob; int* decision; long stride;   // out: [batch][stride], entry n of clip b (n < stride)
  float* no_speech; int no_speech_id;           // out: [batch], or nullptr
};
void launch_timestamp_rules_scored(const TsRulesParams& p, const TsScoreParams& q, hipStream_t s);
// Sampled form (DESIGN.md "Temperature fallback"): the scored kernel whose decision, for a clip with temperature[b] > 0, is drawn
// from softmax(x[A] / t) over the final allowed set by Gumbel-max: argmax over A of x[i] / t - log(-log(u_i)) (lowest id on ties),
// u_i = ((w >> 9) + 0.5) * 2^-23 with w = word i & 3 of Philox4x32-10(counter (i >> 2, n, stream[b] low, stream[b] high), key
// seed low, seed high), n = the clip's history length. The recorded log-probability stays the untempered x[c] - logsumexp(x[A]).
// temperature[b] <= 0: the scored kernel's decision. All three are device memory, so one captured step serves every call.
struct TsSampleParams {
  const float* temperature;          // [batch]
  const unsigned long long* stream;  // [batch]
  const unsigned long long* seed;    // [1]
};
void launch_timestamp_rules_sampled(const TsRulesParams& p, const TsScoreParams& q, const TsSampleParams& r, hipStream_t s);
// out[b] = logits[b][id] - logsumexp(logits[b][0 .. n_vocab)), NaN entries left out; rows [batch][stride], stride a multiple of 4
void launch_row_logprob(const float* logits, long stride, int n_vocab, int id, int batch, float* out, hipStream_t s);

// ---- beam search (decode_beam.hip; DESIGN.md "Beam search"): a clip owns K = beam slots [clip * K, clip * K + K); a hypothesis
// ("rank") of the clip lives in one of them. Three launches per step on one stream, in this order.
constexpr int kBeamMax = 8;                  // K
constexpr int kBeamMaxCand = kBeamMax + 1;   // M = K + 1 candidates per hypothesis
// One workgroup per slot: the M best ids of the final allowed set A (scored mode's: rules 1-5, NaN and -inf out) of the slot's
// row under its history, value descending, lower id first on equal values, each with x[c] - logsumexp(x[A]).
struct BeamCandParams {
  const float* logits; long stride;  // fp32 rows [n_slots][stride], stride a multiple of 4
  int n_slots, n_vocab, eot, ts_begin;
  const int* hist; int hist_stride;  // histories [n_slots][hist_stride] (prefix excluded)
  const int* n_hist; int n;          // history lengths: device [n_slots], or nullptr: n for every slot
  const float* slot_score;           // device [n_slots] or nullptr: a slot whose value is -inf is dead and proposes nothing
  const int* complete; int beam;     // device [n_slots / beam] or nullptr: the slots of a complete clip propose nothing
  int n_cand_max;                    // M <= kBeamMaxCand
  int* cand_id; float* cand_logprob; // out [n_slots][M]; entries from n_cand on: eot, -inf
  int* n_cand;                       // out [n_slots]: min(M, |A|)
  const unsigned* suppress;          // token suppression (suppress.hpp: the mask of the handle's set), or nullptr: no set
};
void launch_beam_candidates(const BeamCandParams& p, hipStream_t s);
// One wave per clip: score = S[parent] + logprob in float32; order by score descending, parent rank, position; walk as
// openai-whisper's BeamSearchDecoder.update. All state is read first and then overwritten in place.
struct BeamSelectParams {
  int n_clips, beam, eot, n;               // n: history length before this step (the chosen ids go to hist[.][n])
  const int* cand_id; const float* cand_logprob; const int* n_cand;  // by slot, M = beam + 1 per slot
  float* S; int* slot;                     // in/out [n_clips * beam] by rank: sum_logprob (-inf: dead), the rank's slot
  float* slot_score;                       // out [n_clips * beam] by slot: S of the rank that lives there
  int* hist; int hist_stride;              // in [.][0, n) / out [.][n], by slot
  int* src;                                // out [n_clips * beam] by slot: the slot its history and cache come from (itself: stays)
  int* pool_n;                             // in/out [n_clips]
  int* pool_ids; int* pool_len; float* pool_score;  // in/out [n_clips * beam][hist_stride] / [n_clips * beam]: records in the order they finished
  int* complete;                           // in/out [n_clips]
  int* n_complete;                         // device counter, bumped once per clip that completes
};
void launch_beam_select(const BeamSelectParams& p, hipStream_t s);
// For every slot with src[slot] != slot: hist[0, n) and, for every (layer, head), the 64-key blocks covering keys [0, off] of K and V
struct BeamReorderParams {
  const int* src; int n_slots;
  int* hist; int hist_stride; int n;
  h16* k; h16* v;                          // self-attention caches, layer 0, slot 0
  long kv_batch_stride; int cap;           // elements of one slot of one layer; allocated slots (layer stride = cap * kv_batch_stride)
  int n_layer, n_head, n_ctx_pad, off;
};
void launch_beam_reorder(const BeamReorderParams& p, hipStream_t s);
// cross K/V of slot src -> slots dst0 .. dst0 + n_dst - 1 in every layer (src itself is skipped); slot_elems a multiple of 8.
// Spreading clips 0 .. C-1 to groups of K: launch for the clips in DESCENDING order (clip i's destinations start at i * K >= i,
// so sources not yet spread are never overwritten).
void launch_beam_spread_cross(h16* k, h16* v, long layer_stride, long slot_elems, int n_layer, int src, int dst0, int n_dst, hipStream_t s);

// ---- prompt prefill (decode_prefill.hip; DESIGN.md "Prompt conditioning"): the context rows [sot_prev, prompt, sot, language] of
// every prompted clip in one pass. Rows of a clip are contiguous; per-row and per-clip tables live in device memory.
// x[row] = tok_emb[ctx[row]] + pos[row_pos[row]], fp32 [rows][d]
void launch_prefill_embed(const h16* tok_emb, const float* pos, const int* ctx, const int* row_pos, float* x, int rows, int d,
                          hipStream_t s);
// K and V columns of qkv (h16 [rows][3 d_model], the QKV GEMM's output) -> cache row row_pos[row] of slot row_slot[row]
struct PrefillStoreParams {
  const h16* qkv; int rows;
  const int* row_pos; const int* row_slot;   // device [rows]
  h16* k_cache; h16* v_cache;                // this layer, slot 0
  long kv_slot_stride; int d_model; int n_ctx_pad;
};
void launch_prefill_cache_store(const PrefillStoreParams& p, hipStream_t s);
// out[row0[c] + i] = softmax(q[row0[c] + i] . K^T / 8) V for i < len[c], per head, over the caches of slot[c]:
// n_keys < 0: causal over the self cache (query i sees keys 0 .. i); else keys 0 .. n_keys - 1 of the cross cache
struct PrefillAttnParams {
  const h16* q; int ldq;                     // h16 rows, head h at columns [64 h, 64 h + 64)
  const h16* k; const h16* v;                // this layer, slot 0: blocked K, row-major V
  long kv_slot_stride; int keys_pad;         // elements per slot; allocated keys per head (a multiple of 64)
  h16* out; int ldo;
  const int* row0; const int* len; const int* slot;  // device [n_clips]
  int n_clips, max_len, n_head, n_keys;
};
void launch_prefill_attention(const PrefillAttnParams& p, hipStream_t s);
// out[c] = x[rows[c]], fp32 rows of d
void launch_prefill_gather_rows(const float* x, const int* rows, float* out, int n, int d, hipStream_t s);
// per prompted clip c, slot b = slot[c]: off[b] = len[c], tok[b] = transcribe, n_out[b] = 0, x[b] = tok_emb[transcribe] + pos[len[c]],
// no_speech[b] = no_speech_clip[c] (both or neither null)
struct PrefillHandoverParams {
  const int* slot; const int* len; int n_clips;
  int* off; int* tok; int* n_out; int transcribe;
  const h16* tok_emb; const float* pos; float* x; int d_model;
  float* no_speech; const float* no_speech_clip;
  const int* task_tok;  // optional device [n_clips]: the id fed at len[c] instead of `transcribe` (a clip's task); nullptr: transcribe
};
void launch_prefill_handover(const PrefillHandoverParams& p, hipStream_t s);

// ---- language detection (decode_language.hip; DESIGN.md "Language and task per clip"): per clip c, the final LayerNorm of the
// fp32 residual row x[x_row ? x_row[c] : c] and its dot products with the n_lang language rows of the tied embedding ->
// lang_logit (optional), lang_logprob = lang_logit - logsumexp (NaN entries left out, -inf), lang_index = the first maximum in
// list order (nothing finite: fallback_index, every lang_logprob -inf); with ctx: ctx[lang_row[c]] = lang_tokens[lang_index[c]]
constexpr int kLangMax = 128;     // languages
constexpr int kLangMaxD = 2048;   // d_model
struct LangDetectParams {
  const float* x; const int* x_row;          // fp32 rows of d_model; device [n_clips] row numbers or nullptr
  const float* ln_w; const float* ln_b; const h16* tok_emb;
  const int* lang_tokens; int n_lang;        // device [n_lang], ids inside the vocabulary
  int d_model, n_clips, fallback_index;
  float* lang_logit; float* lang_logprob;    // out [n_clips][n_lang]
  int* lang_index;                           // out [n_clips]
  int* ctx; const int* lang_row;             // optional: the prefill pass's context table and, per clip, the entry to patch
};
void launch_language_detect(const LangDetectParams& p, hipStream_t s);

// ---- slot stream in timestamp mode (decode_timestamps.hip: stream_rules_kernel; DESIGN.md "Slot stream in timestamp mode"): the
// scored rules kernel for slots that are refilled. Slot b with done[b] set: nothing at all. Else at offset 0: no_speech[b], and with
// detect[b] the language pick of the row that is already there (lang_logit[j] = row[lang_tokens[j]], the definition of
// LangDetectParams) -> slot_ctx[4 b + 1] = lang_tokens[pick], lang_out[b], lang_logprob[b][0 .. n_lang). Offset 1: nothing. From
// offset n_prefix - 1 on: the scored decision. TsRulesParams::off and ::done and TsScoreParams::no_speech are required.
struct StreamRulesParams {
  const int* detect;                         // device [batch]
  int* slot_ctx;                             // device [batch][4]: [sot, language id, task id, unused], the table advance_kernel feeds from
  const int* lang_tokens; int n_lang;        // device [n_lang] (n_lang <= kLangMax), ids inside the vocabulary
  int fallback_index;                        // nothing finite: this index
  int* lang_out; float* lang_logprob;        // out [batch], [batch][n_lang]
};
void launch_stream_rules(const TsRulesParams& p, const TsScoreParams& q, const StreamRulesParams& t, hipStream_t s);

// ---- word-level timestamps (decode_align.hip; DESIGN.md "Word-level timestamps"). The rows of a clip are contiguous in q (clip c at
// row0[c], len[c] rows); clip c attends to its own n_keys[c] frames. All per-clip tables are device memory.
// P[c][a][i][f] = softmax over f < n_keys[c] of q[row0[c] + i][head a] . K[slot[c]][head a][f] / 8 for i < len[c], fp32; columns
// [n_keys[c], the end of the last 64-key block) are written as zeros, nothing else is touched
struct AlignQKParams {
  const h16* q; int ldq;                     // h16 rows, head h at columns [64 h, 64 h + 64)
  const h16* k; long kv_slot_stride; int keys_pad;  // this layer's blocked cross K, slot 0; allocated keys per head (a multiple of 64)
  const int* row0; const int* len; const int* slot; const int* n_keys;  // device [n_clips]
  const int* heads; int n_align;             // device [n_align]: the layer's alignment heads
  float* P; int rows_pad, f_pad;             // out [n_clips][n_align][rows_pad][f_pad], f_pad a multiple of 64
  int n_clips, max_len;
};
void launch_align_qk_softmax(const AlignQKParams& p, hipStream_t s);
// matrix[c][i][f] += inv_heads * median7 over f (reflect padding; skipped at n_keys[c] <= 3) of (P[c][a][i][f] - mean_i) / std_i, summed
// over the layer's heads a, for i < len[c], f < n_keys[c]; mean and population std over the clip's len[c] rows
struct AlignNormParams {
  const float* P; int rows_pad, f_pad, n_align;
  const int* len; const int* n_keys;         // device [n_clips]
  float* matrix; int m_rows, m_ld;           // [n_clips][m_rows][m_ld]
  float inv_heads;
  int n_clips, max_keys;
};
void launch_align_normalize(const AlignNormParams& p, hipStream_t s);
// jump[c][i] = the frame of the first point in row i of the DTW path over -matrix[c][3 + i][f], i < N = len[c] - 4, f < n_keys[c]
// (align_path.hpp); a clip with N < 1 or no frame is skipped
constexpr int kAlignDtwThreads = 512;        // a thread per row of the cost table: N + 1 <= 512
struct AlignDtwParams {
  const float* matrix; int m_rows, m_ld;     // m_ld a multiple of 4
  const int* len; const int* n_keys;         // device [n_clips]
  uint8_t* trace; long trace_clip_stride;    // scratch [n_clips][>= (N + 1) (F + 1)]
  int* jump; int jump_ld;                    // out [n_clips][jump_ld]
  int n_clips, max_len;
};
void launch_align_dtw(const AlignDtwParams& p, hipStream_t s);
// out[r] = logits[r][id[r]] - logsumexp(logits[r][0 .. n_ids)); rows [rows][stride]; an id outside [0, n_ids): -inf
void launch_row_id_logprob(const float* logits, long stride, int n_ids, const int* id, int rows, float* out, hipStream_t s);

// ---- fused vocabulary log-probabilities (vocab_logprob.hip): out[r] = logit[r][id[r]] - logsumexp(logit[r][0 .. eot)) with
// logit = a . W^T, a the LayerNorm'ed rows in the 16-bit type; the logits are never written. An id outside [0, eot): -inf.
constexpr size_t kVocabLogProbMaxLds = 66560;  // the row tile in LDS: 64 rows of 512 + 8, 32 of 1024 + 8, 16 of 2048 + 8 elements
struct VocabLogProbParams {
  const h16* a;                  // [rows rounded up to row_tile][d]: the rows beyond `rows` are zeros
  const h16* W; int n_vocab;     // the tied embedding [n_vocab][d]
  const int* id;                 // device [rows]
  int rows, d, eot;
  int row_tile, n_splits, split_cols;  // vocab_logprob_plan's
  float* part_m; float* part_s;  // scratch [n_splits][rows]
  float* target;                 // scratch [rows]
  float* out;                    // [rows]
};
void launch_vocab_logprob(const VocabLogProbParams& p, hipStream_t s);  // the main and the merge launch

// ---- persistent decode (decode_persistent.hip, decode_persistent2.hip): the whole greedy loop of one to three clips in ONE launch
typedef unsigned long long u64;
struct PersistParams {
  const h16* wl; const float* fl;   // decoder-layer weight arenas (DecArena layout)
  const float* qf;                  // d_model <= 768: the query-fold arena (decode_persistent.hip), nullptr = unfolded
  const h16* tok_emb; const float* pos; const float* ln_w; const float* ln_b;
  const h16* cross_k; const h16* cross_v; long cross_layer_stride;  // this clip's slot, layer 0
  int n_layer, n_vocab, n_ctx, n_audio_ctx;
  int eot, max_new, total_steps;
  const int* sot;               // device [4]
  const int* forced; int n_forced; float* logits_dump; int* argmax_dump;   // teacher forcing (tests)
  u64* gran; unsigned* err;     // granule area + error word, zeroed before every launch
  int gran_bytes;               // size of the granule area (buffer-resource bound of the 16-byte polls)
  int* out_ids; int* n_out; DecState* state;
  int fault;                    // test hook (AX_WHISPER_PERSIST_FAULT=1): workgroup 0 leaves at once, so the launch must give up
  long long* prof;              // optional [grid][64]: per-phase 100 MHz tick sums + one layer's absolute timeline (AX_WHISPER_PERSIST_PROF), else nullptr
  // Two or three clips in one launch (n_clip 2 or 3; greedy decode only): every phase runs for clip 0, then clip 1 (and 2) with
  // the same weight rows in registers, so that one clip's hand-off is in flight while the next clip's rows are computed. Clip 0
  // keeps the LDS-resident K/V of the one-clip launch; the later clips read their K/V from global memory: clip 1's cross K/V in
  // the next slot (cross_clip_stride elements on), its self-attention cache in self_k1 / self_v1 ([n_layer * n_head][8 blocks]
  // [4096], the per-owner layouts of the LDS cache). Granules, ids and counts of clip 1: gran + gran_clip_u64, out_ids1, n_out1.
  int n_clip;
  int prof_clip;  // multi-clip timeline: whose absolute stamps are kept (decode_persistent2.hip)
  long cross_clip_stride;
  h16* self_k1; h16* self_v1;
  long gran_clip_u64;
  int* out_ids1; int* n_out1; int max_new1;
  // three clips (n_clip == 3): clip 2's ids at out_ids1 + n_ctx, its count at n_out1 + 1, its self cache self_clip_stride elements on
  int max_new2; long self_clip_stride;
  // One-clip launch: the poller waves keep the tail of their workgroup's vocabulary rows in registers for the whole launch
  // (decode_persistent.hip "resident vocabulary rows"); 0 (AX_WHISPER_VOCAB_RESIDENT=0): every row is streamed every step
  int vocab_resident;
  // One-clip launch under the timestamp rules (decode_persistent_rules.hpp; rules = 1: the kernel's rules instantiation). n_prefix: ids
  // of the prefix (4 plain: [sot, language, transcribe, notimestamps]; 3 under the rules); ts_begin: id of 0.00 s; suppress: the
  // suppress mask's words (decode_rules.hpp) or nullptr. Scored mode: ts_logprob / ts_decision ([ts_stride], index = history length)
  // and no_speech (one value) as the scored rules kernel writes them, nullptr: timestamp mode. logits0_dump: teacher forcing, the row
  // of the step that fed sot (scored mode only).
  int rules, n_prefix, ts_begin;
  const unsigned* suppress;
  float* ts_logprob; int* ts_decision; long ts_stride; float* no_speech; int no_speech_id;
  float* logits0_dump;
};
bool decode_persistent_supported(int d_model, int n_head, int n_layer, int n_cu);
int decode_persistent_grid(int d_model, int n_cu);
size_t decode_persistent_gran_bytes(int d_model, int grid);   // granule area; the error word sits in its last 8 bytes
size_t qfold_floats(int d_model, int n_layer);                // floats of the query-fold arena
void launch_qfold_build(const h16* wl, const float* fl, float* qf, int d_model, int n_layer, hipStream_t s);
hipError_t launch_decode_persistent(const PersistParams& p, int d_model, int grid, hipStream_t s);  // n_clip 1, 2 or 3
int decode_persistent_max_clips(int d_model, int n_head, int n_layer, int grid);  // clips per persistent launch: 1, 2 or 3
bool decode_persistent_rules_supported(int n_vocab, int grid);  // the rules instantiation: every workgroup's rows fit its suppress image
int decode_persistent_vocab_resident_rows(int d_model, int n_vocab, int grid);    // vocabulary rows a workgroup of the one-clip launch keeps on-chip
// host only: the decisions above for a shape + the cross-attention role assignment of a launch (AX_WHISPER_PersistentDecodePlan)
int decode_persistent_plan(int d_model, int n_head, int n_layer, int n_cu, int n_clips, int t0, int n_slots, int* plan4, int* units);

// weight preparation (device): raw file dtype -> h16 / fp32, with the layout changes the kernels want
void launch_convert_to_h16(const void* src, int src_dtype /*0 f32,1 bf16,2 f16*/, h16* dst, long n, hipStream_t s);
void launch_convert_to_f32(const void* src, int src_dtype, float* dst, long n, hipStream_t s);
// conv weight [Cout][Cin][3] -> [Cout][Kpad] with k-major taps: dst[n][k*Cin + c]
void launch_conv_weight_pack(const void* src, int src_dtype, h16* dst, int cout, int cin, int kpad, hipStream_t s);

}  // inline namespace AXW_NS
}  // namespace axw
