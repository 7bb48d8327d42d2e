// decode_attention_group_common.hpp — what the two grouped cross-attention kernels share around their own K/V streams:
// decode_cross_attention_group_kernel (decode_attention_group.hip, h16 images) and decode_cross_attention_group_fp8_kernel
// (decode_attention_group_fp8.hip, FP8 code images). The 16-row A images of v_mfma_f32_16x16x32 (rank g's hi half on row 2 g, its lo
// half on row 2 g + 1), the reductions over a 16-lane row, and the transposed reads of the swizzled V tile.
#pragma once
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {
namespace {

constexpr int kGroupMax = 8;     // ranks a workgroup serves
constexpr int kARowStride = 72;  // h16 per row of the query and probability images: 144 bytes, rows 4 q land 16 banks apart
constexpr int kAImage = 16 * kARowStride;
constexpr int kActStride = 1024; // floats per LayerNormed row (d_model <= 1024)

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

__device__ __forceinline__ float row16_max(float v) {
#define AXW_DPP_F(CTRL, X) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(X), CTRL, 0xf, 0xf, true))
  v = fmaxf(v, AXW_DPP_F(0xB1, v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, AXW_DPP_F(0x4E, v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, AXW_DPP_F(0x141, v));  // row_half_mirror
  v = fmaxf(v, AXW_DPP_F(0x140, v));  // row_mirror
  return v;
}
__device__ __forceinline__ float quad_sum(float v) {
  v += AXW_DPP_F(0xB1, v);
  v += AXW_DPP_F(0x4E, v);
#undef AXW_DPP_F
  return v;
}
// rank g's value of column `col` into an A image: hi on row 2 g, lo on row 2 g + 1
__device__ __forceinline__ void put_pair(h16* img, int g, int col, float x) {
  const h16 hi = (h16)x;
  img[(2 * g) * kARowStride + col] = hi;
  img[(2 * g + 1) * kARowStride + col] = (h16)(x - (float)hi);
}
// the lane's A fragment of k-step ks: row lane % 16, k = 32 ks + 8 (lane / 16) .. + 7
__device__ __forceinline__ h16x8 a_frag(const h16* img, int ks, int lane) {
  return *reinterpret_cast<const h16x8*>(img + (lane & 15) * kARowStride + 32 * ks + 8 * (lane >> 4));
}
// B piece (dim block nb, k-step ks) of the swizzled row-major V tile: two transposed reads, every lane of the wave active
__device__ __forceinline__ h16x8 v_frag(const h16* tile, int base, int nb, int ks) {
  struct { s16x4 lo, hi; } r;
  r.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tile + layout::cross_v_read_offset(base, nb, ks, 0, true)));
  r.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tile + layout::cross_v_read_offset(base, nb, ks, 1, true)));
  return __builtin_bit_cast(h16x8, r);
}

}  // namespace
}  // inline namespace AXW_NS
}  // namespace axw
