// cross_tile_driver.cpp — the persistent launches' staging of cross K/V tiles (stage_cross_kv, csrc/decode_persistent_common.hpp)
// together with the 64-key block that reads them, for tests/test_gpu_cross_v_swizzle.py: one workgroup of eight waves, wave w owns
// block w of eight K and V blocks that lie in GLOBAL memory as the cross caches hold them (blocked K, row-major V).
// Modes: 0 = the blocks copied into LDS as they are, attn_block<false> (the plain row-major V home);
//        1 = LDS-DMA through stage_cross_kv in the kernels' own piece splits (0,2) (2,8) (8,11) (11,13) (13,16), then the block
//            on the image that helper leaves (attn_block<false, kCrossVSwizzle>, what cross_unit_block runs);
//        2 = the same with the whole block staged by one call (the first layer's prologue).
// Built per dtype (-DAXW_F16) and per form of the block (-DAXW_ATTN_MFMA); the case file is attn_block_driver's.
//   cross_tile_driver <cases.bin> <out.bin>
//   cases.bin: int32 n, then per case { int32 mode, nw (8), nvalid[8]; uint32 fill; uint32 q[64]; uint16 K[8][4096], V[8][4096] }
//   out.bin:   per case float32 [8][66]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "decode_persistent_common.hpp"

using namespace axw;

constexpr int kBlocks = NCW, kBlkElems = layout::kKvBlockElems;
constexpr unsigned kSentinel = 0x7FC57FC5u;
constexpr size_t kLds = (size_t)2 * kBlocks * kBlkElems * 2 + 64 * 4 + kBlocks * 64 * 4 + kBlocks * kPS * 4;

template <int MODE>
__global__ void __launch_bounds__(NCW * 64) cross_tile_case(const h16* K, const h16* V, const unsigned* q, const int* nvalid, unsigned fill, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  h16* sK = reinterpret_cast<h16*>(smem);
  h16* sV = sK + kBlocks * kBlkElems;
  unsigned* qs = reinterpret_cast<unsigned*>(sV + kBlocks * kBlkElems);
  float* pscr = reinterpret_cast<float*>(qs + 64);
  float* wpart = pscr + kBlocks * 64;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, cw = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the tile region starts out as NaN patterns: a piece the staging missed shows in the record
  for (int i = tid; i < 2 * kBlocks * kBlkElems / 8; i += nt) reinterpret_cast<u32x4*>(smem)[i] = u32x4{kSentinel, kSentinel, kSentinel, kSentinel};
  for (int i = tid; i < 64; i += nt) qs[i] = q[i];
  for (int i = tid; i < kBlocks * 64; i += nt) pscr[i] = __uint_as_float(fill);
  for (int i = tid; i < kBlocks * kPS; i += nt) wpart[i] = __uint_as_float(kSentinel);
  __syncthreads();
  if constexpr (MODE == 0) {
    for (int i = tid; i < kBlocks * kBlkElems / 8; i += nt) {
      reinterpret_cast<u32x4*>(sK)[i] = reinterpret_cast<const u32x4*>(K)[i];
      reinterpret_cast<u32x4*>(sV)[i] = reinterpret_cast<const u32x4*>(V)[i];
    }
  } else {
    const h16 *gk = K + cw * kBlkElems, *gv = V + cw * kBlkElems;
    h16 *sKw = sK + layout::kv_chunk_offset(cw, 0, 0), *sVw = sV + layout::kv_chunk_offset(cw, 0, 0);
    if constexpr (MODE == 1) {
      stage_cross_kv(gk, gv, sKw, sVw, 0, 2, lane);
      stage_cross_kv(gk, gv, sKw, sVw, 2, 8, lane);
      stage_cross_kv(gk, gv, sKw, sVw, 8, 11, lane);
      stage_cross_kv(gk, gv, sKw, sVw, 11, 13, lane);
      stage_cross_kv(gk, gv, sKw, sVw, 13, 16, lane);
    } else {
      stage_cross_kv(gk, gv, sKw, sVw, 0, 16, lane);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the LDS-DMA has landed
  }
  __syncthreads();
  const bool valid = lane < nvalid[cw];
  if constexpr (MODE == 0) attn_block<false>(sK + cw * kBlkElems, sV + cw * kBlkElems, qs, valid, pscr + cw * 64, wpart + cw * kPS, lane);
  else attn_block<false, kCrossVSwizzle>(sK + cw * kBlkElems, sV + cw * kBlkElems, qs, valid, pscr + cw * 64, wpart + cw * kPS, lane);
  __syncthreads();
  for (int i = tid; i < kBlocks * kPS; i += nt) out[i] = wpart[i];
}

#define CHECK(X)                                                                                  \
  do {                                                                                            \
    const hipError_t e_ = (X);                                                                    \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #X, hipGetErrorString(e_)); return 2; } \
  } while (0)

struct CaseHead { int mode, nw, nvalid[8]; unsigned fill; unsigned q[64]; };

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  int n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 1 || n > 4096) { fprintf(stderr, "bad case count\n"); return 1; }
  const size_t kv_bytes = (size_t)kBlocks * kBlkElems * 2;
  std::vector<unsigned short> hk(kBlocks * kBlkElems), hv(kBlocks * kBlkElems);
  std::vector<float> res((size_t)n * kBlocks * kPS);
  h16 *dK, *dV;
  unsigned* dq;
  int* dn;
  float* dout;
  CHECK(hipMalloc(&dK, kv_bytes));
  CHECK(hipMalloc(&dV, kv_bytes));
  CHECK(hipMalloc(&dq, 64 * 4));
  CHECK(hipMalloc(&dn, 8 * 4));
  CHECK(hipMalloc(&dout, kBlocks * kPS * 4));
  void (*kern[3])(const h16*, const h16*, const unsigned*, const int*, unsigned, float*) = {cross_tile_case<0>, cross_tile_case<1>, cross_tile_case<2>};
  for (auto k : kern) CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
  for (int c = 0; c < n; ++c) {
    CaseHead h;
    if (fread(&h, sizeof h, 1, f) != 1 || fread(hk.data(), 2, hk.size(), f) != hk.size() || fread(hv.data(), 2, hv.size(), f) != hv.size()) {
      fprintf(stderr, "case %d: short read\n", c);
      return 1;
    }
    if (h.mode < 0 || h.mode > 2 || h.nw != NCW) { fprintf(stderr, "case %d: bad mode / waves\n", c); return 1; }
    CHECK(hipMemcpy(dK, hk.data(), kv_bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dV, hv.data(), kv_bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dq, h.q, 64 * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dn, h.nvalid, 8 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kern[h.mode], dim3(1), dim3(NCW * 64), kLds, 0, dK, dV, dq, dn, h.fill, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(res.data() + (size_t)c * kBlocks * kPS, dout, kBlocks * kPS * 4, hipMemcpyDeviceToHost));
  }
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(res.data(), 4, res.size(), o) != res.size()) { perror(argv[2]); return 1; }
  fclose(o);
  printf("%s mfma=%d swizzle=%d cases %d done\n", kDtypeName, (int)kAttnMfma, (int)kCrossVSwizzle, n);
  return 0;
}
