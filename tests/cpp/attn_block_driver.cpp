// attn_block_driver.cpp — the persistent launches' 64-key attention block (csrc/decode_persistent_common.hpp) on its own, for
// tests/test_gpu_attn_block.py: one workgroup of nw waves stages eight K and V blocks, the query and a pre-filled scratch area
// into LDS, wave w runs block w with its first nvalid[w] keys valid, and the eight partial records (m, l, o[64]) come back.
// Forms: 0 = row-major V (cross tile), 1 = transposed V (self cache), 2 = the register-held block (K/V pieces from global memory).
// Built per dtype (-DAXW_F16) and per form of the block (-DAXW_ATTN_MFMA).
//   attn_block_driver <cases.bin> <out.bin>
//   cases.bin: int32 n, then per case { int32 form, nw, nvalid[8]; uint32 fill; uint32 q[64]; uint16 K[8][4096], V[8][4096] }
//   out.bin:   per case float32 [8][66]; records of waves >= nw keep the sentinel they were filled with
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "decode_persistent_common.hpp"

using namespace axw;

constexpr int kBlocks = NCW, kBlkElems = layout::kKvBlockElems;
constexpr unsigned kSentinel = 0x7FC57FC5u;
constexpr size_t kLds = (size_t)2 * kBlocks * kBlkElems * 2 + 64 * 4 + kBlocks * 64 * 4 + kBlocks * kPS * 4;

template <int FORM>
__global__ void __launch_bounds__(NCW * 64) attn_block_case(const h16* K, const h16* V, const unsigned* q, const int* nvalid, unsigned fill, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  h16* sK = reinterpret_cast<h16*>(smem);
  h16* sV = sK + kBlocks * kBlkElems;
  unsigned* qs = reinterpret_cast<unsigned*>(sV + kBlocks * kBlkElems);
  float* pscr = reinterpret_cast<float*>(qs + 64);
  float* wpart = pscr + kBlocks * 64;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < kBlocks * kBlkElems / 8; i += nt) {
    reinterpret_cast<u32x4*>(sK)[i] = reinterpret_cast<const u32x4*>(K)[i];
    reinterpret_cast<u32x4*>(sV)[i] = reinterpret_cast<const u32x4*>(V)[i];
  }
  for (int i = tid; i < 64; i += nt) qs[i] = q[i];
  for (int i = tid; i < kBlocks * 64; i += nt) pscr[i] = __uint_as_float(fill);
  for (int i = tid; i < kBlocks * kPS; i += nt) wpart[i] = __uint_as_float(kSentinel);
  __syncthreads();
  const int lane = tid & 63, cw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool valid = lane < nvalid[cw];
  if constexpr (FORM == 0) attn_block<false>(sK + cw * kBlkElems, sV + cw * kBlkElems, qs, valid, pscr + cw * 64, wpart + cw * kPS, lane);
  if constexpr (FORM == 1) attn_block<true>(sK + cw * kBlkElems, sV + cw * kBlkElems, qs, valid, pscr + cw * 64, wpart + cw * kPS, lane);
  if constexpr (FORM == 2) {
    u32x4 kr[8], vr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kr[i] = kv_global16(K + cw * kBlkElems, attn_regs_piece(i, lane));
#pragma unroll
    for (int i = 0; i < 8; ++i) vr[i] = kv_global16(V + cw * kBlkElems, attn_regs_piece(i, lane));
    attn_block_regs(kr, vr, qs, valid, pscr + cw * 64, wpart + cw * kPS, lane);
  }
  __syncthreads();
  for (int i = tid; i < kBlocks * kPS; i += nt) out[i] = wpart[i];
}

#define CHECK(X)                                                                                  \
  do {                                                                                            \
    const hipError_t e_ = (X);                                                                    \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #X, hipGetErrorString(e_)); return 2; } \
  } while (0)

struct CaseHead { int form, nw, nvalid[8]; unsigned fill; unsigned q[64]; };

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
  void (*kern[3])(const h16*, const h16*, const unsigned*, const int*, unsigned, float*) = {attn_block_case<0>, attn_block_case<1>, attn_block_case<2>};
  for (auto k : kern) CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
  for (int c = 0; c < n; ++c) {
    CaseHead h;
    if (fread(&h, sizeof h, 1, f) != 1 || fread(hk.data(), 2, hk.size(), f) != hk.size() || fread(hv.data(), 2, hv.size(), f) != hv.size()) {
      fprintf(stderr, "case %d: short read\n", c);
      return 1;
    }
    if (h.form < 0 || h.form > 2 || h.nw < 1 || h.nw > NCW) { fprintf(stderr, "case %d: bad form / waves\n", c); return 1; }
    CHECK(hipMemcpy(dK, hk.data(), kv_bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dV, hv.data(), kv_bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dq, h.q, 64 * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dn, h.nvalid, 8 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kern[h.form], dim3(1), dim3(h.nw * 64), kLds, 0, dK, dV, dq, dn, h.fill, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(res.data() + (size_t)c * kBlocks * kPS, dout, kBlocks * kPS * 4, hipMemcpyDeviceToHost));
  }
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(res.data(), 4, res.size(), o) != res.size()) { perror(argv[2]); return 1; }
  fclose(o);
  printf("%s mfma=%d cases %d done\n", kDtypeName, (int)kAttnMfma, n);
  return 0;
}
