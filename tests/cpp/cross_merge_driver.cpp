// cross_merge_driver.cpp — the row producers' merge of the cross-attention records in both forms (csrc/decode_persistent_common.hpp),
// for tests/test_gpu_cross_merge.py: ONE workgroup of 1024 threads (eight poller waves, eight compute waves, as in the launch)
// reads H * kCrossSplit complete records that the host wrote as {tag, value} granules before the launch, and merges them
//   form 0: inside the gather (co_gather_merge, called by the compute waves as in the kernel; one barrier), and
//   form 1: through LDS (the gather of pairs into pbuf, a barrier, merge_cross_records, a barrier),
// each as decode_persistent.hip spells it. Nothing waits on a missing tag: a lane that polled a granule without the tag would give
// up after the launch's 50 ms, and the driver reports it.
//   cross_merge_driver <cases.bin> <out.bin>
//   cases.bin: int32 n, then per case { int32 H; float rec[H * kCrossSplit][66] (o[64], m, l) }
//   out.bin:   per case float32 form 0 [H * 64], form 1 [H * 64]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "decode_persistent_common.hpp"

using namespace axw;

constexpr unsigned kTag = 0x1234u;

template <int H, int FORM>
__global__ void __launch_bounds__(PT) cross_merge_case(u64* gran, int gran_bytes, unsigned* err, float* out, int* failed) {
  constexpr int D = 64 * H, NPART = H * kCrossSplit * kPS, NPP = NPART / 2, NPP1 = (NPP + 1) / 2, GP1 = (NPP1 + PL - 1) / PL, GP2 = (NPP - NPP1 + CT - 1) / CT;
  constexpr int GD = 2 * ((D / 2 + PL - 1) / PL), O_PART = 0;
  __shared__ __attribute__((aligned(16))) float act[D + NPART];
  __shared__ int ctl[16];
  const int tid = threadIdx.x;
  const bool poller = tid < PL;
  const __amdgpu_buffer_rsrc_t GR = __builtin_amdgcn_make_buffer_rsrc((void*)gran, 0, gran_bytes, 0x27000);
  for (int i = tid; i < D + NPART; i += PT) act[i] = __uint_as_float(0x7FC57FC5u);
  if (tid < 16) ctl[tid] = 0;
  __syncthreads();
  const unsigned tag = kTag;
  bool fail = false;
  if constexpr (FORM == 0) {
    if (!poller) fail = co_gather_merge<D>(GR, tag, O_PART, tid - PL, act, err, ctl);  // the kernel's call: the dealing is the helper's
    if (fail) ctl[0] = 1;
    wg_barrier();
  } else {
    float* pbuf = act + D;
    if (poller) {
      unsigned y[2 * GP1];
      fail = gather2<GP1>(GR, tag, y, err, ctl, [&](int j) { const int pi = tid + j * PL; return pi < NPP1 ? O_PART + (pi / (kPS / 2)) * kRec + 2 * (pi % (kPS / 2)) : -1; });
#pragma unroll
      for (int j = 0; j < GP1; ++j) {
        const int pi = tid + j * PL;
        if (pi < NPP1) { pbuf[2 * pi] = __uint_as_float(y[2 * j]); pbuf[2 * pi + 1] = __uint_as_float(y[2 * j + 1]); }
      }
      if (fail) ctl[0] = 1;
      wg_barrier();
#pragma unroll
      for (int k = 0; k < GD; ++k) {
        const int i = tid + k * PL;
        if (i < D) act[i] = merge_cross_records(pbuf, i);
      }
      wg_barrier();
    } else {
      const int ctid = tid - PL;
      unsigned y[2 * GP2];
      fail = gather2<GP2>(GR, tag, y, err, ctl, [&](int j) { const int pi = NPP1 + ctid + j * CT; return pi < NPP ? O_PART + (pi / (kPS / 2)) * kRec + 2 * (pi % (kPS / 2)) : -1; });
#pragma unroll
      for (int j = 0; j < GP2; ++j) {
        const int pi = NPP1 + ctid + j * CT;
        if (pi < NPP) { pbuf[2 * pi] = __uint_as_float(y[2 * j]); pbuf[2 * pi + 1] = __uint_as_float(y[2 * j + 1]); }
      }
      if (fail) ctl[0] = 1;
      wg_barrier();
      wg_barrier();
    }
  }
  if (ctl[0] && tid == 0) *failed = 1;
  for (int i = tid; i < D; i += PT) out[i] = act[i];
}

#define CHECK(X)                                                                                  \
  do {                                                                                            \
    const hipError_t e_ = (X);                                                                    \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #X, hipGetErrorString(e_)); return 2; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  int n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 1 || n > 4096) { fprintf(stderr, "bad case count\n"); return 1; }
  constexpr int HMAX = 12;
  const size_t gran_n = (size_t)HMAX * kCrossSplit * kRec;
  std::vector<u64> hg(gran_n);
  std::vector<float> rec((size_t)HMAX * kCrossSplit * kPS), res;
  u64* dg;
  unsigned* derr;
  float* dout;
  int* dfail;
  CHECK(hipMalloc(&dg, gran_n * 8));
  CHECK(hipMalloc(&derr, 4));
  CHECK(hipMalloc(&dout, HMAX * 64 * 4));
  CHECK(hipMalloc(&dfail, 4));
  CHECK(hipMemset(derr, 0, 4));
  for (int c = 0; c < n; ++c) {
    int H = 0;
    if (fread(&H, 4, 1, f) != 1 || (H != 2 && H != 12)) { fprintf(stderr, "case %d: heads must be 2 or 12\n", c); return 1; }
    const size_t nrec = (size_t)H * kCrossSplit;
    if (fread(rec.data(), 4, nrec * kPS, f) != nrec * kPS) { fprintf(stderr, "case %d: short read\n", c); return 1; }
    // the records as granules: o[64], m, l of record r at r * kRec; the 14 granules of padding behind each keep tag 0
    std::fill(hg.begin(), hg.end(), 0ull);
    for (size_t r = 0; r < nrec; ++r)
      for (int i = 0; i < kPS; ++i) {
        unsigned bits;
        memcpy(&bits, &rec[r * kPS + i], 4);
        hg[r * kRec + i] = ((u64)kTag << 32) | bits;
      }
    CHECK(hipMemcpy(dg, hg.data(), gran_n * 8, hipMemcpyHostToDevice));
    for (int form = 0; form < 2; ++form) {
      CHECK(hipMemset(dfail, 0, 4));
      CHECK(hipMemset(dout, 0xFF, HMAX * 64 * 4));
      const int gb = (int)(nrec * kRec * 8);
      if (H == 2) {
        if (form == 0) hipLaunchKernelGGL((cross_merge_case<2, 0>), dim3(1), dim3(PT), 0, 0, dg, gb, derr, dout, dfail);
        else hipLaunchKernelGGL((cross_merge_case<2, 1>), dim3(1), dim3(PT), 0, 0, dg, gb, derr, dout, dfail);
      } else {
        if (form == 0) hipLaunchKernelGGL((cross_merge_case<12, 0>), dim3(1), dim3(PT), 0, 0, dg, gb, derr, dout, dfail);
        else hipLaunchKernelGGL((cross_merge_case<12, 1>), dim3(1), dim3(PT), 0, 0, dg, gb, derr, dout, dfail);
      }
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
      int failed = 0;
      CHECK(hipMemcpy(&failed, dfail, 4, hipMemcpyDeviceToHost));
      if (failed) { fprintf(stderr, "case %d form %d: a lane gave up on a record that is complete\n", c, form); return 3; }
      const size_t at = res.size();
      res.resize(at + (size_t)H * 64);
      CHECK(hipMemcpy(res.data() + at, dout, (size_t)H * 64 * 4, hipMemcpyDeviceToHost));
    }
  }
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(res.data(), 4, res.size(), o) != res.size()) { perror(argv[2]); return 1; }
  fclose(o);
  printf("%s cases %d done\n", kDtypeName, n);
  return 0;
}
