// persist_ts_driver.cpp — the pieces of the persistent launch's rules instantiation (csrc/decode_persistent_rules.hpp, and
// allowed_sets_from_state of csrc/decode_rules.hpp) alone, for tests/test_gpu_persist_ts_kernels.py. The test kernels use the launch's
// geometry (1024 threads, pollers tid < PL, compute waves ctid = tid - PL, wg_barrier between phases) and the lane layout of its two
// row loops — slot ctid / LD of the compute waves streams rows r0 + slot, + SD, ..; slot tid / LD of the pollers keeps the resident
// tail — on logits the host supplies in place of the dot products, and spell the calls as decode_persistent.hip does.
//
// NO kernel here waits on another workgroup: the merge launch runs after the launch that published has finished, so every granule it
// polls already carries the tag; a give-up is reported as a failure (exit status 3).
//
//   persist_ts_driver <cases.bin> <out.bin>
//   cases.bin: int32 n, then per case int32 form and
//     0 sets   int32 T, E, nv, n; int32 ids[n]      -> int32 [2][6]: text_on, eot_on, ts_lo, ts_hi, text_begin, text_end of
//                                                       allowed_sets (the history scan), then of allowed_sets_from_state
//     1 step   int32 T, E, nv, P, LD, resident, whole, no_speech_id, has_mask, n; int32 ids[n]; float x[nv]; uint32 mask[(nv + 127) / 128 * 4]
//              -> uint32 rec[P][8] (the published records); int32 id; float value, logprob (the decision; whole: id = si, value = sv,
//                 logprob = logprob_of(sv, mt, st)); uint32 grid[8] (the merged record)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "decode_persistent_rules.hpp"

using namespace axw;

constexpr unsigned kTag = 0x51u;
constexpr int kMaxHist = 448;
constexpr int kSupWords = 576;  // the suppress image here covers the ranges of P = 3 as well (the launch's own: kRulesSupWords, P >= 26)

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); }     \
  } while (0)

// ---------------------------------------------------------------------------------------- sets
__global__ void __launch_bounds__(256) sets_case(const int* ids, int n, int T, int E, int nv, int* out) {
  const AllowedSets a = allowed_sets(ids, n, T, E, nv);  // one barrier: all 256 threads
  RulesState h{-1, false, false};
  for (int i = 0; i < n; ++i) rules_state_push(h, ids[i], T);
  const AllowedSets b = allowed_sets_from_state(n, h.last_ts, h.last_is_ts, h.penult_is_ts, T, E, nv);
  if (threadIdx.x == 0) {
    const AllowedSets* s[2] = {&a, &b};
    for (int k = 0; k < 2; ++k) {
      out[6 * k + 0] = s[k]->text_on; out[6 * k + 1] = s[k]->eot_on; out[6 * k + 2] = s[k]->ts_lo; out[6 * k + 3] = s[k]->ts_hi;
      out[6 * k + 4] = s[k]->text_begin; out[6 * k + 5] = s[k]->text_end;
    }
  }
}

// ---------------------------------------------------------------------------------------- step: records of P workgroups
struct StepArgs {
  const float* x; const int* ids; const unsigned* mask;
  int T, E, nv, LD, resident, whole, no_speech_id, n;
  u64* gran; int gran_bytes;
  int* dec; unsigned* grid; unsigned* err;
};

// launch 1: every workgroup's record over its range [wg N / P, (wg + 1) N / P), both row loops, the fold and the publish
__global__ void __launch_bounds__(PT) step_publish(StepArgs p) {
  __shared__ unsigned rec_c[NCW * kRecWords], rec_p[NPW * kRecWords], sup[kSupWords];
  const int tid = threadIdx.x, P = gridDim.x, wg = blockIdx.x, LD = p.LD;
  const unsigned N = (unsigned)p.nv;
  const int v0 = (int)((unsigned)wg * N / (unsigned)P), v1 = (int)((unsigned)(wg + 1) * N / (unsigned)P);
  if (tid < kSupWords) {
    const int wi = (v0 >> 5) + tid;
    sup[tid] = (p.mask && wi <= (int)((N - 1) >> 5)) ? p.mask[wi] : 0u;
  }
  __syncthreads();
  RulesState h{-1, false, false};
  for (int i = 0; i < p.n; ++i) rules_state_push(h, p.ids[i], p.T);
  RulesStep q;
  q.E = p.E; q.no_speech_id = p.no_speech_id; q.w0 = v0 >> 5; q.whole = p.whole != 0;
  q.a = allowed_sets_from_state(p.n, h.last_ts, h.last_is_ts, h.penult_is_ts, p.T, p.E, p.nv);
  const int VCAP = p.resident;  // rows of the resident tail (0: none)
  const int nres = VCAP > 0 ? (v1 - v0 > VCAP ? VCAP : v1 - v0) : 0;
  RulesRec rec = rules_rec_empty();
  if (tid < PL) {  // the pollers' resident rows: passes of PL / LD rows
    const int vb = v1 - nres;
    if (vb < v1) {
      for (int k = 0; vb + k * (PL / LD) < v1; ++k) {
        const int row = vb + k * (PL / LD) + tid / LD;
        if (tid % LD == 0 && row < v1) rules_rec_row(rec, q, sup, p.x[row], row);
      }
      rules_rec_wave_reduce(rec);
      if ((tid & 63) == 0) rules_rec_store(rec_p + (tid >> 6) * kRecWords, rec);
    }
    wg_barrier();  // B3
  } else {  // the compute waves' streamed rows
    const int ctid = tid - PL, SD = CT / LD, slot = ctid / LD, j = ctid % LD, lane = ctid & 63, cw = ctid >> 6;
    const int r0 = v0, r1 = v1 - nres;
    for (int row = r0 + slot; row < r1; row += SD)
      if (j == 0) rules_rec_row(rec, q, sup, p.x[row], row);
    rules_rec_wave_reduce(rec);
    if (lane == 0) rules_rec_store(rec_c + cw * kRecWords, rec);
    wg_barrier();  // B3
    if (cw == 0) {
      const RulesRec wr = rules_rec_fold(rec_c, rec_p, nres > 0, lane);
      if (lane < kRecWords) gput_u(p.gran + kRecWords * wg + lane, kTag, rules_rec_word(wr, lane));
    }
  }
}

// launch 2 (after launch 1 has finished): the pollers' gather of the P records, the merge and the decision
__global__ void __launch_bounds__(PL) step_merge(StepArgs p, int P) {
  __shared__ unsigned rec_g[NPW * 4];
  __shared__ int ctl[16];
  const int tid = threadIdx.x;
  if (tid < 16) ctl[tid] = 0;
  __syncthreads();
  const __amdgpu_buffer_rsrc_t GR = __builtin_amdgcn_make_buffer_rsrc((void*)p.gran, 0, p.gran_bytes, 0x27000);
  unsigned v[4];
  const int gw = tid & 255;
  const bool fail = gather2<2>(GR, kTag, v, p.err, ctl, [&](int k) { return gw < P ? kRecWords * gw + (tid >> 8) * 4 + 2 * k : -1; });
  float r0 = __uint_as_float(v[0]), r2 = __uint_as_float(v[2]);
  if (tid < 256) {
    int i0 = (int)v[1], i1 = (int)v[3];
    if (gw >= P) { r0 = -INFINITY; i0 = 0x7fffffff; r2 = -INFINITY; i1 = 0x7fffffff; }
    wave_argmax(r0, i0);
    wave_argmax(r2, i1);
    if ((tid & 63) == 0) { unsigned* o = rec_g + 4 * (tid >> 6); o[0] = __float_as_uint(r0); o[1] = (unsigned)i0; o[2] = __float_as_uint(r2); o[3] = (unsigned)i1; }
  } else {
    float r1 = __uint_as_float(v[1]), r3 = __uint_as_float(v[3]);
    if (gw >= P) { r0 = -INFINITY; r1 = 0.f; r2 = -INFINITY; r3 = 0.f; }
    lse_wave_reduce_dpp(r0, r1);
    lse_wave_reduce_dpp(r2, r3);
    if ((tid & 63) == 0) { unsigned* o = rec_g + 4 * (tid >> 6); o[0] = __float_as_uint(r0); o[1] = __float_as_uint(r1); o[2] = __float_as_uint(r2); o[3] = __float_as_uint(r3); }
  }
  if (fail) ctl[0] = 1;
  wg_barrier();
  if (tid != 0) return;
  if (ctl[0]) { p.err[0] = 1u; return; }
  const RulesRec g = rules_rec_grid(rec_g);
  rules_rec_store(p.grid, g);
  if (p.whole) {
    p.dec[0] = g.si;
    reinterpret_cast<float*>(p.dec)[1] = g.sv;
    reinterpret_cast<float*>(p.dec)[2] = rules_no_speech_logprob(g);
  } else {
    const RulesDecision d = rules_decide(g, p.E);
    p.dec[0] = d.id;
    reinterpret_cast<float*>(p.dec)[1] = d.value;
    reinterpret_cast<float*>(p.dec)[2] = d.logprob;
  }
}

template <typename T>
static T* dev(const void* src, size_t n) {
  T* d = nullptr;
  CHECK(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
  if (src && n) CHECK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: persist_ts_driver <cases.bin> <out.bin>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<char> in;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + n);
  fclose(f);
  size_t pos = 0;
  auto need = [&](size_t n) { if (pos + n > in.size()) { fprintf(stderr, "cases.bin is cut short\n"); exit(2); } };
  auto geti = [&]() { need(4); int v; memcpy(&v, &in[pos], 4); pos += 4; return v; };
  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  const int n_cases = geti();
  for (int c = 0; c < n_cases; ++c) {
    const int form = geti();
    if (form == 0) {
      const int T = geti(), E = geti(), nv = geti(), n = geti();
      if (n < 0 || n > kMaxHist) { fprintf(stderr, "case %d: history of %d ids\n", c, n); return 2; }
      need((size_t)n * 4);
      int* d_ids = dev<int>(&in[pos], n);
      pos += (size_t)n * 4;
      int* d_out = dev<int>(nullptr, 12);
      hipLaunchKernelGGL(sets_case, dim3(1), dim3(256), 0, 0, d_ids, n, T, E, nv, d_out);
      CHECK(hipDeviceSynchronize());
      int h[12];
      CHECK(hipMemcpy(h, d_out, sizeof h, hipMemcpyDeviceToHost));
      fwrite(h, 4, 12, out);
      CHECK(hipFree(d_ids)); CHECK(hipFree(d_out));
    } else if (form == 1) {
      StepArgs p{};
      p.T = geti(); p.E = geti(); p.nv = geti();
      const int P = geti();
      p.LD = geti(); p.resident = geti(); p.whole = geti(); p.no_speech_id = geti();
      const int has_mask = geti();
      p.n = geti();
      const size_t mw = ((size_t)p.nv + 127) / 128 * 4;
      if (P < 1 || P > 256 || (p.LD != 16 && p.LD != 32) || p.n < 0 || p.n > kMaxHist || p.nv < 1 || p.nv / P + 1 > kSupWords * 32 - 32 || p.resident < 0 ||
          p.resident % (PL / p.LD) != 0 || p.T <= p.E || p.T > p.nv) {
        fprintf(stderr, "case %d: refused (P %d LD %d nv %d resident %d)\n", c, P, p.LD, p.nv, p.resident);
        return 2;
      }
      need((size_t)p.n * 4 + (size_t)p.nv * 4 + mw * 4);
      int* d_ids = dev<int>(&in[pos], p.n); pos += (size_t)p.n * 4;
      float* d_x = dev<float>(&in[pos], p.nv); pos += (size_t)p.nv * 4;
      unsigned* d_mask = dev<unsigned>(&in[pos], mw); pos += mw * 4;
      const size_t ng = (size_t)kRecWords * 256 + 64;  // the records, then slack for the 16-byte polls; the error word apart
      u64* d_gran = dev<u64>(nullptr, ng);
      CHECK(hipMemset(d_gran, 0, ng * 8));
      int* d_dec = dev<int>(nullptr, 4);
      unsigned* d_grid = dev<unsigned>(nullptr, 8);
      unsigned* d_err = dev<unsigned>(nullptr, 2);
      CHECK(hipMemset(d_err, 0, 8));
      p.x = d_x; p.ids = d_ids; p.mask = has_mask ? d_mask : nullptr;
      p.gran = d_gran; p.gran_bytes = (int)(ng * 8); p.dec = d_dec; p.grid = d_grid; p.err = d_err;
      hipLaunchKernelGGL(step_publish, dim3(P), dim3(PT), 0, 0, p);
      CHECK(hipDeviceSynchronize());  // the merge launch polls granules that are all there
      hipLaunchKernelGGL(step_merge, dim3(1), dim3(PL), 0, 0, p, P);
      CHECK(hipDeviceSynchronize());
      unsigned err[2];
      CHECK(hipMemcpy(err, d_err, 8, hipMemcpyDeviceToHost));
      if (err[0]) { fprintf(stderr, "case %d: the merge launch gave up\n", c); return 3; }
      std::vector<u64> g((size_t)kRecWords * P);
      CHECK(hipMemcpy(g.data(), d_gran, g.size() * 8, hipMemcpyDeviceToHost));
      for (u64 w : g) {
        if ((unsigned)(w >> 32) != kTag) { fprintf(stderr, "case %d: a record granule without its tag\n", c); return 3; }
        const unsigned v = (unsigned)w;
        fwrite(&v, 4, 1, out);
      }
      int dec[4]; unsigned grid[8];
      CHECK(hipMemcpy(dec, d_dec, 16, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(grid, d_grid, 32, hipMemcpyDeviceToHost));
      fwrite(dec, 4, 3, out);
      fwrite(grid, 4, 8, out);
      for (void* q : {(void*)d_ids, (void*)d_x, (void*)d_mask, (void*)d_gran, (void*)d_dec, (void*)d_grid, (void*)d_err}) CHECK(hipFree(q));
    } else {
      fprintf(stderr, "case %d: unknown form %d\n", c, form);
      return 2;
    }
  }
  fclose(out);
  return 0;
}
