// persist_rows_driver.cpp — the weight-row machinery of the persistent launches (csrc/decode_persistent_common.hpp) alone, for
// tests/test_gpu_persist_rows.py: the lane-group reductions, RowSet's prefetch / run / run_ln / publish, rows_dot_reg, the query
// fold's producer and consumer sides and the load-time fold arena. The test kernels use the launch's geometry (1024 threads, pollers
// tid < PL, compute waves ctid = tid - PL, wg_barrier between phases) and spell the calls as decode_persistent.hip does. Linked
// with build/decode_persistent.<dt>.o and build/decode_persistent2.<dt>.o: launch_qfold_build and qfold_floats are the shipped ones.
//
// NO kernel here waits on another workgroup. The one launch that consumes granules (fold_consume: qfold_unit_query) runs after the
// launch that wrote them has finished, and only after the host has seen the tag in every granule it will poll; a give-up (ctl[0])
// is reported as a failure (exit status 3). A case that a launch could not take (a workgroup with more than 2 * SLOTS or more than
// 64 rows, an unknown shape) is refused with exit status 2 before anything is launched.
//
//   persist_rows_driver <cases.bin> <out.bin>
//   cases.bin: int32 n, then per case int32 form and
//     0 reduce    int32 nv; float v[nv][64]                              -> float [nv][6][64]: group_sum<16>, <32>, <64>, wsum, wmax, sum_hi3
//     1 rows      int32 LPR, CH, N, P, NS, first, report, reuse; unless report or reuse (= the previous rows case's inputs): h16 W[N][K]; float b[N], s[N], c[N], x[4][K], mean, rstd
//                 -> int32 own[P][2] (r0, r1 as prefetch computed them); unless report: u64 gran[4][64 + N + 64]
//                 phases: run with bias, run without, run_ln, run published through gelu_erf; workgroup wg deals as rwg = (wg - NS + P) % P
//     2 rows_reg  int32 LD, CD; h16 W[PL / LD][K]; float x[K]            -> float [2][PL]: rows_dot, rows_dot_reg in every lane
//     3 fold      int32 D; h16 w_o[D][D], w_cq[D][D]; float fl[17 D] (one layer of DecArena's floats), a[D], xg[D], x0[D], shift
//                 -> float qf[qfold_stride(D)]; u64 gran[64 + NG + 64]; float dbg[2][D] (A0, M a + d); uint32 qs[H][64]
//     4 arena     int32 D, L; h16 wl[L][14 D D]; float fl[L][17 D]        -> float qf[L][qfold_stride(D)]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "decode_persistent_common.hpp"

using namespace axw;

constexpr unsigned kTag = 0x1234u;
constexpr int kGuard = 64;                         // granules in front of and behind every granule buffer
constexpr u64 kSent = 0x7FC57FC57FC57FC5ull;       // what a granule nobody wrote holds
constexpr unsigned kSent32 = 0x7FC57FC5u;

// ---------------------------------------------------------------------------------------- reduce
__global__ void __launch_bounds__(64) reduce_case(const float* in, float* out) {
  const int lane = threadIdx.x;
  const float v = in[blockIdx.x * 64 + lane];
  float* o = out + (long)blockIdx.x * 6 * 64;
  o[lane] = group_sum<16>(v);
  o[64 + lane] = group_sum<32>(v);
  o[128 + lane] = group_sum<64>(v);
  o[192 + lane] = wsum(v);
  o[256 + lane] = wmax(v);
  o[320 + lane] = sum_hi3(v);
}

// ---------------------------------------------------------------------------------------- rows
struct RowsArgs {
  const h16* W;
  const float *b, *s, *c, *x;
  float mean, rstd;
  int N, NS, first, report;
  u64* g;    // four buffers of kGuard + N + kGuard granules
  int* own;  // [P][2]
};

// One "layer": four phases on one arrival counter (ctl + 2) and one pk[64]; the next phase's rows are requested into the same
// register set before the current phase publishes, a workgroup barrier between phases.
template <int LPR, int CH>
__global__ void __launch_bounds__(PT) rows_case(RowsArgs a) {
  constexpr int K = 8 * LPR * CH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* act = reinterpret_cast<float*>(smem);  // [4][K]: one activation vector per phase
  float* pk = act + 4 * K;
  int* ctl = reinterpret_cast<int*>(pk + 64);
  const int tid = threadIdx.x, P = gridDim.x, wg = blockIdx.x;
  const bool poller = tid < PL;
  const int rwg = (wg - a.NS + P) % P;
  if (!a.report)
    for (int i = tid; i < 4 * K; i += PT) act[i] = a.x[i];
  if (tid < 64) pk[tid] = __uint_as_float(kSent32);
  if (tid < 16) ctl[tid] = 0;
  __syncthreads();
  if (poller) {
    if (!a.report) { wg_barrier(); wg_barrier(); wg_barrier(); }
    return;
  }
  const int ctid = tid - PL;
  const long stride = (long)a.N + 2 * kGuard;
  u64* const G = a.g + kGuard;
  RowSet<LPR, CH> rs;
  float res[2];
  rs.prefetch(a.W, a.b, K, a.N, rwg, P, ctid, a.first);
  if (ctid == 0) { a.own[2 * wg] = rs.r0; a.own[2 * wg + 1] = rs.r1; }
  if (a.report) return;
  // ---- run with a bias
  rs.run(a.W, a.b, K, act, ctid, res);
  {
    const float keep[2] = {res[0], res[1]};
    rs.prefetch(a.W, nullptr, K, a.N, rwg, P, ctid, a.first);
    rs.publish(ctid, keep, pk, ctl + 2, G, kTag, [](float v) { return v; });
  }
  wg_barrier();
  // ---- run with b == nullptr
  rs.run(a.W, nullptr, K, act + K, ctid, res);
  {
    const float keep[2] = {res[0], res[1]};
    rs.prefetch_ln(a.W, a.s, a.c, K, a.N, rwg, P, ctid, a.first);
    rs.publish(ctid, keep, pk, ctl + 2, G + stride, kTag, [](float v) { return v; });
  }
  wg_barrier();
  // ---- run_ln
  rs.run_ln(a.W, a.s, a.c, K, act + 2 * K, ctid, res, a.mean, a.rstd);
  {
    const float keep[2] = {res[0], res[1]};
    rs.prefetch(a.W, a.b, K, a.N, rwg, P, ctid, a.first);
    rs.publish(ctid, keep, pk, ctl + 2, G + 2 * stride, kTag, [](float v) { return v; });
  }
  wg_barrier();
  // ---- run, published through gelu_erf
  rs.run(a.W, a.b, K, act + 3 * K, ctid, res);
  rs.publish(ctid, res, pk, ctl + 2, G + 3 * stride, kTag, [](float v) { return gelu_erf(v); });
}

// ---------------------------------------------------------------------------------------- rows_reg
template <int LD, int CD>
__global__ void __launch_bounds__(PL) rows_reg_case(const h16* W, const float* x, float* out) {
  constexpr int K = 8 * LD * CD;
  __shared__ __attribute__((aligned(16))) float act[K];
  const int tid = threadIdx.x;
  for (int i = tid; i < K; i += PL) act[i] = x[i];
  __syncthreads();
  const int j = tid % LD;
  u32x4 w[CD];
  rows_load<LD, CD>(w, W, K, tid / LD, tid);
  float4 a[CD][2];
#pragma unroll
  for (int i = 0; i < CD; ++i) {
    a[i][0] = *reinterpret_cast<const float4*>(act + (j + LD * i) * 8);
    a[i][1] = *reinterpret_cast<const float4*>(act + (j + LD * i) * 8 + 4);
  }
  int tid2 = tid;
  asm volatile("" : "+v"(tid2));
  out[tid] = rows_dot<LD, CD>(w, act, tid2);
  out[PL + tid] = rows_dot_reg<LD, CD>(w, a);
}

// ---------------------------------------------------------------------------------------- fold
struct FoldArgs {
  const h16 *w_cq, *w_o;
  const float *b_o, *qfl;  // qfl: the layer's block of the fold arena (M, then d, s, c, ...)
  const float *a, *xg, *x0;
  float shift;
  u64* G;  // the clip's granule area (behind the guard)
  int gran_bytes;
  float* dbg;
  unsigned* err;
  int* failed;
  unsigned* qs_out;
};

// The producer side of decode_persistent.hip's query fold: A0 = W_cq (g . x0) while "self-attention runs", then W_o's rows, the rows
// of M, and T, the two sums and y1 published by qfold_publish. Workgroup NP_D of the grid owns no rows and must publish nothing.
template <int LD, int CD, int LF, int CF>
__global__ void __launch_bounds__(PT) fold_produce(FoldArgs p) {
  AXW_PERSIST_SHAPES
  constexpr int XG = D, X0R = 2 * D, A0S = 3 * D;
  constexpr int NP_D = (D + CT / LD - 1) / (CT / LD);
  __shared__ __attribute__((aligned(16))) float act[3 * D + 64];
  __shared__ float red[2 * NPW + 4], pk[64], pscr[64];
  __shared__ int ctl[16];
  const int tid = threadIdx.x, P = gridDim.x, rwg = blockIdx.x;
  for (int i = tid; i < D; i += PT) { act[i] = p.a[i]; act[XG + i] = p.xg[i]; act[X0R + i] = p.x0[i]; }
  if (tid < 64) { act[A0S + tid] = pk[tid] = pscr[tid] = __uint_as_float(kSent32); }
  if (tid < 16) ctl[tid] = 0;
  if (tid == 0) red[2 * NPW] = p.shift;
  __syncthreads();
  if (tid < PL) { wg_barrier(); return; }
  const int ctid = tid - PL, lane = ctid & 63;
  const bool in_o = rwg < NP_D;
  constexpr int pk_d = 0;
  RowSet<LD, CD> ra, rb;
  float res[2];
  if (in_o) {
    ra.prefetch(p.w_cq, nullptr, D, D, rwg, P, ctid, pk_d);
    float ra0[2];
    ra.run(p.w_cq, nullptr, D, act + XG, ctid, ra0);
    if (ctid % LD == 0) act[A0S + ctid / LD] = ra0[0];
  }
  rb.prefetch(p.w_o, p.b_o, D, D, rwg, P, ctid, pk_d);
  if (in_o) {
    const float* qfl = p.qfl;
    const int slot = ctid / LD, row = rb.r0 + slot < rb.r1 ? rb.r0 + slot : rb.r0;
    RowSetF32<LD, CD> rm;
    rm.prefetch(qfl, qfl + (long)D * D, D, row, rb.r0 + slot < rb.r1, ctid);
    wg_barrier();
    rb.run(p.w_o, p.b_o, D, act, ctid, res);
    const float tq = rm.run(act, ctid);
    const int j = ctid % LD, nrows = rb.r1 - rb.r0;
    if (j == 0 && slot < nrows) {
      pk[slot] = res[0];
      pk[32 + slot] = tq + act[A0S + slot];
      pscr[slot] = (act[X0R + rb.r0 + slot] + res[0]) - red[2 * NPW];
      p.dbg[rb.r0 + slot] = act[A0S + slot];
      p.dbg[D + rb.r0 + slot] = tq;
    }
    qfold_publish(lane, pk, pscr, ctl + 2, p.G, O_CQ, O_STAT, O_Y1, rb.r0, nrows, rwg, kTag);
  } else {
    wg_barrier();
  }
}

// A cross-attention unit's side, one workgroup per head, on the granules that fold_produce (finished) left complete.
template <int LD, int CD, int LF, int CF>
__global__ void __launch_bounds__(PT) fold_consume(FoldArgs p) {
  AXW_PERSIST_SHAPES
  constexpr int NP_D = (D + CT / LD - 1) / (CT / LD);
  __shared__ unsigned qs[64];
  __shared__ int ctl[16];
  const int tid = threadIdx.x, ca_head = blockIdx.x;
  if (tid < 64) qs[tid] = kSent32;
  if (tid < 16) ctl[tid] = 0;
  __syncthreads();
  const __amdgpu_buffer_rsrc_t GR = __builtin_amdgcn_make_buffer_rsrc((void*)p.G, 0, p.gran_bytes, 0x27000);
  const unsigned tag = kTag;
  const float shift = p.shift;
  if (tid < PL) {
    const bool fail = qfold_unit_query<D, NP_D>(GR, tag, tid, O_CQ, O_STAT, p.qfl + (long)D * D, ca_head, shift, qs, p.err, ctl);
    if (fail) ctl[0] = 1;
  }
  __syncthreads();
  if (ctl[0] && tid == 0) *p.failed = 1;
  if (tid < 64) p.qs_out[ca_head * 64 + tid] = qs[tid];
}

// the launch's granule offsets of a shape (AXW_PERSIST_SHAPES), for the host and for the printed layout
struct FoldLayout { int y1, cq, stat, np_d, heads; };
template <int LD, int CD, int LF, int CF>
FoldLayout fold_layout() {
  AXW_PERSIST_SHAPES
  (void)GD; (void)GP1; (void)GP2; (void)NU; (void)O_QKV; (void)O_ATT; (void)O_PART; (void)O_Y2; (void)O_HID; (void)O_Y3; (void)O_AMAX;
  return FoldLayout{O_Y1, O_CQ, O_STAT, (D + CT / LD - 1) / (CT / LD), H};
}

// ---------------------------------------------------------------------------------------- host
#define CHECK(X)                                                                                 \
  do {                                                                                            \
    const hipError_t e_ = (X);                                                                    \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #X, hipGetErrorString(e_)); return 4; } \
  } while (0)

struct Reader {
  std::vector<char> buf;
  size_t at = 0;
  bool take(void* dst, size_t n) {
    if (at + n > buf.size()) return false;
    memcpy(dst, buf.data() + at, n);
    at += n;
    return true;
  }
  const char* span(size_t n) {
    if (at + n > buf.size()) return nullptr;
    const char* p = buf.data() + at;
    at += n;
    return p;
  }
};

template <typename T>
static hipError_t upload(T** d, const char* src, size_t n) {
  hipError_t e = hipMalloc(d, n * sizeof(T) + 16);
  if (e != hipSuccess) return e;
  return hipMemcpy(*d, src, n * sizeof(T), hipMemcpyHostToDevice);
}
static void append(std::vector<char>& out, const void* p, size_t n) { out.insert(out.end(), (const char*)p, (const char*)p + n); }

// prefetch()'s deal on the host: what a launch may be given
static bool deal_ok(int lpr, int N, int P, int NS, int first) {
  const int slots = CT / lpr;
  for (int wg = 0; wg < P; ++wg) {
    const int rwg = (wg - NS + P) % P;
    long r0, r1;
    if (first < 0) {
      r0 = (long)rwg * N / P;
      r1 = (long)(rwg + 1) * N / P;
    } else {
      int pidx = rwg - first;
      if (pidx < 0) pidx += P;
      r0 = (long)pidx * slots < N ? (long)pidx * slots : 0;
      r1 = (long)pidx * slots < N ? (r0 + slots < N ? r0 + slots : N) : 0;
    }
    if (r1 - r0 > 2 * slots || r1 - r0 > 64 || r1 > N || r0 < 0) return false;
  }
  if (first >= 0 && (first >= P || (long)P * slots < N)) return false;  // every row needs a producer
  return true;
}

#define ROW_SHAPES(X) X(16, 1) X(32, 1) X(16, 3) X(32, 2) X(32, 3) X(32, 5) X(64, 2) X(64, 3) X(64, 4) X(64, 6) X(64, 10)
#define REG_SHAPES(X) X(16, 1) X(32, 1) X(16, 3) X(32, 2) X(32, 3)
#define FOLD_SHAPES(X) X(16, 1, 32, 2) X(32, 1, 64, 2) X(16, 3, 64, 3) X(32, 2, 64, 4) X(32, 3, 64, 6)

static int run_reduce(Reader& in, std::vector<char>& out) {
  int nv = 0;
  if (!in.take(&nv, 4) || nv < 1 || nv > 4096) return 2;
  const char* v = in.span((size_t)nv * 64 * 4);
  if (!v) return 2;
  float *dv, *dout;
  CHECK(upload(&dv, v, (size_t)nv * 64));
  CHECK(hipMalloc(&dout, (size_t)nv * 6 * 64 * 4));
  hipLaunchKernelGGL(reduce_case, dim3(nv), dim3(64), 0, 0, dv, dout);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> h((size_t)nv * 6 * 64);
  CHECK(hipMemcpy(h.data(), dout, h.size() * 4, hipMemcpyDeviceToHost));
  append(out, h.data(), h.size() * 4);
  CHECK(hipFree(dv));
  CHECK(hipFree(dout));
  printf("ran reduce %d\n", nv);
  return 0;
}

// the inputs of the last rows case that carried some: a case with reuse = 1 runs another deal on the same (W, b, s, c, x, mean, rstd)
static struct { h16* W = nullptr; float *b = nullptr, *s = nullptr, *c = nullptr, *x = nullptr; float mean = 0.f, rstd = 0.f; int N = 0, K = 0; } g_rows;

static int run_rows(Reader& in, std::vector<char>& out) {
  int h[8];
  if (!in.take(h, sizeof h)) return 2;
  const int LPR = h[0], CH = h[1], N = h[2], P = h[3], NS = h[4], first = h[5], report = h[6], reuse = h[7];
  const int K = 8 * LPR * CH;
  bool known = false;
#define X(L, C) known |= (LPR == L && CH == C);
  ROW_SHAPES(X)
#undef X
  if (!known || N < 1 || N > 65536 || P < 1 || P > 256 || NS < 0 || NS >= P) { fprintf(stderr, "rows: no such shape or grid\n"); return 2; }
  if (!report && !deal_ok(LPR, N, P, NS, first)) { fprintf(stderr, "rows: a workgroup would own more than 2 * SLOTS or 64 rows\n"); return 2; }
  if (report && (first >= 0 || reuse)) return 2;
  if (reuse && (!g_rows.W || g_rows.N != N || g_rows.K != K)) { fprintf(stderr, "rows: nothing to reuse\n"); return 2; }
  RowsArgs a{};
  h16* dW = nullptr;
  const size_t gn = 4 * ((size_t)N + 2 * kGuard);
  if (report) {
    CHECK(hipMalloc(&dW, (size_t)N * K * 2));
    CHECK(hipMemset(dW, 0, (size_t)N * K * 2));
    a.W = dW;
  } else {
    if (!reuse) {
      for (void* q : {(void*)g_rows.W, (void*)g_rows.b, (void*)g_rows.s, (void*)g_rows.c, (void*)g_rows.x})
        if (q) CHECK(hipFree(q));
      g_rows.W = nullptr;
      const char *w = in.span((size_t)N * K * 2), *b = in.span((size_t)N * 4), *s = in.span((size_t)N * 4), *c = in.span((size_t)N * 4), *x = in.span((size_t)4 * K * 4);
      if (!w || !b || !s || !c || !x || !in.take(&g_rows.mean, 4) || !in.take(&g_rows.rstd, 4)) return 2;
      CHECK(upload(&g_rows.W, w, (size_t)N * K));
      CHECK(upload(&g_rows.b, b, N));
      CHECK(upload(&g_rows.s, s, N));
      CHECK(upload(&g_rows.c, c, N));
      CHECK(upload(&g_rows.x, x, (size_t)4 * K));
      g_rows.N = N;
      g_rows.K = K;
    }
    a.W = g_rows.W; a.b = g_rows.b; a.s = g_rows.s; a.c = g_rows.c; a.x = g_rows.x; a.mean = g_rows.mean; a.rstd = g_rows.rstd;
  }
  std::vector<u64> hg(gn, kSent);
  std::vector<int> hown((size_t)2 * P, -1);
  u64* dg;
  int* down;
  CHECK(hipMalloc(&dg, gn * 8));
  CHECK(hipMemcpy(dg, hg.data(), gn * 8, hipMemcpyHostToDevice));
  CHECK(hipMalloc(&down, hown.size() * 4));
  CHECK(hipMemcpy(down, hown.data(), hown.size() * 4, hipMemcpyHostToDevice));
  a.N = N; a.NS = NS; a.first = first; a.report = report; a.g = dg; a.own = down;
  const size_t lds = (size_t)4 * K * 4 + 64 * 4 + 16 * 4;
#define X(L, C)                                                                                                              \
  if (LPR == L && CH == C) {                                                                                                 \
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rows_case<L, C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL((rows_case<L, C>), dim3(P), dim3(PT), lds, 0, a);                                                     \
  }
  ROW_SHAPES(X)
#undef X
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(hown.data(), down, hown.size() * 4, hipMemcpyDeviceToHost));
  append(out, hown.data(), hown.size() * 4);
  if (!report) {
    CHECK(hipMemcpy(hg.data(), dg, gn * 8, hipMemcpyDeviceToHost));
    append(out, hg.data(), gn * 8);
  }
  if (dW) CHECK(hipFree(dW));
  CHECK(hipFree(dg));
  CHECK(hipFree(down));
  printf("ran rows %d %d N %d P %d NS %d first %d report %d\n", LPR, CH, N, P, NS, first, report);
  return 0;
}

static int run_rows_reg(Reader& in, std::vector<char>& out) {
  int h[2];
  if (!in.take(h, sizeof h)) return 2;
  const int LD = h[0], CD = h[1], K = 8 * LD * CD;
  bool known = false;
#define X(L, C) known |= (LD == L && CD == C);
  REG_SHAPES(X)
#undef X
  if (!known) { fprintf(stderr, "rows_reg: no such shape\n"); return 2; }
  const int R = PL / LD;
  const char *w = in.span((size_t)R * K * 2), *x = in.span((size_t)K * 4);
  if (!w || !x) return 2;
  h16* dW;
  float *dx, *dout;
  CHECK(upload(&dW, w, (size_t)R * K));
  CHECK(upload(&dx, x, K));
  CHECK(hipMalloc(&dout, 2 * PL * 4));
#define X(L, C) \
  if (LD == L && CD == C) hipLaunchKernelGGL((rows_reg_case<L, C>), dim3(1), dim3(PL), 0, 0, dW, dx, dout);
  REG_SHAPES(X)
#undef X
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> ho(2 * PL);
  CHECK(hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost));
  append(out, ho.data(), ho.size() * 4);
  CHECK(hipFree(dW));
  CHECK(hipFree(dx));
  CHECK(hipFree(dout));
  printf("ran rows_reg %d %d\n", LD, CD);
  return 0;
}

static int run_fold(Reader& in, std::vector<char>& out) {
  int D = 0;
  if (!in.take(&D, 4)) return 2;
  int LD = 0, CD = 0;
  FoldLayout lay{};
#define X(A, B, C, E) \
  if (D == 8 * A * B) { LD = A; CD = B; lay = fold_layout<A, B, C, E>(); }
  FOLD_SHAPES(X)
#undef X
  if (!LD) { fprintf(stderr, "fold: d_model %d has no query fold\n", D); return 2; }
  const long DD = (long)D * D;
  const int H = lay.heads, NP_D = lay.np_d;
  const int O_Y1 = lay.y1, O_CQ = lay.cq, O_STAT = lay.stat;
  const int NG = O_STAT + 16 * NP_D;
  const char *wo = in.span(DD * 2), *wcq = in.span(DD * 2), *fl = in.span((size_t)17 * D * 4), *av = in.span((size_t)D * 4), *xg = in.span((size_t)D * 4),
             *x0 = in.span((size_t)D * 4);
  float shift;
  if (!wo || !wcq || !fl || !av || !xg || !x0 || !in.take(&shift, 4)) return 2;
  // one layer of both arenas; the units this form does not read stay zero
  h16* dwl;
  float *dfl, *dqf, *da, *dxg, *dx0, *ddbg;
  CHECK(hipMalloc(&dwl, DecArena::w_stride(D) * 2));
  CHECK(hipMemset(dwl, 0, DecArena::w_stride(D) * 2));
  CHECK(hipMemcpy(dwl + DecArena::W_O * DD, wo, DD * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dwl + DecArena::W_CQ * DD, wcq, DD * 2, hipMemcpyHostToDevice));
  CHECK(upload(&dfl, fl, (size_t)17 * D));
  const size_t nqf = qfold_floats(D, 1);
  CHECK(hipMalloc(&dqf, nqf * 4));
  CHECK(hipMemset(dqf, 0xFF, nqf * 4));
  launch_qfold_build(dwl, dfl, dqf, D, 1, 0);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(upload(&da, av, D));
  CHECK(upload(&dxg, xg, D));
  CHECK(upload(&dx0, x0, D));
  CHECK(hipMalloc(&ddbg, (size_t)2 * D * 4));
  CHECK(hipMemset(ddbg, 0xFF, (size_t)2 * D * 4));
  const size_t gn = (size_t)NG + 2 * kGuard;
  std::vector<u64> hg(gn, kSent);
  u64* dg;
  unsigned *derr, *dqs;
  int* dfail;
  CHECK(hipMalloc(&dg, gn * 8));
  CHECK(hipMemcpy(dg, hg.data(), gn * 8, hipMemcpyHostToDevice));
  CHECK(hipMalloc(&derr, 4));
  CHECK(hipMemset(derr, 0, 4));
  CHECK(hipMalloc(&dfail, 4));
  CHECK(hipMemset(dfail, 0, 4));
  CHECK(hipMalloc(&dqs, (size_t)H * 64 * 4));
  CHECK(hipMemset(dqs, 0xFF, (size_t)H * 64 * 4));
  FoldArgs p{};
  p.w_cq = dwl + DecArena::W_CQ * DD; p.w_o = dwl + DecArena::W_O * DD;
  p.b_o = dfl + DecArena::F_B_O * D; p.qfl = dqf;
  p.a = da; p.xg = dxg; p.x0 = dx0; p.shift = shift;
  p.G = dg + kGuard; p.gran_bytes = NG * 8; p.dbg = ddbg; p.err = derr; p.failed = dfail; p.qs_out = dqs;
#define X(A, B, C, E) \
  if (LD == A && CD == B) hipLaunchKernelGGL((fold_produce<A, B, C, E>), dim3(NP_D + 1), dim3(PT), 0, 0, p);
  FOLD_SHAPES(X)
#undef X
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(hg.data(), dg, gn * 8, hipMemcpyDeviceToHost));
  // the consumer polls T [D] and the two statistics of every producer: all of them must carry the tag before it is launched
  bool complete = true;
  for (int i = 0; i < D; ++i) complete &= (unsigned)(hg[kGuard + O_CQ + i] >> 32) == kTag && (unsigned)(hg[kGuard + O_Y1 + i] >> 32) == kTag;
  for (int q = 0; q < NP_D; ++q)
    for (int e = 0; e < 2; ++e) complete &= (unsigned)(hg[kGuard + O_STAT + 16 * q + e] >> 32) == kTag;
  std::vector<float> hqf(nqf), hdbg((size_t)2 * D);
  std::vector<unsigned> hqs((size_t)H * 64, kSent32);
  int failed = 0;
  if (complete) {
#define X(A, B, C, E) \
  if (LD == A && CD == B) hipLaunchKernelGGL((fold_consume<A, B, C, E>), dim3(H), dim3(PT), 0, 0, p);
    FOLD_SHAPES(X)
#undef X
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&failed, dfail, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hqs.data(), dqs, hqs.size() * 4, hipMemcpyDeviceToHost));
  }
  if (failed) { fprintf(stderr, "fold %d: a lane gave up on a granule that is complete\n", D); return 3; }
  CHECK(hipMemcpy(hqf.data(), dqf, nqf * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hdbg.data(), ddbg, hdbg.size() * 4, hipMemcpyDeviceToHost));
  append(out, hqf.data(), nqf * 4);
  append(out, hg.data(), gn * 8);
  append(out, hdbg.data(), hdbg.size() * 4);
  append(out, hqs.data(), hqs.size() * 4);
  for (void* q : {(void*)dwl, (void*)dfl, (void*)dqf, (void*)da, (void*)dxg, (void*)dx0, (void*)ddbg, (void*)dg, (void*)derr, (void*)dfail, (void*)dqs}) CHECK(hipFree(q));
  printf("ran fold %d complete %d O_Y1 %d O_CQ %d O_STAT %d NP_D %d NG %d qfold_stride %ld\n", D, complete ? 1 : 0, O_Y1, O_CQ, O_STAT, NP_D, NG, qfold_stride(D));
  return 0;
}

static int run_arena(Reader& in, std::vector<char>& out) {
  int h[2];
  if (!in.take(h, sizeof h)) return 2;
  const int D = h[0], L = h[1];
  if (D < 64 || D > 768 || D % 64 || L < 1 || L > 4) { fprintf(stderr, "arena: no such shape\n"); return 2; }
  const size_t nw = (size_t)L * DecArena::w_stride(D), nf = (size_t)L * DecArena::f_stride(D), nq = qfold_floats(D, L);
  const char *wl = in.span(nw * 2), *fl = in.span(nf * 4);
  if (!wl || !fl) return 2;
  h16* dwl;
  float *dfl, *dqf;
  CHECK(upload(&dwl, wl, nw));
  CHECK(upload(&dfl, fl, nf));
  CHECK(hipMalloc(&dqf, nq * 4));
  CHECK(hipMemset(dqf, 0xFF, nq * 4));
  launch_qfold_build(dwl, dfl, dqf, D, L, 0);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> hq(nq);
  CHECK(hipMemcpy(hq.data(), dqf, nq * 4, hipMemcpyDeviceToHost));
  append(out, hq.data(), nq * 4);
  CHECK(hipFree(dwl));
  CHECK(hipFree(dfl));
  CHECK(hipFree(dqf));
  printf("ran arena %d %d\n", D, L);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 1; }
  Reader in;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    in.buf.resize(n);
    if (fread(in.buf.data(), 1, n, f) != (size_t)n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);
  }
  // the layout this build was compiled with: Python hard-codes none of it
  printf("layout PT %d PL %d CT %d NCW %d guard %d tag %u W_O %d W_CQ %d W_QKV %d W_FC1 %d W_UNITS %d F_ATTN_LN_W %d F_ATTN_LN_B %d F_B_QKV %d F_B_O %d "
         "F_CROSS_LN_W %d F_CROSS_LN_B %d F_B_CQ %d F_MLP_LN_W %d F_MLP_LN_B %d F_B_FC1 %d F_UNITS %d QF_SQKV %d QF_CQKV %d QF_SFC1 %d QF_CFC1 %d "
         "W_CO %d W_FC2 %d F_B_CO %d F_B_FC2 %d\n",
         PT, PL, CT, NCW, kGuard, kTag, DecArena::W_O, DecArena::W_CQ, DecArena::W_QKV, DecArena::W_FC1, DecArena::W_UNITS, DecArena::F_ATTN_LN_W,
         DecArena::F_ATTN_LN_B, DecArena::F_B_QKV, DecArena::F_B_O, DecArena::F_CROSS_LN_W, DecArena::F_CROSS_LN_B, DecArena::F_B_CQ,
         DecArena::F_MLP_LN_W, DecArena::F_MLP_LN_B, DecArena::F_B_FC1, DecArena::F_UNITS, QF_SQKV, QF_CQKV, QF_SFC1, QF_CFC1,
         DecArena::W_CO, DecArena::W_FC2, DecArena::F_B_CO, DecArena::F_B_FC2);
  int n = 0;
  if (!in.take(&n, 4) || n < 1 || n > 4096) { fprintf(stderr, "bad case count\n"); return 1; }
  std::vector<char> out;
  for (int c = 0; c < n; ++c) {
    int form = -1;
    if (!in.take(&form, 4)) { fprintf(stderr, "case %d: short read\n", c); return 2; }
    int rc;
    switch (form) {
      case 0: rc = run_reduce(in, out); break;
      case 1: rc = run_rows(in, out); break;
      case 2: rc = run_rows_reg(in, out); break;
      case 3: rc = run_fold(in, out); break;
      case 4: rc = run_arena(in, out); break;
      default: fprintf(stderr, "case %d: no form %d\n", c, form); return 2;
    }
    if (rc) { fprintf(stderr, "case %d (form %d): status %d\n", c, form, rc); return rc; }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) { perror(argv[2]); return 1; }
  fclose(o);
  printf("%s cases %d done\n", kDtypeName, n);
  return 0;
}
