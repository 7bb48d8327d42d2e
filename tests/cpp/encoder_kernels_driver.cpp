// Runs the encoder kernels that go into libax_whisper.so one launch at a time, for tests/test_gpu_encoder_kernels.py.
// Host-only code, built twice (-DAXW_F16=0 / 1) and linked against the objects `make` produced (build/gemm.{bf16,f16}.o,
// build/encoder_attn.{bf16,f16}.o): the library has hidden visibility, and a recompilation would not be the shipped code.
//
//   encoder_kernels_driver <manifest>       one command per line, executed in order:
//     alloc NAME BYTES FILE|-     device buffer with GUARD sentinel bytes before and after; content from FILE (raw), "-": sentinel
//     reset NAME                  initial content again (guards included)
//     dump NAME FILE [BASE]       the whole allocation, guards included; with BASE: nothing is written (and "same FILE" printed)
//                                 when the content equals that of the earlier dump BASE bit for bit
//     free NAME
//     gemm ID key=value ...       one launch_gemm under gemm_force_tile = force; prints "ran ID <kernel of the launch before> <last kernel>"
//     ln ID key=value ...         one launch_layernorm_bf16
//     attn ID key=value ...       one launch_encoder_attention
// Buffers are named; offsets and strides are in elements, as GemmParams has them. Every launch is checked against the
// sizes of the buffers it names before it runs, and synchronised and checked for errors after.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "common.hpp"

namespace axw {
inline namespace AXW_NS {
extern int gemm_force_tile, gemm_last_kernel, gemm_prev_kernel;
}
}  // namespace axw
using namespace axw;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(3); } } while (0)
static void die(const std::string& m) { fprintf(stderr, "driver: %s\n", m.c_str()); exit(2); }

constexpr size_t GUARD = 4096;
constexpr unsigned short SENT16 = 0x7fc5;

struct Buf { char* dev = nullptr; size_t bytes = 0; std::vector<char> init; };
static std::map<std::string, Buf> bufs;

static Buf& buf(const std::string& n) {
  auto it = bufs.find(n);
  if (it == bufs.end()) die("no buffer " + n);
  return it->second;
}
typedef std::map<std::string, std::string> KV;
static long num(const KV& kv, const char* k, long dflt = 0) { auto it = kv.find(k); return it == kv.end() ? dflt : atol(it->second.c_str()); }
static double real(const KV& kv, const char* k, double dflt = 0) { auto it = kv.find(k); return it == kv.end() ? dflt : atof(it->second.c_str()); }
static bool has(const KV& kv, const char* k) { auto it = kv.find(k); return it != kv.end() && it->second != "-"; }
// pointer to element `off` (of `esz` bytes) of a named buffer, checked to hold `count` elements from there
static void* ptr(const KV& kv, const char* k, size_t esz, long off, long count) {
  if (!has(kv, k)) return nullptr;
  Buf& b = buf(kv.at(k));
  if (off < 0 || count < 0 || (size_t)(off + count) * esz > b.bytes) die(std::string("launch would leave buffer ") + kv.at(k) + " (" + k + ")");
  return b.dev + GUARD + (size_t)off * esz;
}
static void sync_or_die(const char* what) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { fprintf(stderr, "driver: %s: %s\n", what, hipGetErrorString(e)); exit(4); }
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: encoder_kernels_driver <manifest>");
  std::ifstream mf(argv[1]);
  if (!mf) die("cannot read the manifest");
  std::string line;
  while (std::getline(mf, line)) {
    std::istringstream ls(line);
    std::string cmd, a, tok;
    if (!(ls >> cmd) || cmd[0] == '#') continue;
    ls >> a;
    if (cmd == "alloc") {
      size_t bytes; std::string file;
      ls >> bytes >> file;
      if (bufs.count(a) || bytes == 0 || bytes % 2) die("bad alloc " + a);
      Buf b;
      b.bytes = bytes;
      b.init.resize(bytes + 2 * GUARD);
      unsigned short* w = reinterpret_cast<unsigned short*>(b.init.data());
      for (size_t i = 0; i < b.init.size() / 2; ++i) w[i] = SENT16;
      if (file != "-") {
        FILE* f = fopen(file.c_str(), "rb");
        if (!f || fread(b.init.data() + GUARD, 1, bytes, f) != bytes || fgetc(f) != EOF) die("bad input file " + file);
        fclose(f);
      }
      CK(hipMalloc(&b.dev, b.init.size()));
      CK(hipMemcpy(b.dev, b.init.data(), b.init.size(), hipMemcpyHostToDevice));
      bufs[a] = std::move(b);
    } else if (cmd == "reset") {
      Buf& b = buf(a);
      CK(hipMemcpy(b.dev, b.init.data(), b.init.size(), hipMemcpyHostToDevice));
    } else if (cmd == "dump") {
      std::string file, base;
      ls >> file >> base;
      Buf& b = buf(a);
      std::vector<char> h(b.init.size());
      CK(hipMemcpy(h.data(), b.dev, h.size(), hipMemcpyDeviceToHost));
      if (!base.empty()) {
        std::vector<char> ref(h.size());
        FILE* fb = fopen(base.c_str(), "rb");
        const bool same = fb && fread(ref.data(), 1, ref.size(), fb) == ref.size() && memcmp(ref.data(), h.data(), h.size()) == 0;
        if (fb) fclose(fb);
        if (same) { printf("same %s\n", file.c_str()); continue; }
      }
      FILE* f = fopen(file.c_str(), "wb");
      if (!f || fwrite(h.data(), 1, h.size(), f) != h.size() || fclose(f) != 0) die("cannot write " + file);
    } else if (cmd == "free") {
      CK(hipFree(buf(a).dev));
      bufs.erase(a);
    } else if (cmd == "gemm" || cmd == "ln" || cmd == "attn") {
      KV kv;
      while (ls >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) die("bad token " + tok);
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
      }
      if (cmd == "gemm") {
        GemmParams p{};
        p.epilogue = (int)num(kv, "epi");
        p.M = (int)num(kv, "M"); p.N = (int)num(kv, "N"); p.K = (int)num(kv, "K"); p.batch = (int)num(kv, "batch");
        p.d_model = (int)num(kv, "d"); p.t_pad = (int)num(kv, "t_pad"); p.n_batch_total = (int)num(kv, "nbt");
        p.n_layer = (int)num(kv, "n_layer"); p.qkv_part = (int)num(kv, "qkv_part"); p.ksplit = (int)num(kv, "ksplit");
        p.lda = num(kv, "lda"); p.a_batch_stride = num(kv, "a_bs"); p.ldc = num(kv, "ldc"); p.c_batch_stride = num(kv, "c_bs");
        p.c2_batch_stride = num(kv, "c2_bs"); p.c3_batch_stride = num(kv, "c3_bs"); p.part_stride = num(kv, "part_stride");
        const long B = p.batch, M = p.M, N = p.N, K = p.K, d = p.d_model;
        if (B < 1 || M < 1 || N < 128 || N % 128 || K < 64 || K % 64 || p.lda < 1) die("bad gemm shape");
        p.A = (const h16*)ptr(kv, "A", 2, num(kv, "A_off"), (B - 1) * p.a_batch_stride + (M - 1) * p.lda + K);
        p.W = (const h16*)ptr(kv, "W", 2, 0, N * K);
        p.bias = (const float*)ptr(kv, "bias", 4, 0, N);
        if (!p.A || !p.W) die("gemm without A or W");
        const long rowmajor = (B - 1) * p.c_batch_stride + (M - 1) * p.ldc + N;
        switch (p.epilogue) {
          case EPI_BIAS_BF16: case EPI_BIAS_GELU_BF16: p.C = ptr(kv, "C", 2, num(kv, "C_off"), rowmajor); break;
          case EPI_RESID_F32: p.C = ptr(kv, "C", 4, num(kv, "C_off"), rowmajor); break;
          case EPI_GELU_POS_F32:
            p.C = ptr(kv, "C", 4, num(kv, "C_off"), rowmajor);
            p.aux = (const float*)ptr(kv, "aux", 4, 0, M * N);
            if (!p.aux) die("conv2 without positions");
            break;
          case EPI_QKV:
            if (N != 3 * d || M % 4 || p.t_pad % 16 || p.t_pad < (M + 15) / 16 * 16) die("bad qkv shape");
            p.C = ptr(kv, "C", 2, 0, (B - 1) * p.c_batch_stride + M * d);
            p.C2 = ptr(kv, "C2", 2, 0, (B - 1) * p.c2_batch_stride + M * d);
            p.C3 = ptr(kv, "C3", 2, 0, (B - 1) * p.c3_batch_stride + d * p.t_pad);
            if (!p.C2 || !p.C3) die("qkv without K or V^T");
            break;
          case EPI_CROSS_KV: {
            if (N != 2 * p.n_layer * d || d % 64 || p.t_pad % 64 || p.t_pad < M || p.n_batch_total < B) die("bad cross shape");
            const long all = (long)p.n_layer * p.n_batch_total * d * p.t_pad;
            p.C = ptr(kv, "C", 2, 0, all);
            p.C2 = ptr(kv, "C2", 2, 0, all);
            p.kv_slot_map = (const int*)ptr(kv, "slot_map", 4, 0, B);
            if (!p.C2) die("cross without V");
            if (p.kv_slot_map) {
              const int* hm = reinterpret_cast<const int*>(buf(kv.at("slot_map")).init.data() + GUARD);
              for (long b = 0; b < B; ++b) if (hm[b] < 0 || hm[b] >= p.n_batch_total) die("slot out of range");
            }
            break;
          }
          case EPI_PARTIAL_F32:
            if (p.ksplit < 1) die("bad ksplit");
            p.part = (float*)ptr(kv, "part", 4, 0, (p.ksplit - 1) * p.part_stride + B * M * N);
            if (!p.part) die("split-K without partials");
            break;
          default: die("unknown epilogue");
        }
        if (p.epilogue != EPI_PARTIAL_F32 && !p.C) die("gemm without C");
        gemm_force_tile = (int)num(kv, "force");
        gemm_last_kernel = gemm_prev_kernel = 0;
        launch_gemm(p, nullptr);
        sync_or_die(a.c_str());
        printf("ran %s %d %d\n", a.c_str(), gemm_prev_kernel, gemm_last_kernel);
      } else if (cmd == "ln") {
        const long rows = num(kv, "rows"), d = num(kv, "d"), n_part = num(kv, "n_part"), ps = num(kv, "part_stride");
        if (rows < 1 || d < 4 || d % 4 || d > 2048 || n_part < 0) die("bad layernorm shape");
        float* x = (float*)ptr(kv, "x", 4, 0, rows * d);
        const float* g = (const float*)ptr(kv, "g", 4, 0, d);
        const float* b = (const float*)ptr(kv, "b", 4, 0, d);
        h16* y = (h16*)ptr(kv, "y", 2, 0, rows * d);
        const float* part = n_part ? (const float*)ptr(kv, "part", 4, 0, (n_part - 1) * ps + rows * d) : nullptr;
        const float* pb = n_part ? (const float*)ptr(kv, "part_bias", 4, 0, d) : nullptr;
        if (!x || !g || !b || !y || (n_part && (!part || !pb))) die("layernorm without a buffer");
        launch_layernorm_bf16(x, g, b, y, rows, (int)d, nullptr, part, (int)n_part, ps, pb);
        sync_or_die(a.c_str());
        printf("ran %s 0 0\n", a.c_str());
      } else {
        const long B = num(kv, "batch"), T = num(kv, "T"), tp = num(kv, "t_pad"), d = num(kv, "d"), H = num(kv, "heads");
        if (B < 1 || T < 1 || tp % 64 || tp < T || tp - T >= 64 || d != H * 64) die("bad attention shape");
        const h16* q = (const h16*)ptr(kv, "q", 2, 0, B * T * d);
        const h16* k = (const h16*)ptr(kv, "k", 2, 0, B * T * d);
        const h16* vt = (const h16*)ptr(kv, "vt", 2, 0, B * d * tp);
        h16* o = (h16*)ptr(kv, "o", 2, 0, B * T * d);
        if (!q || !k || !vt || !o) die("attention without a buffer");
        launch_encoder_attention(q, k, vt, o, (int)B, (int)T, (int)tp, (int)d, (int)H, nullptr, (float)real(kv, "thr", 8.0));
        sync_or_die(a.c_str());
        printf("ran %s 0 0\n", a.c_str());
      }
      fflush(stdout);
    } else {
      die("unknown command " + cmd);
    }
  }
  printf("done\n");
  return 0;
}
