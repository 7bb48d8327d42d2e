// Runs the resample kernel that goes into libax_whisper.so one launcher call at a time, for tests/test_gpu_resample_kernel.py.
// Host-only code, built twice (-DAXW_F16=0 / 1) and linked against the objects `make` produced (build/resample.{bf16,f16}.o): the
// library has hidden visibility, and a recompilation would not be the shipped code.
//
//   resample_kernel_driver <manifest>       one command per line, executed in order:
//     alloc NAME BYTES FILE|-     device buffer with GUARD sentinel bytes before and after; content from FILE (raw), "-": sentinel
//     dump NAME FILE              the whole allocation, guards included
//     free NAME
//     resample ID key=value ...   one launch_resample
//   every launch prints "ran ID gx gy gz" with its grid.
// Every pointer of ResampleParams is the name of a buffer; the clip descriptors and over_off are read from the buffers' initial
// content, which the kernel does not write. Every launch is checked against the sizes of the buffers it names before it runs (status 2
// for what the launcher cannot take: the kernel itself trusts its parameters), and synchronised and checked for errors after.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "common.hpp"

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
static bool has(const KV& kv, const char* k) { auto it = kv.find(k); return it != kv.end() && it->second != "-"; }
// pointer to a named buffer, checked to hold `count` elements of `esz` bytes
static void* need(const KV& kv, const char* k, size_t esz, long count) {
  if (!has(kv, k)) die(std::string("launch without ") + k);
  Buf& b = buf(kv.at(k));
  if (count < 0 || (size_t)count * esz > b.bytes) die(std::string("launch would leave buffer ") + kv.at(k) + " (" + k + ")");
  return b.dev + GUARD;
}
static long elems(const KV& kv, const char* k, size_t esz) { return (long)(buf(kv.at(k)).bytes / esz); }
template <typename T> static const T* host(const KV& kv, const char* k) { return reinterpret_cast<const T*>(buf(kv.at(k)).init.data() + GUARD); }

int main(int argc, char** argv) {
  if (argc != 2) die("usage: resample_kernel_driver <manifest>");
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
    } else if (cmd == "dump") {
      std::string file;
      ls >> file;
      Buf& b = buf(a);
      std::vector<char> h(b.init.size());
      CK(hipMemcpy(h.data(), b.dev, h.size(), hipMemcpyDeviceToHost));
      FILE* f = fopen(file.c_str(), "wb");
      if (!f || fwrite(h.data(), 1, h.size(), f) != h.size() || fclose(f) != 0) die("cannot write " + file);
    } else if (cmd == "free") {
      CK(hipFree(buf(a).dev));
      bufs.erase(a);
    } else if (cmd == "resample") {
      KV kv;
      while (ls >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) die("bad token " + tok);
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
      }
      ResampleParams p{};
      p.batch = (int)num(kv, "batch");
      p.stride = (int)num(kv, "stride");
      p.max_out = (int)num(kv, "max_out");
      const long n_rows = num(kv, "n_rows");
      if (p.batch < 1 || p.stride < 0 || p.max_out < 1 || (p.stride > 0 && n_rows < 1)) die("bad resample shape");
      p.clips = (const ResampleClip*)need(kv, "clips", sizeof(ResampleClip), p.batch);
      const ResampleClip* c = host<ResampleClip>(kv, "clips");
      const long n_in = elems(kv, "in", 4), n_tab = elems(kv, "tables", 4), n_outbuf = elems(kv, "out", 4);
      const long n_over = has(kv, "overflow") ? elems(kv, "overflow", 4) : 0;
      const long long* oo = has(kv, "over_off") ? host<long long>(kv, "over_off") : nullptr;
      if (oo && elems(kv, "over_off", 8) < n_rows) die("over_off below the row count");
      if (p.stride > 0 && n_rows * p.stride > n_outbuf) die("rows beyond the output buffer");
      for (int b = 0; b < p.batch; ++b) {
        const ResampleClip& k = c[b];
        if (k.n_in < 1 || !resample_shape_ok(k.L, k.M, k.K)) die("a clip the kernel cannot take");
        if (k.n_out != (int)(((long)k.n_in * k.L + k.M - 1) / k.M) || k.n_out > p.max_out) die("n_out is not ceil(n_in L / M) or beyond max_out");
        if (k.in_off < 0 || k.in_off + k.n_in > n_in) die("a clip beyond the input buffer");
        if (k.tab_off < 0 || k.tab_off + (long)k.L * 2 * k.K > n_tab) die("a table that does not hold L * 2 K entries");
        if (p.stride == 0) {
          if (k.out_off < 0 || k.out_off + k.n_out > n_outbuf) die("an output beyond its capacity");
        } else {
          if (k.row < 0 || k.row >= n_rows) die("a row outside the staging rows");
          if (k.n_out > p.stride) {
            if (!n_over || !oo) die("an output beyond its staging row without an overflow buffer");
            if (oo[k.row] < 0 || oo[k.row] + k.n_out - p.stride > n_over) die("a tail beyond the overflow buffer");
          }
        }
      }
      p.in = (const float*)need(kv, "in", 4, 1);
      p.tables = (const float*)need(kv, "tables", 4, 1);
      p.out = (float*)need(kv, "out", 4, 1);
      if (has(kv, "overflow")) {
        p.overflow = (float*)need(kv, "overflow", 4, 1);
        p.over_off = (const long long*)need(kv, "over_off", 8, n_rows);
      }
      launch_resample(p, nullptr);
      hipError_t e = hipDeviceSynchronize();
      if (e == hipSuccess) e = hipGetLastError();
      if (e != hipSuccess) { fprintf(stderr, "driver: %s: %s\n", a.c_str(), hipGetErrorString(e)); exit(4); }
      printf("ran %s %d %d 1\n", a.c_str(), (p.max_out + kResampleTile - 1) / kResampleTile, p.batch);
      fflush(stdout);
    } else {
      die("unknown command " + cmd);
    }
  }
  printf("done\n");
  return 0;
}
