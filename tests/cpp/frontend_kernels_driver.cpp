// Runs the log-mel front-end kernels that go into libax_whisper.so one launcher call at a time, for
// tests/test_gpu_frontend_kernels.py. Host-only code, built twice (-DAXW_F16=0 / 1) and linked against the objects `make`
// produced (build/frontend.{bf16,f16}.o): the library has hidden visibility, and a recompilation would not be the shipped code.
//
//   frontend_kernels_driver <manifest>       one command per line, executed in order:
//     alloc NAME BYTES FILE|-     device buffer with GUARD sentinel bytes before and after; content from FILE (raw), "-": sentinel
//     dump NAME FILE              the whole allocation, guards included
//     free NAME
//     frontend ID key=value ...       one launch_frontend (gmax_reset_kernel, stft_mel_kernel, mel_normalize_kernel)
//     frontend_long ID key=value ...  one launch_frontend_long (gmax_reset_kernel, stft_mel_long_kernel)
//     mel_window ID key=value ...     one launch_mel_window
//     mel_to_tm ID key=value ...      one launch_mel_to_tm
//   every launch prints "ran ID gx gy gz" with the grid of its widest kernel.
// Every pointer of FrontendParams, LongStoreParams and MelWindowParams is the name of a buffer (or "-" / absent: nullptr where the
// kernels take one); the integer arrays are read from the buffers' initial content, which no kernel writes. Every launch is
// checked against the sizes of the buffers it names before it runs (status 2 for what a launcher cannot take), and synchronised
// and checked for errors after.
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
constexpr int kMelRows = 3004;  // rows of an encoder slot, as the engine allocates them

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
// pointer to a named buffer, checked to hold `count` elements of `esz` bytes; nullptr where the key is absent
static void* ptr(const KV& kv, const char* k, size_t esz, long count) {
  if (!has(kv, k)) return nullptr;
  Buf& b = buf(kv.at(k));
  if (count < 0 || (size_t)count * esz > b.bytes) die(std::string("launch would leave buffer ") + kv.at(k) + " (" + k + ")");
  return b.dev + GUARD;
}
static void* need(const KV& kv, const char* k, size_t esz, long count) {
  void* p = ptr(kv, k, esz, count);
  if (!p) die(std::string("launch without ") + k);
  return p;
}
// the initial content of an integer buffer (no kernel writes one)
template <typename T> static const T* host(const KV& kv, const char* k) { return reinterpret_cast<const T*>(buf(kv.at(k)).init.data() + GUARD); }
static void sync_or_die(const char* what) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { fprintf(stderr, "driver: %s: %s\n", what, hipGetErrorString(e)); exit(4); }
}

// the fields the clip and the file kernel share
static void constants(const KV& kv, FrontendParams& p) {
  p.batch = (int)num(kv, "batch");
  p.n_mels = (int)num(kv, "n_mels");
  p.max_frames = (int)num(kv, "max_frames");
  if (p.batch < 1 || p.n_mels < 8 || p.n_mels % 8 || p.n_mels > 128 || p.max_frames < 1) die("bad front-end shape");
  p.twiddle = (const float*)need(kv, "twiddle", 4, 2 * kNFFT);
  p.window = (const float*)need(kv, "window", 4, kNFFT);
  p.mel_basis = (const float*)need(kv, "basis", 4, (long)kBins * p.n_mels);
  p.n_samples = (const int*)need(kv, "n_samples", 4, p.batch);
  p.gmax = (unsigned*)need(kv, "gmax", 4, p.batch);
  const int* n = host<int>(kv, "n_samples");
  for (int b = 0; b < p.batch; ++b)
    if (n[b] < 1) die("clip without samples");
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: frontend_kernels_driver <manifest>");
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
    } else if (cmd == "frontend" || cmd == "frontend_long" || cmd == "mel_window" || cmd == "mel_to_tm") {
      KV kv;
      while (ls >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) die("bad token " + tok);
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
      }
      long gx = 0, gy = 0;
      if (cmd == "frontend") {
        FrontendParams p{};
        constants(kv, p);
        const long B = p.batch, nm = p.n_mels;
        p.stride = (int)num(kv, "stride");
        p.openai = (int)num(kv, "openai");
        p.mel_rows = kMelRows;
        if (p.stride < 1 || (p.openai != 0 && p.openai != 1)) die("bad stride or mode");
        p.pcm = (const float*)need(kv, "pcm", 4, B * p.stride);
        p.power = (float*)ptr(kv, "power", 4, 1);  // read by no kernel
        p.logmel = (float*)need(kv, "logmel", 4, B * kFramesOut * nm);
        p.mel_ref = (float*)ptr(kv, "mel_ref", 4, B * nm * kFramesOut);
        p.mel_tm = (h16*)ptr(kv, "mel_tm", 2, B * kMelRows * nm);
        const int* n = host<int>(kv, "n_samples");
        long over = 0;
        for (long b = 0; b < B; ++b) over = std::max(over, (long)n[b] - p.stride);
        if (over > 0) {  // a clip beyond its staging row: its tail must lie inside the overflow buffer
          if (!has(kv, "overflow") || !has(kv, "over_off")) die("a clip beyond the staging row without overflow / over_off");
          p.over_off = (const long long*)need(kv, "over_off", 8, B);
          const long long* oo = host<long long>(kv, "over_off");
          long end = 0;
          for (long b = 0; b < B; ++b) {
            if (n[b] <= p.stride) continue;
            if (oo[b] < 0) die("negative over_off");
            end = std::max(end, (long)oo[b] + n[b] - p.stride);
          }
          p.overflow = (const float*)need(kv, "overflow", 4, end);
        } else {
          p.overflow = (const float*)ptr(kv, "overflow", 4, 1);
          p.over_off = (const long long*)ptr(kv, "over_off", 8, B);
        }
        launch_frontend(p, nullptr);
        gx = (p.max_frames + 31) / 32; gy = B;
      } else if (cmd == "frontend_long") {
        FrontendParams p{};
        LongStoreParams lp{};
        constants(kv, p);
        const long B = p.batch, nm = p.n_mels;
        lp.pcm_off = (const long long*)need(kv, "pcm_off", 8, B);
        lp.frame_off = (const long long*)need(kv, "frame_off", 8, B);
        const int* n = host<int>(kv, "n_samples");
        const long long* po = host<long long>(kv, "pcm_off");
        const long long* fo = host<long long>(kv, "frame_off");
        long pcm_end = 0, row_end = 0;
        for (long b = 0; b < B; ++b) {
          if (po[b] < 0 || fo[b] < 0) die("negative offset");
          pcm_end = std::max(pcm_end, (long)po[b] + n[b]);
          row_end = std::max(row_end, (long)fo[b] + 1 + n[b] / kHop);
        }
        p.pcm = (const float*)need(kv, "pcm", 4, pcm_end);
        lp.store = (float*)need(kv, "store", 4, row_end * nm);
        launch_frontend_long(p, lp, nullptr);
        gx = (p.max_frames + 31) / 32; gy = B;
      } else if (cmd == "mel_window") {
        MelWindowParams p{};
        p.n_mels = (int)num(kv, "n_mels");
        p.n_windows = (int)num(kv, "n_windows");
        p.mel_rows = kMelRows;
        const long nf = num(kv, "n_files"), nm = p.n_mels, W = p.n_windows;
        if (nm < 8 || nm % 8 || nm > 128 || W < 1 || nf < 1) die("bad window shape");
        p.frame_off = (const long long*)need(kv, "frame_off", 8, nf);
        p.n_frames = (const int*)need(kv, "n_frames", 4, nf);
        p.gmax = (const unsigned*)need(kv, "gmax", 4, nf);
        p.win_file = (const int*)need(kv, "win_file", 4, W);
        p.win_seek = (const int*)need(kv, "win_seek", 4, W);
        const long long* fo = host<long long>(kv, "frame_off");
        const int* fr = host<int>(kv, "n_frames");
        const int* wf = host<int>(kv, "win_file");
        const int* ws = host<int>(kv, "win_seek");
        long row_end = 0;
        for (long f = 0; f < nf; ++f) {
          if (fo[f] < 0 || fr[f] < 0) die("negative offset or row count");
          row_end = std::max(row_end, (long)fo[f] + fr[f]);
        }
        for (long w = 0; w < W; ++w)
          if (wf[w] < 0 || wf[w] >= nf || ws[w] < 0 || ws[w] > (1 << 30)) die("window outside the files");
        p.store = (const float*)need(kv, "store", 4, row_end * nm);
        p.mel_tm = (h16*)ptr(kv, "mel_tm", 2, W * kMelRows * nm);
        p.mel_ref = (float*)ptr(kv, "mel_ref", 4, W * nm * kFramesOut);
        if (!p.mel_tm && !p.mel_ref) die("window without an output");
        launch_mel_window(p, nullptr);
        gx = (kFramesOut + 63) / 64; gy = W;
      } else {
        const long B = num(kv, "batch"), nm = num(kv, "n_mels");
        if (B < 1 || nm < 1) die("bad mel_to_tm shape");
        const float* mel_ref = (const float*)need(kv, "mel_ref", 4, B * nm * kFramesOut);
        h16* mel_tm = (h16*)need(kv, "mel_tm", 2, B * kMelRows * nm);
        launch_mel_to_tm(mel_ref, mel_tm, (int)B, (int)nm, kMelRows, nullptr);
        gx = 64; gy = B;
      }
      sync_or_die(a.c_str());
      printf("ran %s %ld %ld 1\n", a.c_str(), gx, gy);
      fflush(stdout);
    } else {
      die("unknown command " + cmd);
    }
  }
  printf("done\n");
  return 0;
}
