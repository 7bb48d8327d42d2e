// Runs the two kernels of csrc/cross_kv_fp8.hip one launch at a time, for tests/test_gpu_cross_fp8_kernels.py.
// Host-only code, built twice (-DAXW_F16=0 / 1) and linked against the object `make` produced (build/cross_kv_fp8.{bf16,f16}.o): the
// library has hidden visibility, and a recompilation would not be the shipped code.
//
//   cross_fp8_driver <manifest>             one command per line, executed in order (the manifest language of decode_kernels_driver.cpp):
//     alloc NAME BYTES FILE|-     device buffer with GUARD sentinel bytes before and after; content from FILE (raw), "-": sentinel
//     reset NAME                  initial content again (guards included)
//     dump NAME FILE              the whole allocation, guards included
//     free NAME
//     quant ID key=value ...      one launch_cross_kv_quantize (CrossKvQuantParams)
//     attn8 ID key=value ...      one launch_decode_cross_attention_fp8 (DecAttnFp8Params)
//   every launch prints "ran ID gx gy gz" with the grid it started.
// Keys carry the names of the parameter structs' fields; a pointer field names a buffer. Every launch is checked against the sizes of
// the buffers it names (and the slots a slot map would send a clip to) before it runs, and synchronised and checked for errors after.
// Parameters a launcher's own checks would abort() on are refused here, with exit status 2.
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
static void* need(const KV& kv, const char* k, size_t esz, long count) {
  if (!has(kv, k)) die(std::string("launch without ") + k);
  Buf& b = buf(kv.at(k));
  if (count < 0 || (size_t)count * esz > b.bytes) die(std::string("launch would leave buffer ") + kv.at(k) + " (" + k + ")");
  return b.dev + GUARD;
}
static const int* host_ints(const KV& kv, const char* k) { return reinterpret_cast<const int*>(buf(kv.at(k)).init.data() + GUARD); }

int main(int argc, char** argv) {
  if (argc != 2) die("usage: cross_fp8_driver <manifest>");
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
    } else if (cmd == "quant" || cmd == "attn8") {
      KV kv;
      while (ls >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) die("bad token " + tok);
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
      }
      long gx = 1, gy = 1, gz = 1;
      if (cmd == "quant") {
        CrossKvQuantParams p{};
        p.n_layer = (int)num(kv, "n_layer"); p.n_slots = (int)num(kv, "n_slots"); p.n_head = (int)num(kv, "n_head"); p.clips = (int)num(kv, "clips");
        p.n_keys = (int)num(kv, "n_keys"); p.keys_pad = (int)num(kv, "keys_pad");
        const long L = p.n_layer, S = p.n_slots, H = p.n_head;
        if (L < 1 || S < 1 || H < 1 || p.clips < 1 || p.clips > S || p.keys_pad < 64 || p.keys_pad % 64 || p.n_keys < 0 || p.n_keys > p.keys_pad) die("bad quantise shape");
        const long heads = L * S * H;
        p.k = (const h16*)need(kv, "k", 2, heads * layout::kv_head_elems(p.keys_pad));
        p.v = (const h16*)need(kv, "v", 2, heads * layout::kv_head_elems(p.keys_pad));
        p.k8 = (unsigned char*)need(kv, "k8", 1, heads * layout::kv8_head_bytes(p.keys_pad));
        p.v8 = (unsigned char*)need(kv, "v8", 1, heads * layout::kv8_head_bytes(p.keys_pad));
        p.scales = (float*)need(kv, "scales", 4, layout::kv8_scale_elems(p.n_layer, p.n_slots, p.n_head));
        if (has(kv, "slot_map")) {
          p.slot_map = (const int*)need(kv, "slot_map", 4, p.clips);
          const int* hm = host_ints(kv, "slot_map");
          for (int b = 0; b < p.clips; ++b) if (hm[b] < 0 || hm[b] >= S) die("slot map entry outside the slots");
        }
        gx = 2 * H; gy = p.clips; gz = L;
        launch_cross_kv_quantize(p, nullptr);
      } else {
        DecAttnFp8Params p{};
        p.batch = (int)num(kv, "batch"); p.n_head = (int)num(kv, "n_head"); p.d_model = (int)num(kv, "d_model"); p.n_keys = (int)num(kv, "n_keys");
        p.cap_blocks = (int)num(kv, "cap_blocks"); p.n_split = (int)num(kv, "n_split", 1); p.kv_batch_bytes = num(kv, "kv_batch_bytes");
        p.scale_batch_stride = num(kv, "scale_batch_stride"); p.nbs = (int)num(kv, "nbs"); p.done_late = (int)num(kv, "done_late");
        const long B = p.batch, H = p.n_head, d = p.d_model, cap = p.cap_blocks, ns = p.n_split;
        const long head_bytes = layout::kv8_head_bytes((int)cap * layout::kKvBlockKeys);
        if (B < 1 || H < 1 || d != H * 64 || cap < 1 || ns < 1 || ns > cap || ns > layout::kAttnSplitMax || p.kv_batch_bytes < H * head_bytes ||
            p.scale_batch_stride < H * layout::kKv8ScaleHead || p.n_keys < 1 || p.n_keys > cap * 64 || p.nbs < (B + 15) / 16) die("bad attention shape");
        p.k8 = (const unsigned char*)need(kv, "k8", 1, (B - 1) * p.kv_batch_bytes + H * head_bytes);
        p.v8 = (const unsigned char*)need(kv, "v8", 1, (B - 1) * p.kv_batch_bytes + H * head_bytes);
        p.scales = (const float*)need(kv, "scales", 4, (B - 1) * p.scale_batch_stride + H * layout::kKv8ScaleHead);
        p.done = (const int*)need(kv, "done", 4, B);
        p.out_hi = (h16*)need(kv, "out_hi", 2, layout::pair_elems(d / 32, p.nbs));
        p.out_lo = (h16*)need(kv, "out_lo", 2, layout::pair_elems(d / 32, p.nbs));
        if (ns > 1) {
          p.mpart = (float*)need(kv, "mpart", 4, layout::part_elems(B, H, ns));
          p.mcnt = (unsigned*)need(kv, "mcnt", 4, B * H);
        }
        if (has(kv, "tq")) {
          if (d > 1024) die("folded query: unsupported launch");
          p.tq = (const float*)need(kv, "tq", 4, B * d);
          p.stat_part = (const float*)need(kv, "stat_part", 4, B * (d / 16) * 2);
          p.fold_s = (const float*)need(kv, "fold_s", 4, d);
          p.fold_c = (const float*)need(kv, "fold_c", 4, d);
        } else if (has(kv, "wq")) {
          if (d > 1024) die("fused query projection: unsupported launch");
          p.x = (const float*)need(kv, "x", 4, B * d);
          p.ln_w = (const float*)need(kv, "ln_w", 4, d);
          p.ln_b = (const float*)need(kv, "ln_b", 4, d);
          p.wq = (const h16*)need(kv, "wq", 2, d * d);
          p.bq = (const float*)need(kv, "bq", 4, d);
        } else {
          p.q = (const float*)need(kv, "q", 4, B * d);
        }
        gx = ns; gy = H; gz = B;
        launch_decode_cross_attention_fp8(p, nullptr);
      }
      hipError_t e = hipDeviceSynchronize();
      if (e == hipSuccess) e = hipGetLastError();
      if (e != hipSuccess) { fprintf(stderr, "driver: %s: %s\n", a.c_str(), hipGetErrorString(e)); exit(4); }
      printf("ran %s %ld %ld %ld\n", a.c_str(), gx, gy, gz);
      fflush(stdout);
    } else {
      die("unknown command " + cmd);
    }
  }
  printf("done\n");
  return 0;
}
