// Runs the kernel of csrc/decode_attention_group_fp8.hip one launch at a time, for tests/test_gpu_cross_group_fp8_kernel.py, with the
// manifest, buffers, guards and size checks of cross_group_driver.cpp: that file is included inside a namespace, behind the headers it
// needs, so that only its own text lands there (its main stays unused). An attng line is one launch_decode_cross_attention_group_fp8.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "common.hpp"
namespace h16_driver {
#include "cross_group_driver.cpp"
}
using namespace h16_driver;
int main(int argc, char** argv) {
  std::ifstream mf(argc == 2 ? argv[1] : "");
  if (!mf) die("usage: cross_group_fp8_driver <manifest>");
  std::string line, cmd, a, file, tok;
  while (std::getline(mf, line)) {
    std::istringstream ls(line);
    if (!(ls >> cmd >> a)) continue;
    if (cmd == "alloc") {
      Buf b;
      ls >> b.bytes >> file;
      std::ifstream f(file, std::ios::binary);
      b.init.assign(b.bytes + 2 * GUARD, 0);
      for (size_t i = 0; i < b.init.size() / 2; ++i) reinterpret_cast<unsigned short*>(b.init.data())[i] = SENT16;
      if (bufs.count(a) || b.bytes == 0 || b.bytes % 2 || !f.read(b.init.data() + GUARD, b.bytes) || f.get() != EOF) die("bad alloc " + a);
      CK(hipMalloc(&b.dev, b.init.size()));
      CK(hipMemcpy(b.dev, b.init.data(), b.init.size(), hipMemcpyHostToDevice));
      bufs[a] = std::move(b);
    } else if (cmd == "dump") {
      ls >> file;
      std::vector<char> h(buf(a).init.size());
      CK(hipMemcpy(h.data(), buf(a).dev, h.size(), hipMemcpyDeviceToHost));
      if (!std::ofstream(file, std::ios::binary).write(h.data(), h.size())) die("cannot write " + file);
    } else if (cmd == "attng") {
      KV kv;
      while (ls >> tok) kv[tok.substr(0, tok.find('='))] = tok.substr(tok.find('=') + 1);
      DecAttnGroupFp8Params p{};
      p.group = (int)num(kv, "group"); p.slot0 = (int)num(kv, "slot0"); p.nslots = (int)num(kv, "nslots"); p.n_head = (int)num(kv, "n_head");
      p.d_model = (int)num(kv, "d_model"); p.n_keys = (int)num(kv, "n_keys"); p.cap_blocks = (int)num(kv, "cap_blocks"); p.n_split = (int)num(kv, "n_split", 1);
      p.nbs = (int)num(kv, "nbs"); p.done_late = (int)num(kv, "done_late");
      const long S = num(kv, "n_slots"), KS = num(kv, "kv_slots"), H = p.n_head, d = p.d_model, cap = p.cap_blocks, ns = p.n_split, s0 = p.slot0;
      p.kv_slot_bytes = H * layout::kv8_head_bytes((int)cap * layout::kKvBlockKeys);
      p.scale_slot_stride = H * layout::kKv8ScaleHead;
      if (p.group < 1 || p.group > 8 || s0 < 0 || s0 % 16 || p.nslots < 1 || s0 + p.nslots > S || (s0 + p.nslots - 1) / p.group >= KS || H < 1 || d != H * 64 ||
          d > 1024 || cap < 1 || ns < 1 || ns > layout::kAttnSplitMax || p.n_keys < 1 || p.n_keys > cap * 64 || p.nbs < (S + 15) / 16) die("bad attention shape");
      const long pair = layout::pair_elems((int)d / 32, p.nbs), blk0 = layout::clip_block_offset((int)s0);
      p.k8 = at<const unsigned char>(kv, "k8", KS * p.kv_slot_bytes); p.v8 = at<const unsigned char>(kv, "v8", KS * p.kv_slot_bytes);
      p.scales = at<const float>(kv, "scales", KS * p.scale_slot_stride);
      p.out_hi = at<h16>(kv, "out_hi", pair, blk0); p.out_lo = at<h16>(kv, "out_lo", pair, blk0);
      p.done = at<const int>(kv, "done", S, s0);
      if (ns > 1) {
        p.mpart = at<float>(kv, "mpart", layout::part_elems(S, (int)H, (int)ns), layout::part_elems(s0, (int)H, (int)ns));
        p.mcnt = at<unsigned>(kv, "mcnt", S * H, s0 * H);
      }
      if (has(kv, "tq")) {
        p.tq = at<const float>(kv, "tq", S * d, s0 * d); p.stat_part = at<const float>(kv, "stat_part", S * (d / 16) * 2, s0 * (d / 16) * 2);
        p.fold_s = at<const float>(kv, "fold_s", d); p.fold_c = at<const float>(kv, "fold_c", d);
      } else if (has(kv, "wq")) {
        p.x = at<const float>(kv, "x", S * d, s0 * d); p.wq = at<const h16>(kv, "wq", d * d);
        p.ln_w = at<const float>(kv, "ln_w", d); p.ln_b = at<const float>(kv, "ln_b", d); p.bq = at<const float>(kv, "bq", d);
      } else {
        p.q = at<const float>(kv, "q", S * d, s0 * d);
      }
      launch_decode_cross_attention_group_fp8(p, nullptr);
      hipError_t e = hipDeviceSynchronize();
      if (e == hipSuccess) e = hipGetLastError();
      if (e != hipSuccess) { fprintf(stderr, "driver: %s: %s\n", a.c_str(), hipGetErrorString(e)); exit(4); }
      printf("ran %s %ld %ld %d\n", a.c_str(), ns, H, cross_group_clips(p.slot0, p.nslots, p.group));
      fflush(stdout);
    } else {
      die("unknown command " + cmd);
    }
  }
  printf("done\n");
  return 0;
}
