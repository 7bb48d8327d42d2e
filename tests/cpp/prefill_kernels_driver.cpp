// prefill_kernels_driver.cpp — the prompt-prefill kernels (csrc/decode_prefill.hip) on their own, for tests/test_gpu_prefill_kernels.py:
// one launch of one kernel on the caller's buffers through the engine's own launch functions. Built per dtype (-DAXW_F16) and
// linked against the shipped decode_prefill object.
//   prefill_kernels_driver <embed|store|attn> <in.bin> <out.bin>
//   in.bin: int32 head[8], then the arrays below in order; 16-bit arrays are raw h16 bits
//     embed  head = rows, d, n_vocab, n_pos           int32 ctx[rows], row_pos[rows]; h16 tok_emb[n_vocab][d]; f32 pos[n_pos][d]
//            out: f32 x[rows][d]
//     store  head = rows, d, n_ctx_pad, n_slots        int32 row_pos[rows], row_slot[rows]; h16 qkv[rows][3d]; h16 k[n_slots][H][n_ctx_pad*64], v[...]
//            out: h16 k, v (as they are after the launch)
//     attn   head = n_clips, n_head, keys_pad, n_keys, n_slots, ldq, rows, max_len
//            int32 row0[n_clips], len[n_clips], slot[n_clips]; h16 q[rows][ldq]; h16 k[n_slots][H][keys_pad*64], v[...]; h16 out0[rows][d]
//            out: h16 out[rows][d] (out0 overwritten where the kernel wrote)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

using namespace axw;

#define CHECK(X)                                                                                  \
  do {                                                                                            \
    const hipError_t e_ = (X);                                                                    \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #X, hipGetErrorString(e_)); return 2; } \
  } while (0)

static std::vector<char> g_in;
static size_t g_pos = 0;
// the next `bytes` of the input, on the device
static int take(size_t bytes, void** dev) {
  if (g_pos + bytes > g_in.size()) { fprintf(stderr, "input too short\n"); return 1; }
  if (hipMalloc(dev, bytes ? bytes : 16) != hipSuccess || hipMemcpy(*dev, g_in.data() + g_pos, bytes, hipMemcpyHostToDevice) != hipSuccess) return 2;
  g_pos += bytes;
  return 0;
}
#define TAKE(PTR, BYTES) do { void* p_ = nullptr; if (int rc_ = take((BYTES), &p_)) return rc_; PTR = static_cast<decltype(PTR)>(p_); } while (0)

static int write_out(const char* path, const std::vector<std::pair<const void*, size_t>>& parts) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 1; }
  for (const auto& p : parts) {
    std::vector<char> h(p.second);
    if (hipMemcpy(h.data(), p.first, p.second, hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); return 2; }
    if (fwrite(h.data(), 1, h.size(), f) != h.size()) { fclose(f); return 1; }
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s embed|store|attn in.bin out.bin\n", argv[0]); return 1; }
  const std::string mode = argv[1];
  {
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    fseek(f, 0, SEEK_END);
    g_in.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(g_in.data(), 1, g_in.size(), f) != g_in.size()) { fclose(f); return 1; }
    fclose(f);
  }
  if (g_in.size() < 32) { fprintf(stderr, "no header\n"); return 1; }
  int head[8];
  memcpy(head, g_in.data(), 32);
  g_pos = 32;
  hipStream_t s = nullptr;
  int rc = 1;
  if (mode == "embed") {
    const int rows = head[0], d = head[1], nv = head[2], np = head[3];
    if (rows < 1 || d < 1 || nv < 1 || np < 1) return 1;
    int *ctx, *row_pos; h16* emb; float *pos, *x;
    TAKE(ctx, (size_t)rows * 4); TAKE(row_pos, (size_t)rows * 4); TAKE(emb, (size_t)nv * d * 2); TAKE(pos, (size_t)np * d * 4);
    CHECK(hipMalloc(&x, (size_t)rows * d * 4));
    CHECK(hipMemset(x, 0xC5, (size_t)rows * d * 4));
    launch_prefill_embed(emb, pos, ctx, row_pos, x, rows, d, s);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    rc = write_out(argv[3], {{x, (size_t)rows * d * 4}});
  } else if (mode == "store") {
    const int rows = head[0], d = head[1], pad = head[2], slots = head[3];
    if (rows < 1 || d < 64 || d % 64 || pad < 64 || pad % 64 || slots < 1) return 1;
    const size_t cache = (size_t)slots * d * pad * 2;  // H * 64 = d
    PrefillStoreParams p{};
    int *row_pos, *row_slot; h16 *qkv, *k, *v;
    TAKE(row_pos, (size_t)rows * 4); TAKE(row_slot, (size_t)rows * 4); TAKE(qkv, (size_t)rows * 3 * d * 2); TAKE(k, cache); TAKE(v, cache);
    p.qkv = qkv; p.rows = rows; p.row_pos = row_pos; p.row_slot = row_slot; p.k_cache = k; p.v_cache = v;
    p.kv_slot_stride = (long)d * pad; p.d_model = d; p.n_ctx_pad = pad;
    launch_prefill_cache_store(p, s);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    rc = write_out(argv[3], {{k, cache}, {v, cache}});
  } else if (mode == "attn") {
    const int nc = head[0], H = head[1], pad = head[2], nk = head[3], slots = head[4], ldq = head[5], rows = head[6], max_len = head[7];
    if (nc < 1 || H < 1 || pad < 64 || pad % 64 || slots < 1 || ldq < H * 64 || rows < 1 || max_len < 1 || nk > pad) return 1;
    const size_t cache = (size_t)slots * H * 64 * pad * 2, outb = (size_t)rows * H * 64 * 2;
    PrefillAttnParams p{};
    int *row0, *len, *slot; h16 *q, *k, *v, *out;
    TAKE(row0, (size_t)nc * 4); TAKE(len, (size_t)nc * 4); TAKE(slot, (size_t)nc * 4); TAKE(q, (size_t)rows * ldq * 2); TAKE(k, cache); TAKE(v, cache);
    TAKE(out, outb);
    p.q = q; p.ldq = ldq; p.k = k; p.v = v; p.kv_slot_stride = (long)H * 64 * pad; p.keys_pad = pad; p.out = out; p.ldo = H * 64;
    p.row0 = row0; p.len = len; p.slot = slot; p.n_clips = nc; p.max_len = max_len; p.n_head = H; p.n_keys = nk;
    launch_prefill_attention(p, s);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    rc = write_out(argv[3], {{out, outb}});
  } else {
    fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 1;
  }
  if (rc == 0) printf("done\n");
  return rc;
}
