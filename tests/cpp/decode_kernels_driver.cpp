// Runs the decoder step's kernels that go into libax_whisper.so one launch at a time, for tests/test_gpu_decode_kernels.py (the
// batched step) and tests/test_gpu_gemv_kernels.py (the GEMV family, advance, embed).
// Host-only code, built twice (-DAXW_F16=0 / 1) and linked against the objects `make` produced (build/decode_gemm.{bf16,f16}.o,
// build/decoder.{bf16,f16}.o, build/decode_gemv.{bf16,f16}.o): the library has hidden visibility, and a recompilation would not be
// the shipped code.
//
//   decode_kernels_driver <manifest>        one command per line, executed in order (the manifest language of
//                                           encoder_kernels_driver.cpp):
//     alloc NAME BYTES FILE|-     device buffer with GUARD sentinel bytes before and after; content from FILE (raw), "-": sentinel
//     reset NAME                  initial content again (guards included)
//     dump NAME FILE [BASE]       the whole allocation, guards included; with BASE: nothing is written (and "same FILE" printed)
//                                 when the content equals that of the earlier dump BASE bit for bit
//     free NAME
//     cgemm ID key=value ...      one launch_decode_cgemm (DecCGemmParams)
//     dgemm ID key=value ...      one launch_decode_gemm (DecGemmParams), rt=0 included
//     actprep ID key=value ...    one launch_act_prep
//     attn ID key=value ...       one launch_decode_attention (DecAttnParams)
//     packw ID key=value ...      one launch_pack_weight_frag
//     packw_split ID key=value .. one launch_pack_weight_frag_split
//     gemv ID key=value ...       one launch_gemv (GemvParams; `state` is not read by the kernels and stays null)
//     advance ID key=value ...    one launch_advance (AdvanceParams; done_host may be an ordinary device buffer)
//     embed ID key=value ...      one launch_embed (tok_emb, pos, tok, off, x, batch, d; n_vocab and n_ctx size the tables)
//   every launch prints "ran ID gx gy gz" with the grid it started.
// Keys carry the names of the parameter structs' fields; a pointer field names a buffer. Every launch is checked against the sizes of
// the buffers it names (and the clip offsets a kernel would index a cache with) before it runs, and synchronised and checked for
// errors after. Parameters a launcher's own checks would abort() on are refused here, with exit status 2.
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
// pointer to the start of a named buffer, checked to hold `count` elements of `esz` bytes; nullptr where the key is absent
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
// the initial host content of an int buffer (clip offsets, done flags): what the kernel will index with
static const int* host_ints(const KV& kv, const char* k) { return reinterpret_cast<const int*>(buf(kv.at(k)).init.data() + GUARD); }
static void sync_or_die(const char* what) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { fprintf(stderr, "driver: %s: %s\n", what, hipGetErrorString(e)); exit(4); }
}

// the self-attention cache of one layer as GEPI_QKV_CACHE addresses it: [clip, stride kv_bs][head][n_ctx_pad rows][64]
static void check_cache(const KV& kv, long batch, long d, long n_ctx_pad, long kv_bs, h16*& kc, h16*& vc, const int*& off) {
  if (d < 64 || d % 64 || n_ctx_pad < 64 || n_ctx_pad % 64 || kv_bs < d * n_ctx_pad) die("bad cache shape");
  kc = (h16*)need(kv, "k_cache", 2, (batch - 1) * kv_bs + d * n_ctx_pad);
  vc = (h16*)need(kv, "v_cache", 2, (batch - 1) * kv_bs + d * n_ctx_pad);
  off = (const int*)need(kv, "off", 4, batch);
  const int* ho = host_ints(kv, "off");
  for (long b = 0; b < batch; ++b) if (ho[b] < 0 || ho[b] >= n_ctx_pad) die("clip offset outside the cache");
}

// launch_gemv's choice of lanes per weight row (decode_gemv.hip pick_lpr), to know the instantiation a launch would ask for
static int gemv_lpr(long K) {
  if (K % 512 == 0 && K / 512 <= 10 && K >= 1024) return 64;
  if (K % 256 == 0 && K / 256 <= 6) return 32;
  if (K % 128 == 0 && K / 128 <= 10) return 16;
  return 0;
}

static long run_gemv(const KV& kv) {
  GemvParams p{};
  p.N = (int)num(kv, "N"); p.K = (int)num(kv, "K"); p.batch = (int)num(kv, "batch"); p.prologue = (int)num(kv, "prologue"); p.epilogue = (int)num(kv, "epilogue");
  p.n_split = (int)num(kv, "n_split"); p.n_head = (int)num(kv, "n_head"); p.d_model = (int)num(kv, "d_model"); p.n_ctx_pad = (int)num(kv, "n_ctx_pad");
  p.kv_batch_stride = num(kv, "kv_batch_stride"); p.amax_stride = (int)num(kv, "amax_stride"); p.logits_dump_stride = num(kv, "logits_dump_stride");
  p.skip_before_step = (int)num(kv, "skip_before_step");
  const long N = p.N, K = p.K, B = p.batch, d = p.d_model;
  if (N < 1 || K < 128 || B < 1) die("bad gemv shape");
  if (B > 4) die("gemv: at most 4 clips per launch");
  const int lpr = gemv_lpr(K);
  const long ch = lpr ? K / (8 * lpr) : 0;
  if (!lpr || !(ch == 1 || ch == 2 || ch == 3 || ch == 4 || ch == 5 || ch == 6 || ch == 8 || ch == 10)) die("gemv: no instantiation for this K");
  const long grid = gemv_grid(p);
  if (grid < 1) die("gemv: no grid");
  p.W = (const h16*)need(kv, "W", 2, N * K);
  p.bias = (const float*)ptr(kv, "bias", 4, N);
  switch (p.prologue) {
    case PRO_PLAIN: p.in = (const float*)need(kv, "in", 4, B * K); break;
    case PRO_LAYERNORM:
      if (B > 1 && K > 2048) die("LayerNorm prologue of gemv_kernel: K > 2048");
      p.in = (const float*)need(kv, "in", 4, B * K);
      p.ln_w = (const float*)need(kv, "ln_w", 4, K);
      p.ln_b = (const float*)need(kv, "ln_b", 4, K);
      break;
    case PRO_ATTN_COMBINE:
      if (p.n_head < 1 || K != (long)p.n_head * 64) die("attention combine: K is 64 n_head");
      if (p.n_split < 1) die("attention combine: n_split < 1");
      if (p.n_split > 8) die("attention combine: n_split > 8");
      p.part = (const float*)need(kv, "part", 4, layout::part_elems(B, p.n_head, p.n_split));
      break;
    default: die("unknown gemv prologue");
  }
  switch (p.epilogue) {
    case GEPI_STORE: case GEPI_GELU: case GEPI_RESID: p.out = (float*)need(kv, "out", 4, B * N); break;
    case GEPI_QKV_CACHE:
      if (N != 3 * d) die("QKV_CACHE: N is 3 d_model");
      p.out = (float*)need(kv, "out", 4, B * d);
      check_cache(kv, B, d, p.n_ctx_pad, p.kv_batch_stride, p.k_cache, p.v_cache, p.off);
      break;
    case GEPI_LOGITS:
      if (p.amax_stride < grid) die("amax_stride below the grid");
      p.off = (const int*)need(kv, "off", 4, B);
      p.amax_val = (float*)need(kv, "amax_val", 4, (B - 1) * p.amax_stride + grid);
      p.amax_idx = (int*)need(kv, "amax_idx", 4, (B - 1) * p.amax_stride + grid);
      if (has(kv, "logits_dump")) {
        if (p.logits_dump_stride < N) die("logits_dump_stride below N");
        p.logits_dump = (float*)need(kv, "logits_dump", 4, (B - 1) * p.logits_dump_stride + N);
      }
      break;
    default: die("unknown gemv epilogue");
  }
  launch_gemv(p, nullptr);
  return grid;
}

static void ids_below(const KV& kv, const char* k, long count, long limit, const char* what) {
  const int* h = host_ints(kv, k);
  for (long i = 0; i < count; ++i) if (h[i] < 0 || h[i] >= limit) die(std::string(what) + " outside its table (" + k + ")");
}

static long run_advance(const KV& kv) {
  AdvanceParams p{};
  p.n_part = (int)num(kv, "n_part"); p.amax_stride = (int)num(kv, "amax_stride"); p.batch = (int)num(kv, "batch"); p.n_ctx = (int)num(kv, "n_ctx");
  p.eot = (int)num(kv, "eot"); p.max_new = (int)num(kv, "max_new"); p.n_vocab = (int)num(kv, "n_vocab"); p.n_forced = (int)num(kv, "n_forced");
  p.d_model = (int)num(kv, "d_model"); p.n_prefix = (int)num(kv, "n_prefix");
  const long B = p.batch, d = p.d_model, V = p.n_vocab, T = p.n_ctx;
  if (B < 1 || T < 1 || V < 1 || p.n_part < 0 || p.n_prefix < 0 || p.n_forced < 0) die("bad advance shape");
  if (d < 4 || d > 2048 || d % 4) die("advance: d_model above 2048 or no multiple of 4");
  if (p.n_part > p.amax_stride) die("advance: n_part above amax_stride");
  const long n_pre = p.n_prefix > 0 ? p.n_prefix : 4;
  p.amax_val = (const float*)need(kv, "amax_val", 4, (B - 1) * p.amax_stride + p.n_part);
  p.amax_idx = (const int*)need(kv, "amax_idx", 4, (B - 1) * p.amax_stride + p.n_part);
  p.state = (DecState*)need(kv, "state", sizeof(DecState), 1);
  p.off = (int*)need(kv, "off", 4, B);
  p.tok = (int*)need(kv, "tok", 4, B);
  p.sot = (const int*)need(kv, "sot", 4, n_pre);
  p.tok_emb = (const h16*)need(kv, "tok_emb", 2, V * d);
  p.pos = (const float*)need(kv, "pos", 4, T * d);
  p.x = (float*)need(kv, "x", 4, B * d);
  ids_below(kv, "off", B, T, "clip offset");
  ids_below(kv, "tok", B, V, "token");
  ids_below(kv, "sot", n_pre, V, "prefix token");
  if (has(kv, "forced")) {
    if (p.n_forced < 1) die("advance: forced without n_forced");
    p.forced = (const int*)need(kv, "forced", 4, B * p.n_forced);
    ids_below(kv, "forced", B * p.n_forced, V, "forced token");
    p.done = (int*)ptr(kv, "done", 4, B);
    p.n_out = (int*)ptr(kv, "n_out", 4, B);
    p.out_ids = (int*)ptr(kv, "out_ids", 4, B * T);
  } else {
    p.done = (int*)need(kv, "done", 4, B);
    p.n_out = (int*)need(kv, "n_out", 4, B);
    p.out_ids = (int*)need(kv, "out_ids", 4, B * T);
    ids_below(kv, "n_out", B, T, "id count");
  }
  if (has(kv, "argmax_dump")) p.argmax_dump = (int*)need(kv, "argmax_dump", 4, B * (p.n_forced + 1));
  p.max_new_clip = (const int*)ptr(kv, "max_new_clip", 4, B);
  p.done_host = (int*)ptr(kv, "done_host", 4, B);
  launch_advance(p, nullptr);
  return (B + 15) / 16;
}

static long run_embed(const KV& kv) {
  const long B = num(kv, "batch"), d = num(kv, "d"), V = num(kv, "n_vocab"), T = num(kv, "n_ctx");
  if (B < 1 || d < 1 || V < 1 || T < 1) die("bad embed shape");
  const h16* te = (const h16*)need(kv, "tok_emb", 2, V * d);
  const float* pos = (const float*)need(kv, "pos", 4, T * d);
  const int* tok = (const int*)need(kv, "tok", 4, B);
  const int* off = (const int*)need(kv, "off", 4, B);
  float* x = (float*)need(kv, "x", 4, B * d);
  ids_below(kv, "tok", B, V, "token");
  ids_below(kv, "off", B, T, "clip offset");
  launch_embed(te, pos, tok, off, x, (int)B, (int)d, nullptr);
  return B;
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: decode_kernels_driver <manifest>");
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
    } else if (cmd == "cgemm" || cmd == "dgemm" || cmd == "actprep" || cmd == "attn" || cmd == "packw" || cmd == "packw_split" || cmd == "gemv" ||
               cmd == "advance" || cmd == "embed") {
      KV kv;
      while (ls >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) die("bad token " + tok);
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
      }
      long gx = 1, gy = 1, gz = 1;
      if (cmd == "gemv") {
        gx = run_gemv(kv);
      } else if (cmd == "advance") {
        gx = run_advance(kv);
      } else if (cmd == "embed") {
        gx = run_embed(kv);
      } else if (cmd == "cgemm") {
        DecCGemmParams p{};
        p.N = (int)num(kv, "N"); p.K = (int)num(kv, "K"); p.batch = (int)num(kv, "batch"); p.nbs = (int)num(kv, "nbs");
        p.epilogue = (int)num(kv, "epilogue"); p.rt = (int)num(kv, "rt", 1); p.d_model = (int)num(kv, "d_model");
        p.n_ctx_pad = (int)num(kv, "n_ctx_pad"); p.kv_batch_stride = num(kv, "kv_batch_stride"); p.fold_row0 = (int)num(kv, "fold_row0");
        const long N = p.N, K = p.K, B = p.batch, KS = K / 32, n_rb = (N + 15) / 16, nbs = p.nbs, fr0 = p.fold_row0, d = p.d_model;
        if (N < 1 || K < 128 || K % 128 || B < 1 || nbs < (B + 15) / 16 || (p.rt != 1 && p.rt != 2) || fr0 < 0 || fr0 >= N) die("bad cgemm shape");
        const bool ln = has(kv, "ln_w");
        p.W = (const h16*)need(kv, "W", 2, layout::wfrag_tile_offset(n_rb, 0, KS));
        p.bias = (const float*)ptr(kv, "bias", 4, N);
        if (ln) {
          if (K > 1280) die("LayerNorm prologue: K > 1280");
          p.x = (const float*)need(kv, "x", 4, B * K);
          p.ln_w = (const float*)need(kv, "ln_w", 4, K);
          p.ln_b = (const float*)need(kv, "ln_b", 4, K);
        } else {
          p.a_hi = (const h16*)need(kv, "a_hi", 2, layout::pair_elems(KS, nbs));
          p.a_lo = (const h16*)need(kv, "a_lo", 2, layout::pair_elems(KS, nbs));
        }
        if (fr0 > 0) {  // what launch_decode_cgemm aborts on, and the row blocks W_lo is indexed with
          if (fr0 % (16 * p.rt) || (N - fr0) % (16 * p.rt)) die("query fold: fold_row0 and the fold rows are whole row tiles");
          p.out2 = (float*)need(kv, "out2", 4, B * (N - fr0));
          if (ln) p.ln_w2 = (const float*)need(kv, "ln_w2", 4, K);
          else {
            if (K > 1024) die("query fold: pair input with K > 1024");
            p.W_lo = (const h16*)need(kv, "W_lo", 2, layout::wfrag_tile_offset((N - fr0) / 16, 0, KS));
          }
        }
        const long nx = fr0 > 0 ? fr0 : N;
        switch (p.epilogue) {
          case GEPI_STORE:
            if (fr0) die("STORE has no fold rows");
            p.out = (float*)need(kv, "out", 4, B * N);
            break;
          case GEPI_RESID:
            if (fr0 && ln) die("RESID fold rows take the pair input");
            p.out = (float*)need(kv, "out", 4, B * nx);
            if (has(kv, "stat_part")) {
              if (p.rt != 1 || nx % 16) die("stat_part: one row tile per workgroup, whole 16-row blocks");
              p.stat_part = (float*)need(kv, "stat_part", 4, B * (nx / 16) * 2);
            }
            break;
          case GEPI_GELU:
            if (fr0) die("GELU has no fold rows");
            p.out_hi = (h16*)need(kv, "out_hi", 2, layout::pair_elems((N + 31) / 32, nbs));
            p.out_lo = (h16*)need(kv, "out_lo", 2, layout::pair_elems((N + 31) / 32, nbs));
            break;
          case GEPI_QKV_CACHE:
            if (!(N == 3 * d && fr0 == 0) && !(N == 4 * d && fr0 == 3 * d && ln)) die("QKV_CACHE: N is 3 d_model, or 4 d_model with fold rows");
            p.out = (float*)need(kv, "out", 4, B * d);
            check_cache(kv, B, d, p.n_ctx_pad, p.kv_batch_stride, p.k_cache, p.v_cache, p.off);
            break;
          default: die("unknown cgemm epilogue");
        }
        gx = (N + 16 * p.rt - 1) / (16 * p.rt); gy = (B + 15) / 16;
        launch_decode_cgemm(p, nullptr);
      } else if (cmd == "dgemm") {
        DecGemmParams p{};
        p.N = (int)num(kv, "N"); p.K = (int)num(kv, "K"); p.batch = (int)num(kv, "batch"); p.nbs = (int)num(kv, "nbs");
        p.epilogue = (int)num(kv, "epilogue"); p.rt = (int)num(kv, "rt", 1); p.d_model = (int)num(kv, "d_model");
        p.n_ctx_pad = (int)num(kv, "n_ctx_pad"); p.kv_batch_stride = num(kv, "kv_batch_stride");
        p.ksplit = (int)num(kv, "ksplit", 1); p.part_batch = (int)num(kv, "part_batch");
        p.amax_stride = (int)num(kv, "amax_stride"); p.logits_dump_stride = num(kv, "logits_dump_stride"); p.skip_before_step = (int)num(kv, "skip_before_step");
        const long N = p.N, K = p.K, B = p.batch, KS = K / 32, n_rb = (N + 15) / 16, nbs = p.nbs, d = p.d_model;
        if (N < 1 || K < 128 || K % 128 || B < 1 || B > 64 || nbs < (B + 15) / 16 || (p.rt != 0 && p.rt != 1 && p.rt != 2 && p.rt != 4)) die("bad dgemm shape");
        if (p.rt == 0 && (p.epilogue != GEPI_LOGITS || !decode_logits_resident_ok(p.K, p.batch))) die("rt 0: the resident vocabulary projection does not take this launch");
        p.W = (const h16*)need(kv, "W", 2, layout::wfrag_tile_offset(n_rb, 0, KS));
        p.bias = (const float*)ptr(kv, "bias", 4, N);
        p.a_hi = (const h16*)need(kv, "a_hi", 2, layout::pair_elems(KS, nbs));
        p.a_lo = (const h16*)need(kv, "a_lo", 2, layout::pair_elems(KS, nbs));
        gx = decode_gemm_grid(p.N, p.rt);
        switch (p.epilogue) {
          case GEPI_STORE: case GEPI_RESID: p.out = (float*)need(kv, "out", 4, B * N); break;
          case GEPI_GELU:
            p.out_hi = (h16*)need(kv, "out_hi", 2, layout::pair_elems((N + 31) / 32, nbs));
            p.out_lo = (h16*)need(kv, "out_lo", 2, layout::pair_elems((N + 31) / 32, nbs));
            break;
          case GEPI_QKV_CACHE:
            if (N != 3 * d) die("QKV_CACHE: N is 3 d_model");
            p.out = (float*)need(kv, "out", 4, B * d);
            check_cache(kv, B, d, p.n_ctx_pad, p.kv_batch_stride, p.k_cache, p.v_cache, p.off);
            break;
          case GEPI_LOGITS:
            if (p.amax_stride < gx) die("amax_stride below the grid");
            p.off = (const int*)need(kv, "off", 4, B);
            p.amax_val = (float*)need(kv, "amax_val", 4, (B - 1) * p.amax_stride + gx);
            p.amax_idx = (int*)need(kv, "amax_idx", 4, (B - 1) * p.amax_stride + gx);
            if (has(kv, "logits_dump")) {
              if (p.logits_dump_stride < N) die("logits_dump_stride below N");
              p.logits_dump = (float*)need(kv, "logits_dump", 4, (B - 1) * p.logits_dump_stride + N);
            }
            break;
          case GEPI_PARTIAL:
            if (p.ksplit < 1 || KS % p.ksplit || p.part_batch < B) die("bad split-K launch");
            p.out = (float*)need(kv, "out", 4, ((long)(p.ksplit - 1) * p.part_batch + B) * N);
            gy = p.ksplit;
            break;
          default: die("unknown dgemm epilogue");
        }
        launch_decode_gemm(p, nullptr);
      } else if (cmd == "actprep") {
        const long B = num(kv, "batch"), K = num(kv, "K"), nbs = num(kv, "nbs"), n_part = num(kv, "n_part"), pb = num(kv, "part_batch");
        const bool do_ln = num(kv, "do_ln") != 0;
        if (B < 1 || K < 32 || K % 32 || K > 2048 || nbs < (B + 15) / 16 || n_part < 0 || n_part > 4 || (n_part && pb < B)) die("bad act_prep shape");
        float* x = (float*)need(kv, "x", 4, B * K);
        const float* g = do_ln ? (const float*)need(kv, "g", 4, K) : nullptr;
        const float* be = do_ln ? (const float*)need(kv, "be", 4, K) : nullptr;
        h16* hi = (h16*)need(kv, "hi", 2, layout::pair_elems(K / 32, nbs));
        h16* lo = (h16*)need(kv, "lo", 2, layout::pair_elems(K / 32, nbs));
        const float* part = n_part ? (const float*)need(kv, "part", 4, ((n_part - 1) * pb + B) * K) : nullptr;
        const float* pbias = n_part ? (const float*)need(kv, "part_bias", 4, K) : nullptr;
        gx = B;
        launch_act_prep(x, g, be, hi, lo, (int)B, (int)K, do_ln, (int)nbs, part, (int)n_part, (int)pb, pbias, nullptr);
      } else if (cmd == "attn") {
        DecAttnParams p{};
        p.batch = (int)num(kv, "batch"); p.n_head = (int)num(kv, "n_head"); p.d_model = (int)num(kv, "d_model"); p.n_keys = (int)num(kv, "n_keys");
        p.cap_blocks = (int)num(kv, "cap_blocks"); p.n_split = (int)num(kv, "n_split", 1); p.kv_batch_stride = num(kv, "kv_batch_stride");
        p.nbs = (int)num(kv, "nbs"); p.done_late = (int)num(kv, "done_late");
        const long B = p.batch, H = p.n_head, d = p.d_model, cap = p.cap_blocks, ns = p.n_split;
        if (B < 1 || H < 1 || d != H * 64 || cap < 1 || ns < 1 || ns > cap || p.kv_batch_stride < H * layout::kv_head_elems(cap * layout::kKvBlockKeys) ||
            !(p.n_keys == -1 || (p.n_keys >= 1 && p.n_keys <= cap * 64))) die("bad attention shape");
        p.k = (const h16*)need(kv, "k", 2, (B - 1) * p.kv_batch_stride + H * layout::kv_head_elems(cap * layout::kKvBlockKeys));
        p.v = (const h16*)need(kv, "v", 2, (B - 1) * p.kv_batch_stride + H * layout::kv_head_elems(cap * layout::kKvBlockKeys));
        p.done = (const int*)need(kv, "done", 4, B);
        if (p.n_keys < 0) {
          p.off = (const int*)need(kv, "off", 4, B);
          const int* ho = host_ints(kv, "off");
          for (long b = 0; b < B; ++b) if (ho[b] < 0 || ho[b] >= cap * 64) die("clip offset outside the cache");
        }
        const bool pair = has(kv, "out_hi");
        if (pair == has(kv, "part")) die("attention writes the pair or the partials");
        if (pair) {
          if (p.nbs < (B + 15) / 16) die("nbs below the clip blocks");
          p.out_hi = (h16*)need(kv, "out_hi", 2, layout::pair_elems(d / 32, p.nbs));
          p.out_lo = (h16*)need(kv, "out_lo", 2, layout::pair_elems(d / 32, p.nbs));
          if (ns > 1) {
            if (ns > 6) die("the fold of a launch takes at most 6 splits");
            p.mpart = (float*)need(kv, "mpart", 4, layout::part_elems(B, H, ns));
            p.mcnt = (unsigned*)need(kv, "mcnt", 4, B * H);
          }
        } else {
          p.part = (float*)need(kv, "part", 4, layout::part_elems(B, H, ns));
        }
        if (has(kv, "tq")) {  // folded query: what launch_decode_attention aborts on
          if (d > 1024 || (ns != 1 && !pair)) die("folded query: unsupported launch");
          p.tq = (const float*)need(kv, "tq", 4, B * d);
          p.stat_part = (const float*)need(kv, "stat_part", 4, B * (d / 16) * 2);
          p.fold_s = (const float*)need(kv, "fold_s", 4, d);
          p.fold_c = (const float*)need(kv, "fold_c", 4, d);
        } else if (has(kv, "wq")) {
          if (d > 1024 || ns > 6 || (ns != 1 && !pair)) die("fused query projection: unsupported launch");
          p.x = (const float*)need(kv, "x", 4, B * d);
          p.ln_w = (const float*)need(kv, "ln_w", 4, d);
          p.ln_b = (const float*)need(kv, "ln_b", 4, d);
          p.wq = (const h16*)need(kv, "wq", 2, d * d);
          p.bq = (const float*)need(kv, "bq", 4, d);
        } else {
          p.q = (const float*)need(kv, "q", 4, B * d);
        }
        gx = ns; gy = H; gz = B;
        launch_decode_attention(p, nullptr);
      } else {
        const long N = num(kv, "N"), K = num(kv, "K");
        if (N < 1 || K < 32 || K % 32) die("bad pack shape");
        const long packed = layout::wfrag_elems(N, K);
        if (cmd == "packw") {
          launch_pack_weight_frag((const h16*)need(kv, "w", 2, N * K), (h16*)need(kv, "wp", 2, packed), (int)N, (int)K, nullptr);
        } else {
          launch_pack_weight_frag_split((const float*)need(kv, "w", 4, N * K), (h16*)need(kv, "hi", 2, packed), (h16*)need(kv, "lo", 2, packed),
                                        (int)N, (int)K, nullptr);
        }
        gx = 2048;
      }
      sync_or_die(a.c_str());
      printf("ran %s %ld %ld %ld\n", a.c_str(), gx, gy, gz);
      fflush(stdout);
    } else {
      die("unknown command " + cmd);
    }
  }
  printf("done\n");
  return 0;
}
