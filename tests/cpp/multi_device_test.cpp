// CPU check of whisper.axera_amd/csrc/multi_device.hpp with a stand-in engine (no GPU, no HIP): the sharding of a
// batch over G devices, the joining, error propagation, and the device-list parser. The stand-in takes the engine's own
// request type (iengine.hpp, host only), so the block rule checked here is the one the engines get. Built and run by
// tests/test_multi_device.py with plain g++.
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <set>

#include "iengine.hpp"
#include "multi_device.hpp"

using I = axw::IEngine;

struct FakeEngine {
  int device;
  std::mutex mu;
  std::vector<std::pair<int, const float*>> calls;  // (batch, first clip pointer)
  int fail_on_value = -1;
  static std::atomic<int> concurrent, max_concurrent, wait_ms;
  explicit FakeEngine(int d) : device(d) {}
  std::mutex& mutex() { return mu; }
  using DecodeRequest = I::DecodeRequest;
  using ClipContexts = I::ClipContexts;
  struct Window { int file, seek; };
  struct Options { float threshold; };
  // what the last call was handed (check_offsets)
  I::DecodeMode seen_mode = I::kDecodePlain;
  const int* seen_max_new_clip = nullptr;
  I::ClipScores seen_scores{};
  const Options* seen_opts = nullptr;
  // check_request_blocks: the ids row stride; echo: every optional part of clip b goes into clip b's outputs; bare: no optional part
  // was promised, a pointer that arrives all the same is an error
  int n_ctx = 448;
  bool echo = false, bare = false;
  void run_tokens(const DecodeRequest& rq, const float* const* pcm, const float* d_pcm, int, const int* n_samples, int batch, int32_t* ids,
                  int* n_ids) {
    assert(d_pcm == nullptr);
    const int max_new = rq.max_new;
    seen_mode = rq.mode;
    seen_max_new_clip = rq.max_new_clip;
    seen_scores = rq.scores ? *rq.scores : I::ClipScores{};
    const I::LangResult& lo = rq.ctx.lang_out;
    if (bare && (rq.max_new_clip || rq.sample || rq.scores || rq.ctx.prompts || rq.ctx.lang || lo.detected || lo.lang_logprob || lo.lang_logit))
      throw std::runtime_error("an optional part arrived that the call did not carry");
    const int c = ++concurrent;
    int m = max_concurrent.load();
    while (c > m && !max_concurrent.compare_exchange_weak(m, c)) {}
    // stay inside the call until a second worker has been seen inside too (or 2 s: a single worker / a serial bug), so the
    // side-by-side check below does not depend on how fast a loaded machine starts threads
    for (int i = 0; i < wait_ms.load() && max_concurrent.load() < 2; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    calls.push_back({batch, pcm[0]});
    for (int b = 0; b < batch; ++b) {
      if ((int)pcm[b][0] == fail_on_value) { --concurrent; throw std::runtime_error("clip " + std::to_string((int)pcm[b][0]) + " is poisoned"); }
      // ids are a function of the clip content only: [value, value + 1, ...], n = samples % 5 + 1, capped by max_new
      int n = n_samples[b] % 5 + 1;
      if (max_new > 0 && n > max_new) n = max_new;
      n_ids[b] = n;
      for (int i = 0; i < n; ++i) ids[(size_t)b * n_ctx + i] = (int32_t)pcm[b][0] + i;
      if (echo) echo_clip(rq, b, (int32_t)pcm[b][0], ids + (size_t)b * n_ctx, n_ids + b);
    }
    --concurrent;
  }
  // n_ctx = 8, n_lang = 3, prompts of stride 4. ids row: clip value, prompt length, the prompt (0 beyond it), language, task;
  // token_logprob row: budget, temperature, stream, seed, 0 ..; detected: language * 100 + task; lang_logprob row: temperature, language, task
  static void echo_clip(const DecodeRequest& rq, int b, int32_t value, int32_t* ids, int* n_ids) {
    const I::PromptSpec& pr = *rq.ctx.prompts;
    assert(pr.stride == 4);
    ids[0] = value; ids[1] = pr.n_prompt[b];
    for (int i = 0; i < 4; ++i) ids[2 + i] = i < pr.n_prompt[b] ? pr.ids[(size_t)b * pr.stride + i] : 0;
    ids[6] = rq.ctx.lang->lang[b]; ids[7] = rq.ctx.lang->task[b];
    *n_ids = 8;
    float* t = rq.scores->token_logprob + (size_t)b * 8;
    std::fill(t, t + 8, 0.f);
    t[0] = (float)rq.max_new_clip[b]; t[1] = rq.sample->temperature[b]; t[2] = (float)rq.sample->stream[b]; t[3] = (float)rq.sample->seed;
    rq.scores->avg_logprob[b] = (float)value; rq.scores->no_speech_logprob[b] = -(float)value; rq.scores->ended_eot[b] = pr.n_prompt[b] % 2;
    rq.ctx.lang_out.detected[b] = rq.ctx.lang->lang[b] * 100 + rq.ctx.lang->task[b];
    float* l = rq.ctx.lang_out.lang_logprob + (size_t)b * 3;
    l[0] = rq.sample->temperature[b]; l[1] = (float)rq.ctx.lang->lang[b]; l[2] = (float)rq.ctx.lang->task[b];
  }
  // two windows per file, file counted from 0 within this call
  void run_long_windows(const float* const* pcm, const int*, int n_files, int, int, const Options* opts, std::vector<Window>& log) {
    seen_opts = opts;
    calls.push_back({n_files, pcm[0]});
    for (int f = 0; f < n_files; ++f)
      for (int k = 0; k < 2; ++k) log.push_back({f, 1000 * device + k});
  }
};
std::atomic<int> FakeEngine::concurrent{0}, FakeEngine::max_concurrent{0}, FakeEngine::wait_ms{0};

static I::DecodeRequest request(I::DecodeMode mode, int max_new, const int* max_new_clip = nullptr, const I::ClipScores* scores = nullptr) {
  I::DecodeRequest rq;
  rq.mode = mode; rq.max_new = max_new; rq.max_new_clip = max_new_clip;
  if (scores) rq.scores = *scores;
  return rq;
}

static void check_shards() {
  for (int n : {0, 1, 5, 7, 64, 512, 513})
    for (int world : {1, 2, 3, 8}) {
      int next = 0;
      for (int r = 0; r < world; ++r) {
        int lo, hi;
        axw::shard_range(n, r, world, &lo, &hi);
        assert(lo == next || (lo == n && hi == n));
        assert(lo <= hi && hi <= n);
        next = hi > next ? hi : next;
      }
      assert(next == n);
    }
  int lo, hi;
  axw::shard_range(512, 3, 8, &lo, &hi);
  assert(lo == 192 && hi == 256);  // BASELINE configs[4]: 64 clips per GPU
}

static void run_case(int G, int B, int max_new) {
  axw::DeviceGroup<FakeEngine> g;
  for (int d = 0; d < G; ++d) g.add(std::unique_ptr<FakeEngine>(new FakeEngine(d)));
  std::vector<std::vector<float>> clips(B);
  std::vector<const float*> ptrs(B);
  std::vector<int> lens(B);
  for (int b = 0; b < B; ++b) { clips[b].assign(3 + b % 4, (float)(1000 + 10 * b)); ptrs[b] = clips[b].data(); lens[b] = (int)clips[b].size(); }
  std::vector<int32_t> ids((size_t)B * 448, -1), want((size_t)B * 448, -1);
  std::vector<int> n(B, -1), wn(B, -1);
  FakeEngine::max_concurrent = 0;
  FakeEngine::wait_ms = (G < B ? G : B) > 1 ? 2000 : 0;
  g.run_tokens(request(I::kDecodePlain, max_new), ptrs.data(), lens.data(), B, 448, 0, ids.data(), n.data());
  FakeEngine::wait_ms = 0;
  FakeEngine single(99);
  single.run_tokens(request(I::kDecodePlain, max_new), ptrs.data(), nullptr, 0, lens.data(), B, want.data(), wn.data());
  assert(n == wn && ids == want);  // joined result == one engine over the whole batch, in order
  const int world = G < B ? G : B, per = (B + world - 1) / world;
  int covered = 0;
  for (int d = 0; d < G; ++d) {
    FakeEngine& e = g.at(d);
    if (d < world && d * per < B) {
      assert(e.calls.size() == 1);
      assert(e.calls[0].second == ptrs[d * per]);                              // contiguous block d
      assert(e.calls[0].first == (d * per + per < B ? per : B - d * per));
      covered += e.calls[0].first;
    } else {
      assert(e.calls.empty());
    }
  }
  assert(covered == B);
  if (world > 1) assert(FakeEngine::max_concurrent.load() > 1);  // the devices really ran side by side
}

static void check_errors() {
  axw::DeviceGroup<FakeEngine> g;
  for (int d = 0; d < 4; ++d) g.add(std::unique_ptr<FakeEngine>(new FakeEngine(d)));
  g.at(2).fail_on_value = 1000 + 10 * 5;  // clip 5 lives in block 2 of 4 x 2
  const int B = 8;
  std::vector<std::vector<float>> clips(B);
  std::vector<const float*> ptrs(B);
  std::vector<int> lens(B, 4);
  for (int b = 0; b < B; ++b) { clips[b].assign(4, (float)(1000 + 10 * b)); ptrs[b] = clips[b].data(); }
  std::vector<int32_t> ids((size_t)B * 448);
  std::vector<int> n(B);
  bool threw = false;
  try {
    g.run_tokens(request(I::kDecodePlain, 0), ptrs.data(), lens.data(), B, 448, 0, ids.data(), n.data());
  } catch (const std::exception& e) {
    threw = true;
    assert(strstr(e.what(), "device worker 2") && strstr(e.what(), "poisoned"));
  }
  assert(threw);
  for (int d = 0; d < 4; ++d) assert(g.at(d).calls.size() == 1);  // every worker was joined (none left running)
  bool t2 = false;
  try { g.run_tokens(request(I::kDecodePlain, 0), ptrs.data(), lens.data(), 0, 448, 0, ids.data(), n.data()); } catch (const std::exception&) { t2 = true; }
  assert(t2);
}

static void check_rotation() {
  // fewer clips than devices: consecutive calls start at consecutive devices (concurrent 1-clip requests spread out)
  axw::DeviceGroup<FakeEngine> g;
  for (int d = 0; d < 3; ++d) g.add(std::unique_ptr<FakeEngine>(new FakeEngine(d)));
  std::vector<float> clip(4, 7.f);
  const float* ptr = clip.data();
  int len = 4, n = 0;
  std::vector<int32_t> ids(448);
  for (int call = 0; call < 7; ++call) g.run_tokens(request(I::kDecodePlain, 0), &ptr, &len, 1, 448, 0, ids.data(), &n);
  assert(g.at(0).calls.size() == 3 && g.at(1).calls.size() == 2 && g.at(2).calls.size() == 2);
  // two clips on three devices: devices (1, 2) after seven 1-clip calls, then (0, 1)
  const float* two[2] = {ptr, ptr};
  int lens[2] = {4, 4}, ns[2];
  std::vector<int32_t> ids2(2 * 448);
  g.run_tokens(request(I::kDecodePlain, 0), two, lens, 2, 448, 0, ids2.data(), ns);
  assert(g.at(1).calls.size() == 3 && g.at(2).calls.size() == 3 && g.at(0).calls.size() == 3);
  // a full batch always uses every device, block w on device w
  const float* six[6] = {ptr, ptr, ptr, ptr, ptr, ptr};
  int lens6[6] = {4, 4, 4, 4, 4, 4}, ns6[6];
  std::vector<int32_t> ids6(6 * 448);
  g.run_tokens(request(I::kDecodePlain, 0), six, lens6, 6, 448, 0, ids6.data(), ns6);
  for (int d = 0; d < 3; ++d) assert(g.at(d).calls.size() == 4 && g.at(d).calls.back().first == 2);
}

static void check_offsets() {
  // every per-clip array of a call reaches worker w offset by its block's first clip (token_logprob: by whole rows); a long-form
  // log comes back worker by worker with the files renumbered over the whole call
  const int G = 3, B = 7, n_ctx = 448, per = 3;  // blocks [0, 3), [3, 6), [6, 7)
  axw::DeviceGroup<FakeEngine> g;
  for (int d = 0; d < G; ++d) g.add(std::unique_ptr<FakeEngine>(new FakeEngine(d)));
  std::vector<std::vector<float>> clips(B);
  std::vector<const float*> ptrs(B);
  std::vector<int> lens(B, 4), budgets(B, 2), n(B), eot(B);
  for (int b = 0; b < B; ++b) { clips[b].assign(4, (float)(1000 + 10 * b)); ptrs[b] = clips[b].data(); }
  std::vector<int32_t> ids((size_t)B * n_ctx);
  std::vector<float> tok((size_t)B * n_ctx), avg(B), nsp(B);
  const I::ClipScores scores{tok.data(), avg.data(), nsp.data(), eot.data()};
  g.run_tokens(request(I::kDecodeScored, 0, budgets.data(), &scores), ptrs.data(), lens.data(), B, n_ctx, 0, ids.data(), n.data());
  for (int w = 0; w < G; ++w) {
    const FakeEngine& e = g.at(w);
    const int lo = w * per;
    assert(e.calls.size() == 1 && e.calls[0].second == ptrs[lo]);
    assert(e.seen_mode == I::kDecodeScored);
    assert(e.seen_max_new_clip == budgets.data() + lo);
    assert(e.seen_scores.token_logprob == tok.data() + (size_t)lo * n_ctx);
    assert(e.seen_scores.avg_logprob == avg.data() + lo && e.seen_scores.no_speech_logprob == nsp.data() + lo);
    assert(e.seen_scores.ended_eot == eot.data() + lo);
  }
  // absent arrays stay absent
  const I::ClipScores only_avg{nullptr, avg.data(), nullptr, nullptr};
  g.run_tokens(request(I::kDecodeScored, 0, nullptr, &only_avg), ptrs.data(), lens.data(), B, n_ctx, 0, ids.data(), n.data());
  for (int w = 0; w < G; ++w) {
    const FakeEngine& e = g.at(w);
    assert(e.seen_max_new_clip == nullptr && e.seen_scores.token_logprob == nullptr && e.seen_scores.ended_eot == nullptr);
    assert(e.seen_scores.avg_logprob == avg.data() + w * per && e.seen_scores.no_speech_logprob == nullptr);
  }
  const FakeEngine::Options opts{0.5f};
  std::vector<FakeEngine::Window> log;
  g.run_long_windows(ptrs.data(), lens.data(), B, 0, 0, &opts, log);
  assert(log.size() == (size_t)2 * B);
  for (int f = 0; f < B; ++f)
    for (int k = 0; k < 2; ++k) {
      const FakeEngine::Window& x = log[(size_t)2 * f + k];
      assert(x.file == f && x.seek == 1000 * (f / per) + k);  // worker 0's windows first, files counted over the whole call
    }
  for (int w = 0; w < G; ++w) assert(g.at(w).seen_opts == &opts && g.at(w).calls.back().second == ptrs[w * per]);
}

// every optional part of a request travels with its clips: the joined result of G engines equals one engine's over the whole batch,
// and a request without optional parts reaches every shard without any
static void check_request_blocks(int G, int B) {
  const int n_ctx = 8, n_lang = 3, stride = 4;
  std::vector<std::vector<float>> clips(B);
  std::vector<const float*> ptrs(B);
  std::vector<int> lens(B, 4), budgets(B), n_prompt(B), lang(B), task(B);
  std::vector<int32_t> prompt_ids((size_t)B * stride, -7);
  std::vector<float> temps(B);
  std::vector<uint64_t> streams(B);
  for (int b = 0; b < B; ++b) {
    clips[b].assign(4, (float)(1000 + 10 * b)); ptrs[b] = clips[b].data();
    budgets[b] = 1 + b; n_prompt[b] = 1 + b % stride; lang[b] = 10 + b; task[b] = 50 - b;
    for (int i = 0; i < n_prompt[b]; ++i) prompt_ids[(size_t)b * stride + i] = 100 * b + i;
    temps[b] = 0.25f * (float)(b + 1); streams[b] = 7000 + (uint64_t)b;
  }
  struct Out {
    std::vector<int32_t> ids; std::vector<int> n, eot, detected; std::vector<float> tok, avg, nsp, lang_lp;
    explicit Out(int B) : ids((size_t)B * 8, -1), n(B, -1), eot(B, -1), detected(B, -1), tok((size_t)B * 8, -1.f), avg(B, -1.f), nsp(B, -1.f), lang_lp((size_t)B * 3, -1.f) {}
    bool operator==(const Out& o) const {
      return ids == o.ids && n == o.n && eot == o.eot && detected == o.detected && tok == o.tok && avg == o.avg && nsp == o.nsp && lang_lp == o.lang_lp;
    }
  };
  auto full = [&](Out& o) {
    const I::ClipScores scores{o.tok.data(), o.avg.data(), o.nsp.data(), o.eot.data()};
    I::DecodeRequest rq = request(I::kDecodeSampled, 5, budgets.data(), &scores);
    rq.sample = I::SampleSpec{temps.data(), streams.data(), 77};
    rq.ctx.prompts = I::PromptSpec{prompt_ids.data(), stride, n_prompt.data()};
    rq.ctx.lang = I::LangSpec{lang.data(), task.data()};
    rq.ctx.lang_out = {o.detected.data(), o.lang_lp.data(), nullptr};
    return rq;
  };
  axw::DeviceGroup<FakeEngine> g;
  for (int d = 0; d < G; ++d) {
    g.add(std::unique_ptr<FakeEngine>(new FakeEngine(d)));
    g.at(d).n_ctx = n_ctx; g.at(d).echo = true;
  }
  Out got(B), want(B);
  g.run_tokens(full(got), ptrs.data(), lens.data(), B, n_ctx, n_lang, got.ids.data(), got.n.data());
  FakeEngine single(99);
  single.n_ctx = n_ctx; single.echo = true;
  single.run_tokens(full(want), ptrs.data(), nullptr, 0, lens.data(), B, want.ids.data(), want.n.data());
  assert(got == want);
  const int per = (B + G - 1) / G;
  for (int d = 0; d < G; ++d) assert(g.at(d).calls.size() == 1 && g.at(d).calls[0].first == (d * per + per < B ? per : B - d * per));
  for (int b = 0; b < B; ++b) {  // (and the single engine's is what the clip was given)
    assert(want.ids[(size_t)b * 8 + 1] == n_prompt[b] && want.ids[(size_t)b * 8 + 2] == 100 * b && want.ids[(size_t)b * 8 + 6] == lang[b]);
    assert(want.tok[(size_t)b * 8] == (float)budgets[b] && want.tok[(size_t)b * 8 + 2] == (float)streams[b] && want.tok[(size_t)b * 8 + 3] == 77.f);
    assert(want.detected[b] == lang[b] * 100 + task[b] && want.lang_lp[(size_t)b * 3] == temps[b]);
  }
  // nothing optional: every shard sees none of it either
  for (int d = 0; d < G; ++d) { g.at(d).echo = false; g.at(d).bare = true; }
  g.run_tokens(request(I::kDecodeTimestamps, 5), ptrs.data(), lens.data(), B, n_ctx, n_lang, got.ids.data(), got.n.data());
  for (int d = 0; d < G; ++d) assert(g.at(d).calls.size() == 2 && g.at(d).seen_mode == I::kDecodeTimestamps);
}

static void check_device_lists() {
  using axw::parse_device_list;
  assert((parse_device_list("all", 3) == std::vector<int>{0, 1, 2}));
  assert((parse_device_list("", 2) == std::vector<int>{0, 1}));
  assert((parse_device_list("2,0", 4) == std::vector<int>{2, 0}));
  for (const char* bad : {"0,,1", "a", "0,4", "1,1", "-1", "0,"}) {
    bool threw = false;
    try { parse_device_list(bad, 4); } catch (const std::exception&) { threw = true; }
    assert(threw);
  }
}

int main() {
  check_shards();
  for (int G : {1, 2, 3, 8})
    for (int B : {1, 2, 5, 8, 64, 65}) run_case(G, B, B % 2 ? 0 : 3);
  check_errors();
  check_rotation();
  check_offsets();
  check_request_blocks(3, 7);  // blocks of 3, 3 and 1
  check_request_blocks(2, 5);  // blocks of 3 and 2
  check_device_lists();
  printf("multi_device ok\n");
  return 0;
}
