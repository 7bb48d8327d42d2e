// multi_device.hpp — utterance-level data parallelism over the GPUs of one node, inside ONE process (host only).
//
// The unit being sharded is the reference's one-utterance Whisper::run (cpp/src/Whisper.cpp:186-239): every utterance's
// front-end, encoder and decode loop share nothing but read-only weights, so a batch of B clips splits into contiguous
// blocks of ceil(B / G) clips, one block per device, with no collective at all inside a process: each
// device's engine writes its block of the caller's result arrays directly (plain D2H per device). The multi-process
// form of the same partitioning (one rank per GPU, RCCL all_gather of the ids) is whisper.axera_amd/dp.py + bench.py.
//
// Header-only and free of HIP types on purpose: tests/test_multi_device.py instantiates DeviceGroup with a stand-in
// engine under plain g++ to check the sharding and the joining on a box without a GPU.
#pragma once

#include <atomic>
#include <cstdint>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

namespace axw {

// contiguous block [lo, hi) of ceil(n / world) items for worker `rank`; trailing workers may get fewer or none
// (the same rule as dp.shard_range, so the in-process and the multi-process partitions agree)
inline void shard_range(int n, int rank, int world, int* lo, int* hi) {
  const int per = world > 0 ? (n + world - 1) / world : n;
  const long l = (long)rank * per;
  *lo = (int)(l < n ? l : n);
  *hi = *lo + per < n ? *lo + per : n;
}

// fn(worker, lo, hi) for every non-empty shard, one host thread per worker (worker 0 on the calling thread); joins all
// of them, then rethrows the first failure (by worker index) with the worker named in the message.
template <typename Fn>
void run_sharded(int n, int world, Fn&& fn) {
  if (n <= 0 || world <= 0) return;
  std::vector<std::string> errors(world);
  std::vector<char> failed(world, 0);
  auto body = [&](int w) {
    int lo, hi;
    shard_range(n, w, world, &lo, &hi);
    if (hi <= lo) return;
    try {
      fn(w, lo, hi);
    } catch (const std::exception& e) {
      failed[w] = 1;
      errors[w] = e.what();
    } catch (...) {
      failed[w] = 1;
      errors[w] = "unknown error";
    }
  };
  std::vector<std::thread> threads;
  for (int w = 1; w < world; ++w) {
    int lo, hi;
    shard_range(n, w, world, &lo, &hi);
    if (hi > lo) threads.emplace_back(body, w);
  }
  body(0);
  for (auto& t : threads) t.join();
  for (int w = 0; w < world; ++w)
    if (failed[w]) throw std::runtime_error("device worker " + std::to_string(w) + ": " + errors[w]);
}

template <typename O, typename = void> struct has_file_base : std::false_type {};
template <typename O> struct has_file_base<O, decltype((void)std::declval<O&>().file_base)> : std::true_type {};

// G engines, one per device. E needs: std::mutex& mutex(); a copyable struct DecodeRequest with DecodeRequest block(int lo, int n_ctx,
// int n_lang) const, the request of the clips from `lo` on (iengine.hpp states the rule once, for every per-clip array a request
// can carry); run_tokens, run_beam and run_long_windows as they are called below; for detect_language a struct ClipContexts with a
// member lang_out and ClipContexts block(int lo, int n_lang) const.
template <typename E>
class DeviceGroup {
 public:
  DeviceGroup() = default;
  void add(std::unique_ptr<E> e) { engines_.push_back(std::move(e)); }
  int size() const { return (int)engines_.size(); }
  E& at(int i) { return *engines_.at(i); }
  E& primary() { return *engines_.at(0); }

  // Host PCM of `batch` clips -> ids [batch][n_ctx], n_ids [batch] (E::run_tokens). With one engine (or one clip) this is the
  // engine's own call; otherwise workers = min(G, batch) engines each take one contiguous block of the clips, and with it
  // rq.block(first clip, n_ctx, n_lang): budgets, prompts, languages, sample arrays, scores and language results travel with their
  // clips (the random stream ids are the caller's, so a clip's draws do not depend on the device it lands on).
  void run_tokens(const typename E::DecodeRequest& rq, const float* const* pcm, const int* n_samples, int batch, int n_ctx, int n_lang,
                  int32_t* ids, int* n_ids) {
    if (batch < 1) throw std::runtime_error("batch must be >= 1");
    for_each_shard(batch, [&](E& e, int, int lo, int hi) {
      e.run_tokens(rq.block(lo, n_ctx, n_lang), pcm + lo, nullptr, 0, n_samples + lo, hi - lo, ids + (size_t)lo * n_ctx, n_ids + lo);
    });
  }

  // run_tokens, then after(engine, lo, hi) on the same engine while its slots still hold the block's encoder output (word-level
  // timestamps: the alignment of the block's clips)
  template <typename Fn>
  void run_tokens_then(const typename E::DecodeRequest& rq, const float* const* pcm, const int* n_samples, int batch, int n_ctx, int n_lang,
                       int32_t* ids, int* n_ids, Fn&& after) {
    if (batch < 1) throw std::runtime_error("batch must be >= 1");
    for_each_shard(batch, [&](E& e, int, int lo, int hi) {
      e.run_tokens(rq.block(lo, n_ctx, n_lang), pcm + lo, nullptr, 0, n_samples + lo, hi - lo, ids + (size_t)lo * n_ctx, n_ids + lo);
      after(e, lo, hi);
    });
  }

  // Language detection alone (E::detect_language): front-end, encoder and detection of every clip on its shard's device; the results
  // go to out.lang_out.
  void detect_language(const float* const* pcm, const int* n_samples, int batch, int n_lang, const typename E::ClipContexts& out) {
    if (batch < 1) throw std::runtime_error("batch must be >= 1");
    for_each_shard(batch, [&](E& e, int, int lo, int hi) { e.detect_language(pcm + lo, n_samples + lo, hi - lo, out.block(lo, n_lang).lang_out); });
  }

  // Beam search (E::run_beam; R: the result arrays of beam.hpp, all per-clip with row stride n_ctx where they are rows): the clips
  // are split like run_tokens' — every hypothesis of a clip lives on the clip's device.
  template <typename R>
  void run_beam(const float* const* pcm, const int* n_samples, int batch, int beam_size, int max_new, int n_ctx, const R& out,
                float* no_speech_logprob) {
    if (batch < 1) throw std::runtime_error("batch must be >= 1");
    auto from = [](auto* p, size_t k) { return p ? p + k : p; };
    for_each_shard(batch, [&](E& e, int, int lo, int hi) {
      R o = out;
      o.ids = from(out.ids, (size_t)lo * n_ctx); o.n_ids = from(out.n_ids, lo);
      o.sum_logprob = from(out.sum_logprob, lo); o.avg_logprob = from(out.avg_logprob, lo); o.ended_eot = from(out.ended_eot, lo);
      o.rec_ids = from(out.rec_ids, (size_t)lo * beam_size * n_ctx); o.rec_len = from(out.rec_len, (size_t)lo * beam_size);
      o.rec_score = from(out.rec_score, (size_t)lo * beam_size); o.rec_pool = from(out.rec_pool, (size_t)lo * beam_size);
      o.n_rec = from(out.n_rec, lo); o.winner = from(out.winner, lo);
      e.run_beam(pcm + lo, n_samples + lo, hi - lo, beam_size, max_new, o, from(no_speech_logprob, lo));
    });
  }

  // Long-form (E::run_long_windows; opts: the thresholds of the silent-window rule, or null): the FILES are split into contiguous
  // blocks, one per engine; every engine runs its own seek loop. The log holds worker 0's windows first, then worker 1's, ...; file
  // indices count over the whole call, pass and slot are the engine's own. W needs an int member `file`. Options with a member
  // `file_base` (temperature fallback numbers its random streams by file) are handed to every engine with the index of its first file.
  template <typename W, typename O>
  void run_long_windows(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes, const O* opts,
                        std::vector<W>& log) {
    if (n_files < 1) throw std::runtime_error("n_files must be >= 1");
    std::vector<std::vector<W>> logs(size());
    for_each_shard(n_files, [&](E& e, int w, int lo, int hi) {
      if constexpr (has_file_base<O>::value) {
        O mine{};
        if (opts) { mine = *opts; mine.file_base = opts->file_base + lo; }
        e.run_long_windows(pcm + lo, n_samples + lo, hi - lo, max_new, max_passes, opts ? &mine : nullptr, logs[w]);
      } else {
        e.run_long_windows(pcm + lo, n_samples + lo, hi - lo, max_new, max_passes, opts, logs[w]);
      }
      for (W& x : logs[w]) x.file += lo;
    });
    for (auto& l : logs)
      for (W& x : l) log.push_back(std::move(x));
  }

  // Chunked long-form (E::run_long_chunked): the files are split like run_long_windows', every engine plans and decodes its own
  // block, the log is joined the same way. O needs an int member file_base.
  template <typename W, typename O>
  void run_long_chunked(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes, const O& opts, std::vector<W>& log) {
    if (n_files < 1) throw std::runtime_error("n_files must be >= 1");
    std::vector<std::vector<W>> logs(size());
    for_each_shard(n_files, [&](E& e, int w, int lo, int hi) {
      O mine = opts;
      mine.file_base = opts.file_base + lo;
      e.run_long_chunked(pcm + lo, n_samples + lo, hi - lo, max_new, max_passes, mine, logs[w]);
      for (W& x : logs[w]) x.file += lo;
    });
    for (auto& l : logs)
      for (W& x : l) log.push_back(std::move(x));
  }

 private:
  // fn(engine, worker, lo, hi) for every non-empty block of n items (run_sharded over min(G, n) workers). An engine is serialised
  // by its own mutex (a handle may be shared between threads), engines of different devices run concurrently.
  template <typename Fn>
  void for_each_shard(int n, Fn&& fn) {
    const int G = size(), world = G < n ? G : n;
    // calls with fewer items than devices start at a rotating device, so that concurrent small requests on one handle
    // (a server thread pool calling AX_WHISPER_RunPCM) spread over the GPUs instead of queueing on the first engine
    const unsigned first = world < G ? next_.fetch_add((unsigned)world) % (unsigned)G : 0u;
    run_sharded(n, world, [&](int w, int lo, int hi) {
      E& e = *engines_[(first + (unsigned)w) % (unsigned)G];
      std::lock_guard<std::mutex> lock(e.mutex());
      fn(e, w, lo, hi);
    });
  }

  std::vector<std::unique_ptr<E>> engines_;
  std::atomic<unsigned> next_{0};
};

// "0,2,5" / "all" / "" -> device ordinals (all = 0..n_visible-1). Throws on a malformed list or an ordinal out of range.
inline std::vector<int> parse_device_list(const std::string& s, int n_visible) {
  std::vector<int> out;
  if (s.empty() || s == "all") {
    for (int i = 0; i < n_visible; ++i) out.push_back(i);
    return out;
  }
  size_t p = 0;
  while (p <= s.size()) {
    size_t q = s.find(',', p);
    if (q == std::string::npos) q = s.size();
    const std::string tok = s.substr(p, q - p);
    if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos)
      throw std::runtime_error("bad device list '" + s + "'");
    const int d = std::stoi(tok);
    if (d >= n_visible) throw std::runtime_error("device " + tok + " of '" + s + "' is not visible (" + std::to_string(n_visible) + " devices)");
    for (int o : out)
      if (o == d) throw std::runtime_error("device " + tok + " listed twice in '" + s + "'");
    out.push_back(d);
    p = q + 1;
  }
  return out;
}

}  // namespace axw
