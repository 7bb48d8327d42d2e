// long_cuts.hpp — chunked long-form, host side (no HIP types): the definitions of the levels, the cut rule and a window's segments
// in file time (DESIGN.md "Chunked long-form"). The kernels of long_cuts.hip compute the levels and run the same rule on the device;
// tests/long_cuts_reference.py restates all of it independently.
//
// A file of n_samples samples has n_frames = 1 + n_samples / 160 rows S[f][m] in the log-mel store (fp32, before the clamp), the maximum
// G over all of them, and content = n_samples / 160 frames of audio.
//   what the encoder will see   x[f][m] = (max(S[f][m], G - 8) + 4) / 4                       (mel_window_kernel's arithmetic)
//   frame level                 e[f]    = mean over m of x[f][m]
//   smoothed level              s[f]    = 1 / (2 R + 1) * sum over j = -R .. R of e[clamp(f + j, 0, n_frames - 1)]
// R = smooth_frames, 0 .. 64 (default 25: a box of 0.51 s).
//
// The cut rule is a pure function of the fp32 array s[0 .. content) and three integers: content, W_min and W_max (both even,
// 2 <= W_min <= W_max <= 3000; defaults 2000 and 3000).
//   seek = 0
//   while content - seek > W_max:
//     among the even f in [seek + W_min, seek + W_max] take the one with the smallest s[f] (compared as fp32, exactly; a tie goes to
//     the largest f); emit the window (seek, f - seek); seek = f
//   emit the last window (seek, content - seek)
// Cuts are even, so segment times stay multiples of 0.02 s. A file has at most ceil(content / W_min) + 1 windows; a file below one
// frame (content 0) has none. s must be finite (the levels of finite PCM are).
//
// A window's features are rows [seek, seek + len) of the store, clamped and scaled; frames len .. 2999 are zero (mel_window_cut_kernel).
// A window's segments: AX_WHISPER_SplitSegments' contract on the window's ids (the trailing piece is kept: no later window decodes
// that audio again) with clip_seconds = len / 100, every time t mapped to seek / 100 + min(t, len / 100).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace axw {

constexpr int kCutMaxFrames = 3000;     // W_max's ceiling: the encoder's window
constexpr int kCutSmoothMax = 64;       // R's ceiling: the halo the levels kernel keeps in LDS
constexpr int kCutDefaultMax = 3000, kCutDefaultMin = 2000, kCutDefaultSmooth = 25;

struct CutParams {
  int w_max = kCutDefaultMax, w_min = kCutDefaultMin, smooth = kCutDefaultSmooth;
};

// empty: the parameters are accepted; else why not
inline std::string cut_params_error(int w_min, int w_max, int smooth) {
  if (w_min < 2 || w_max < w_min || w_max > kCutMaxFrames)
    return "chunked long-form: need 2 <= chunk_min_frames <= chunk_max_frames <= 3000, got " + std::to_string(w_min) + " and " + std::to_string(w_max);
  if ((w_min & 1) || (w_max & 1))
    return "chunked long-form: chunk_min_frames and chunk_max_frames must be even, got " + std::to_string(w_min) + " and " + std::to_string(w_max);
  if (smooth < 0 || smooth > kCutSmoothMax) return "chunked long-form: smooth_frames must be 0 .. 64, got " + std::to_string(smooth);
  return std::string();
}

// windows a file of `content` frames can have at most under W_min
inline int cut_plan_capacity(int content, int w_min) { return content <= 0 ? 0 : (content + w_min - 1) / w_min + 1; }

struct CutWindow { int seek, len; };

// The rule, literally. s: [content] at least.
inline std::vector<CutWindow> cut_plan(const float* s, int content, int w_min, int w_max) {
  const std::string bad = cut_params_error(w_min, w_max, 0);
  if (!bad.empty()) throw std::runtime_error(bad);
  std::vector<CutWindow> out;
  if (content <= 0) return out;
  for (int f = 0; f < content; ++f)
    if (!std::isfinite(s[f])) throw std::runtime_error("chunked long-form: level " + std::to_string(f) + " is not finite");
  int seek = 0;
  while (content - seek > w_max) {
    int best = seek + w_min;
    for (int f = best + 2; f <= seek + w_max; f += 2)
      if (s[f] <= s[best]) best = f;  // ascending f: a tie goes to the later frame
    out.push_back({seek, best - seek});
    seek = best;
  }
  out.push_back({seek, content - seek});
  return out;
}

// The levels in float64, for reference use. store: [n_frames][n_mels] fp32 rows, gmax: the file's maximum.
inline void frame_levels_reference(const float* store, int n_frames, int n_mels, float gmax, int smooth, std::vector<double>& e, std::vector<double>& s) {
  e.assign((size_t)n_frames, 0.0);
  s.assign((size_t)n_frames, 0.0);
  const float floor_v = gmax - 8.0f;
  for (int f = 0; f < n_frames; ++f) {
    double sum = 0.0;
    for (int m = 0; m < n_mels; ++m) sum += (double)((std::fmax(store[(size_t)f * n_mels + m], floor_v) + 4.0f) * 0.25f);
    e[f] = sum / n_mels;
  }
  for (int f = 0; f < n_frames; ++f) {
    double sum = 0.0;
    for (int j = -smooth; j <= smooth; ++j) sum += e[(size_t)std::min(std::max(f + j, 0), n_frames - 1)];
    s[f] = sum / (2 * smooth + 1);
  }
}

struct ChunkSegment {
  double start, end;       // seconds in FILE time
  int tok_begin, tok_end;  // text ids of the segment: ids[tok_begin .. tok_end)
};

// One window's ids (eot excluded) -> its segments in file time. T = timestamp_begin, E = eot; the window is (seek, len) in frames.
// The split is AX_WHISPER_SplitSegments' (api.cpp), restated here on doubles: pairs of consecutive timestamps close segments, ids that
// end in a single timestamp close the last one, a tail after the last pair is kept and runs to the window's end; without pairs one
// segment over the whole window. A segment without text ids is dropped. Every window time t becomes seek / 100 + min(t, len / 100).
inline std::vector<ChunkSegment> chunked_segments(const int32_t* ids, int n, int T, int E, int seek, int len) {
  std::vector<ChunkSegment> out;
  const double clip = (double)len * 0.01, base = (double)seek * 0.01;
  auto ts = [&](int i) { return ids[i] >= T; };
  auto time = [&](int i) { return (double)(ids[i] - T) * 0.02; };
  auto emit = [&](int lo, int hi, double t0, double t1) {
    int tb = -1, te = -1;
    for (int i = lo; i < hi; ++i)
      if (ids[i] < E) { if (tb < 0) tb = i; te = i + 1; }
    if (tb < 0) return;
    out.push_back({base + std::min(t0, clip), base + std::min(t1, clip), tb, te});
  };
  std::vector<int> bounds;
  for (int i = 1; i < n; ++i)
    if (ts(i - 1) && ts(i)) bounds.push_back(i);
  if (!bounds.empty()) {
    if (n >= 2 && ts(n - 1) && !ts(n - 2)) bounds.push_back(n);
    int prev = 0;
    double prev_end = 0.0;
    for (int b : bounds) {
      prev_end = time(b - 1);
      emit(prev, b, time(prev), prev_end);
      prev = b;
    }
    if (prev < n) emit(prev, n, ts(prev) ? time(prev) : prev_end, clip);
  } else {
    int last = -1;
    for (int i = 0; i < n; ++i)
      if (ts(i)) last = i;
    emit(0, n, 0.0, (last >= 0 && ids[last] != T) ? time(last) : clip);
  }
  return out;
}

}  // namespace axw
