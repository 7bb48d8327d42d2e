// resample.hpp — THE definition of the engine's sample-rate conversion to 16 kHz (DESIGN.md §11 "Sample rates"). Host only, no
// HIP type: api.cpp, both engine builds and stand-alone host programs include it; csrc/resample.hip computes the sum below.
//
// For an input rate `rate`: g = gcd(rate, 16000), L = 16000 / g, M = rate / g; c = ROLLOFF min(1, L / M), W = Z / c, K = ceil(W),
// T = 2 K taps per phase. h(t) = c sinc(c t) I0(BETA sqrt(1 - (t / W)^2)) / I0(BETA) for |t| < W, else 0 (sinc(x) = sin(pi x) / (pi x)):
// a Kaiser-windowed sinc with the published "kaiser_best" constants of resampy / librosa. The table is
//   H[r][i] = float32(h((i - K + 1) - r / L)),  r in [0, L), i in [0, T),
// computed in float64 and rounded once. Output j of a clip of n samples, j < n_out = ceil(n L / M):
//   i0 = floor(j M / L), r = (j M) mod L,  y_j = sum over i < T of x[i0 + i - K + 1] H[r][i],  x zero outside [0, n).
// No per-phase normalisation. rate == 16000 is the identity (no filter, samples copied bit for bit).
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace axw {
namespace resample {

constexpr int kTargetRate = 16000;
constexpr int kZ = 64;  // zero crossings of the sinc on each side, at the cutoff's scale
constexpr double kRolloff = 0.9475937167399596;
constexpr double kBeta = 14.769656459379492;
constexpr int kMinRate = 1000, kMaxRate = 384000;
constexpr long long kMaxTable = 1ll << 22;    // L * T entries
constexpr long long kMaxSamples = 1ll << 29;  // n and n_out (the front-end's own cap)

struct Filter {
  int rate = 0, L = 0, M = 0, K = 0;
  int taps() const { return 2 * K; }
  long long entries() const { return (long long)L * taps(); }
};

inline int gcd_int(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

// modified Bessel function of the first kind, order 0: the power series sum ((x / 2)^2k / (k!)^2), every term positive
inline double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// the filter of `rate`, or false with the reason in err (16000 included: L = M = 1; callers treat it as the identity)
inline bool plan(int rate, Filter& f, std::string& err) {
  if (rate < kMinRate || rate > kMaxRate) {
    err = "sample rate " + std::to_string(rate) + " Hz is outside " + std::to_string(kMinRate) + " .. " + std::to_string(kMaxRate) + " Hz";
    return false;
  }
  const int g = gcd_int(rate, kTargetRate);
  f.rate = rate; f.L = kTargetRate / g; f.M = rate / g;
  const double c = kRolloff * std::min(1.0, (double)f.L / (double)f.M);
  const double W = (double)kZ / c;
  f.K = (int)std::ceil(W);
  if (f.entries() > kMaxTable) {
    err = "sample rate " + std::to_string(rate) + " Hz needs a filter table of " + std::to_string(f.entries()) + " entries (" +
          std::to_string(f.L) + " phases): more than " + std::to_string(kMaxTable);
    return false;
  }
  return true;
}

// n_out = ceil(n L / M) for a clip of n samples at `rate` (n itself at 16000 Hz); -1 with the reason in err when refused
inline long long resampled_length(long long n, int rate, std::string& err) {
  Filter f;
  if (!plan(rate, f, err)) return -1;
  if (n < 0 || n > kMaxSamples) { err = "clip of " + std::to_string(n) + " samples: more than 2^29 (or negative)"; return -1; }
  const long long n_out = rate == kTargetRate ? n : (n * f.L + f.M - 1) / f.M;
  if (n_out > kMaxSamples) {
    err = "clip of " + std::to_string(n) + " samples at " + std::to_string(rate) + " Hz: more than 2^29 samples at 16000 Hz";
    return -1;
  }
  return n_out;
}

// h(tau) in float64, in this operation order (tests/resample_reference.py states the same one)
inline double tap(double tau, double c, double W, double inv_i0_beta) {
  if (!(std::fabs(tau) < W)) return 0.0;
  const double x = c * tau;
  const double px = M_PI * x;
  const double sinc = x == 0.0 ? 1.0 : std::sin(px) / px;
  const double u = tau / W;
  return c * sinc * (bessel_i0(kBeta * std::sqrt(1.0 - u * u)) * inv_i0_beta);
}

// H [L][T], float64 formula rounded once to float32
inline void build_table(const Filter& f, float* H) {
  const double c = kRolloff * std::min(1.0, (double)f.L / (double)f.M);
  const double W = (double)kZ / c;
  const double inv = 1.0 / bessel_i0(kBeta);
  const int T = f.taps();
  for (int r = 0; r < f.L; ++r)
    for (int i = 0; i < T; ++i) H[(size_t)r * T + i] = (float)tap((double)(i - f.K + 1) - (double)r / (double)f.L, c, W, inv);
}

inline std::vector<float> build_table(const Filter& f) {
  std::vector<float> H((size_t)f.entries());
  build_table(f, H.data());
  return H;
}

}  // namespace resample
}  // namespace axw
