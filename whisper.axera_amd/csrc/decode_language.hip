// decode_language.hip — language detection (DESIGN.md "Language and task per clip"): openai-whisper's detect_language on the final
// residual row of the position that fed sot. Only the n_lang (99 or 100) language rows of the tied embedding are read — 152 KB at
// Whisper-small, 256 KB at turbo, shared by all clips — instead of the whole vocabulary through the logits launch.
//
// language_detect_kernel: one workgroup of four waves per detecting clip.
//   1. the final LayerNorm of the clip's row in fp32, the arithmetic of the GEMV family's PRO_LAYERNORM prologue (decode_gemv.hip:
//      prologue_layernorm — element tid + 256 e per thread, the mean, then the squares of the centred values, two block reductions),
//      the normalised row into LDS;
//   2. wave w takes languages w, w + 4, ... (four of them at a time, so that their row reads overlap): a lane reads 16-byte pieces
//      of the embedding row (8 weights), fp32 fused multiply-adds against the LDS row, one wave reduction per language; the n_lang
//      logits go to LDS;
//   3. wave 0: the first maximum in file order (NaN never wins) and logsumexp over the entries that are not NaN;
//      lang_logprob[j] = lang_logit[j] - logsumexp, -inf for NaN entries. Nothing finite: the handle's language, every value -inf.
//   4. with a context table: ctx[lang_row[c]] = lang_tokens[index], so the prefill pass that follows reads the detected language
//      from device memory (no host round trip between detection and the prefill of [..., sot, language]).
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

__global__ __launch_bounds__(256) void language_detect_kernel(LangDetectParams p) {
  __shared__ __attribute__((aligned(16))) float act[kLangMaxD];
  __shared__ float red[8];
  __shared__ float s_logit[kLangMax];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, K = p.d_model, n_lang = p.n_lang;
  const float* x = p.x + (long)(p.x_row ? p.x_row[c] : c) * K;

  // ---- 1. LayerNorm (prologue_layernorm<1>'s arithmetic)
  constexpr int MAXE = kLangMaxD / 256;
  float v[MAXE], g[MAXE], be[MAXE];
#pragma unroll
  for (int e = 0; e < MAXE; ++e) {
    const int i = tid + 256 * e;
    g[e] = i < K ? p.ln_w[i] : 0.f;
    be[e] = i < K ? p.ln_b[i] : 0.f;
    v[e] = i < K ? x[i] : 0.f;
  }
  float s1 = 0.f;
#pragma unroll
  for (int e = 0; e < MAXE; ++e) s1 += v[e];
  s1 = wave_sum(s1);
  if (lane == 0) red[wave * 2] = s1;
  __syncthreads();
  float t1 = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) t1 += red[w * 2];
  const float mean = t1 / K;
  float s2 = 0.f;
#pragma unroll
  for (int e = 0; e < MAXE; ++e) {
    const float t = tid + 256 * e < K ? v[e] - mean : 0.f;
    s2 += t * t;
  }
  s2 = wave_sum(s2);
  if (lane == 0) red[wave * 2 + 1] = s2;
  __syncthreads();
  float t2 = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) t2 += red[w * 2 + 1];
  const float rstd = rsqrtf(t2 / K + 1e-5f);
#pragma unroll
  for (int e = 0; e < MAXE; ++e) {
    const int i = tid + 256 * e;
    if (i < K) act[i] = (v[e] - mean) * rstd * g[e] + be[e];
  }
  __syncthreads();

  // ---- 2. the language rows, four of a wave's languages at a time: their row reads are independent, so four 16-byte loads per
  // lane are in flight where one language after the other would be a chain of n_lang / 4 dependent memory round trips
  const int n_piece = K >> 3;  // 16-byte pieces of a row
  for (int j = wave; j < n_lang; j += 16) {
    const h16* wrow[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wrow[u] = p.tok_emb + (long)p.lang_tokens[min(j + 4 * u, n_lang - 1)] * K;  // (beyond the list: a valid row, its result dropped)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < n_piece; i += 64) {
      u32x4 w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const u32x4*>(wrow[u] + i * 8);
      const float4 a0 = *reinterpret_cast<const float4*>(act + i * 8);
      const float4 a1 = *reinterpret_cast<const float4*>(act + i * 8 + 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = fmaf(h16lo(w[u][0]), a0.x, acc[u]);
        acc[u] = fmaf(h16hi(w[u][0]), a0.y, acc[u]);
        acc[u] = fmaf(h16lo(w[u][1]), a0.z, acc[u]);
        acc[u] = fmaf(h16hi(w[u][1]), a0.w, acc[u]);
        acc[u] = fmaf(h16lo(w[u][2]), a1.x, acc[u]);
        acc[u] = fmaf(h16hi(w[u][2]), a1.y, acc[u]);
        acc[u] = fmaf(h16lo(w[u][3]), a1.z, acc[u]);
        acc[u] = fmaf(h16hi(w[u][3]), a1.w, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float y = wave_sum(acc[u]);
      if (lane == 0 && j + 4 * u < n_lang) s_logit[j + 4 * u] = y;
    }
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- 3. first maximum and logsumexp: lane l holds languages l and l + 64
  const int j0 = lane, j1 = lane + 64;
  const float x0 = j0 < n_lang ? s_logit[j0] : NAN, x1 = j1 < n_lang ? s_logit[j1] : NAN;
  float m = -INFINITY;
  int idx = 0x7fffffff;
  argmax_take(m, idx, x0, j0);  // (a NaN compares false: never taken)
  argmax_take(m, idx, x1, j1);
  wave_argmax(m, idx);
  // nothing finite (every entry NaN, -inf or +inf): the handle's language, as the definition has it
  const float n_finite = wave_sum((fabsf(x0) < INFINITY ? 1.f : 0.f) + (fabsf(x1) < INFINITY ? 1.f : 0.f));
  const bool none = !(n_finite > 0.f) || idx >= n_lang;
  float lp0, lp1;
  if (none) {
    idx = p.fallback_index;
    lp0 = lp1 = -INFINITY;
  } else if (m == INFINITY) {  // the maxima share the whole mass
    lp0 = x0 == INFINITY ? 0.f : -INFINITY;
    lp1 = x1 == INFINITY ? 0.f : -INFINITY;
  } else {
    float s = (x0 == x0 ? expf(x0 - m) : 0.f) + (x1 == x1 ? expf(x1 - m) : 0.f);
    s = wave_sum(s);
    const float lse = m + logf(s);
    lp0 = x0 == x0 ? x0 - lse : -INFINITY;
    lp1 = x1 == x1 ? x1 - lse : -INFINITY;
  }
  if (j0 < n_lang) {
    if (p.lang_logit) p.lang_logit[(long)c * n_lang + j0] = x0;
    p.lang_logprob[(long)c * n_lang + j0] = lp0;
  }
  if (j1 < n_lang) {
    if (p.lang_logit) p.lang_logit[(long)c * n_lang + j1] = x1;
    p.lang_logprob[(long)c * n_lang + j1] = lp1;
  }
  if (lane == 0) {
    p.lang_index[c] = idx;
    if (p.ctx) p.ctx[p.lang_row[c]] = p.lang_tokens[idx];
  }
}

void launch_language_detect(const LangDetectParams& p, hipStream_t s) {
  if (p.n_clips < 1) return;
  if (p.d_model < 8 || p.d_model % 8 != 0 || p.d_model > kLangMaxD || p.n_lang < 1 || p.n_lang > kLangMax || p.fallback_index < 0 ||
      p.fallback_index >= p.n_lang || !p.lang_logprob || !p.lang_index || (p.ctx && !p.lang_row)) {
    fprintf(stderr, "[ax_whisper] launch_language_detect: unsupported d_model %d / n_lang %d\n", p.d_model, p.n_lang);
    abort();  // fail loudly: there is no fallback path
  }
  hipLaunchKernelGGL(language_detect_kernel, dim3(p.n_clips), dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
