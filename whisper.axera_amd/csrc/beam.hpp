// beam.hpp — the host side of beam search (DESIGN.md "Beam search"): what leaves a beam decode, and the finalisation (openai-whisper's
// BeamSearchDecoder.finalize + MaximumLikelihoodRanker without length penalty). Host only, dtype-independent: api.cpp
// (AX_WHISPER_BeamFinalize) and both builds of engine_beam.cpp use it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

namespace axw {

constexpr int kBeamSizeMax = 8;

// the state of `clips` clips after the loop, K = beam: per-slot / per-rank arrays [clips * K], histories and pool ids with row stride
// `stride`, n = the histories' length
struct BeamState {
  int clips, beam, n, stride;
  const int32_t* hist;                        // [clips * K][stride] by slot
  const float* S; const int* slot;            // by rank
  const int* pool_n;                          // [clips]
  const int32_t* pool_ids; const int* pool_len; const float* pool_score;  // [clips * K][stride] / [clips * K]
};
// every array may be null; rec_*: all records of every clip (the pool, then the fill), [clips * K] entries, n_rec [clips]
struct BeamResult {
  int32_t* ids; int* n_ids;                   // the winner: [clips][stride], [clips]
  float *sum_logprob, *avg_logprob; int* ended_eot;  // [clips]
  int32_t* rec_ids; int* rec_len; float* rec_score; int* rec_pool; int* n_rec; int* winner;
};

// While a clip's pool holds fewer than K records its live ranks are appended in rank order as (history, S); the winner is the first
// record with the largest score / max(len, 1). A clip without any record: no ids, -inf.
inline void beam_finalize(const BeamState& st, const BeamResult& out) {
  const int K = st.beam;
  for (int c = 0; c < st.clips; ++c) {
    const int r0 = c * K;
    const int32_t* rid[kBeamSizeMax];
    int rlen[kBeamSizeMax], rpool[kBeamSizeMax];
    float rscore[kBeamSizeMax];
    int nrec = 0;
    for (int i = 0; i < std::min(st.pool_n[c], K); ++i, ++nrec) {
      rid[nrec] = st.pool_ids + (size_t)(r0 + i) * st.stride;
      rlen[nrec] = std::max(0, std::min(st.pool_len[r0 + i], st.stride)); rscore[nrec] = st.pool_score[r0 + i]; rpool[nrec] = 1;
    }
    for (int r = 0; r < K && nrec < K; ++r) {
      if (st.S[r0 + r] == -std::numeric_limits<float>::infinity()) continue;  // dead
      rid[nrec] = st.hist + (size_t)st.slot[r0 + r] * st.stride;
      rlen[nrec] = st.n; rscore[nrec] = st.S[r0 + r]; rpool[nrec] = 0;
      ++nrec;
    }
    int best = -1;
    double best_key = 0.0;
    for (int i = 0; i < nrec; ++i) {
      const double key = (double)rscore[i] / (double)std::max(rlen[i], 1);
      if (best < 0 || key > best_key) { best = i; best_key = key; }
    }
    for (int i = 0; i < nrec; ++i) {
      if (out.rec_ids) std::copy(rid[i], rid[i] + rlen[i], out.rec_ids + (size_t)(r0 + i) * st.stride);
      if (out.rec_len) out.rec_len[r0 + i] = rlen[i];
      if (out.rec_score) out.rec_score[r0 + i] = rscore[i];
      if (out.rec_pool) out.rec_pool[r0 + i] = rpool[i];
    }
    if (out.n_rec) out.n_rec[c] = nrec;
    if (out.winner) out.winner[c] = best;
    const float ninf = -std::numeric_limits<float>::infinity();
    if (out.ids && best >= 0) std::copy(rid[best], rid[best] + rlen[best], out.ids + (size_t)c * st.stride);
    if (out.n_ids) out.n_ids[c] = best >= 0 ? rlen[best] : 0;
    if (out.sum_logprob) out.sum_logprob[c] = best >= 0 ? rscore[best] : ninf;
    if (out.avg_logprob) out.avg_logprob[c] = best >= 0 ? (float)((double)rscore[best] / (double)(rlen[best] + 1)) : ninf;  // openai-whisper: sum / (len + 1)
    if (out.ended_eot) out.ended_eot[c] = best >= 0 ? rpool[best] : 0;
  }
}

}  // namespace axw
