// decode_beam.hip — beam search between the logits dump and advance_kernel (DESIGN.md "Beam search"): every hypothesis is a slot of
// the launch-per-phase step, and three launches per step turn the slots' dumped rows into the next step's hypotheses.
//
//   beam_candidates_kernel  one workgroup per slot: the rules of decode_timestamps.hip on the slot's row and history, then the M = K + 1
//                           best ids of the final allowed set with their log-probabilities
//   beam_select_kernel      one wave per clip: orders the clip's <= K * M candidates, walks them as openai-whisper's
//                           BeamSearchDecoder.update does, and writes the new ranks, the finished pool and the reorder's source map
//   beam_reorder_kernel     copies history and self-attention cache of every slot whose hypothesis came from another slot
//   beam_spread_cross_kernel  before the loop: the cross K/V of a clip into the K slots of its group
//
// The three step kernels run one after the other on one stream and never communicate inside a launch. The rules themselves are
// decode_rules.hpp's; the candidates kernel's loops over the row are its own (they feed sorted lists).
#include "decode_rules.hpp"

namespace axw {
inline namespace AXW_NS {

namespace {

constexpr int kM = kBeamMaxCand;  // list length: every M <= 9 is served by the same fully unrolled lists
constexpr int kNoId = 0x7fffffff;

// A thread's sorted top-kM list: value descending, and among equal values the id that came first (a thread meets its ids in
// ascending order, so that is the lower id). Static indices only: the arrays live in registers.
struct TopList {
  float v[kM];
  int i[kM];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < kM; ++j) { v[j] = -INFINITY; i[j] = kNoId; }
  }
  // NaN and -inf never enter (neither compares greater than the -inf the list starts with)
  __device__ __forceinline__ void push(float x, int id) {
    if (!(x > v[kM - 1])) return;
    v[kM - 1] = x; i[kM - 1] = id;
#pragma unroll
    for (int j = kM - 1; j > 0; --j) {
      const bool up = v[j] > v[j - 1];  // strict: never past an equal value that came earlier
      const float tv = v[j - 1];
      const int ti = i[j - 1];
      v[j - 1] = up ? v[j] : tv; i[j - 1] = up ? i[j] : ti;
      v[j] = up ? tv : v[j];     i[j] = up ? ti : i[j];
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j < kM - 1; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
    v[kM - 1] = -INFINITY; i[kM - 1] = kNoId;
  }
};

// the wave's M best (value descending, lowest id on ties) -> out_v / out_i [M] in LDS, by M rounds of wave_argmax over the heads
__device__ __forceinline__ void wave_top(TopList& l, int M, float* out_v, int* out_i, int lane) {
  for (int r = 0; r < M; ++r) {
    float bv = l.v[0];
    int bi = l.i[0];
    wave_argmax(bv, bi);
    if (bi != kNoId && bi == l.i[0]) l.pop();  // ids are unique over the wave: exactly one lane owns the winner
    if (lane == 0) { out_v[r] = bv; out_i[r] = bi; }
  }
}

}  // namespace

__global__ __launch_bounds__(256) void beam_candidates_kernel(BeamCandParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int E = p.eot, M = p.n_cand_max;
  // dead hypotheses and frozen clips propose nothing
  if ((p.slot_score && p.slot_score[b] == -INFINITY) || (p.complete && p.complete[b / p.beam])) {
    if (tid == 0) p.n_cand[b] = 0;
    return;
  }
  // ---- the slot's history: ids sampled so far (prefix excluded)
  const int n = min(max(p.n_hist ? p.n_hist[b] : p.n, 0), p.hist_stride);
  const AllowedSets a = allowed_sets(p.hist + (long)b * p.hist_stride, n, p.ts_begin, E, p.n_vocab);

  const float* row = p.logits + (long)b * p.stride;
  float tv = -INFINITY;                    // best unmasked id below T (rule 5's right-hand side)
  float m = -INFINITY, s = 0.f;            // online logsumexp over the unmasked timestamps
  float mt = -INFINITY, st = 0.f;          // ... over the unmasked text ids and eot
  TopList lt, ls;                          // text + eot / timestamps: rule 5 is only known after the reduction
  lt.clear();
  ls.clear();
  for (int c = (a.text_begin >> 2) + tid; 4 * c < a.text_end; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    const unsigned sup = p.suppress ? suppress_bits4(p.suppress, c) : 0u;  // (measured: this loop loses nothing to the test inside it)
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      x[e] = (text_id_on(a, i, E) && !suppressed(sup, e) && v[e] == v[e]) ? v[e] : -INFINITY;
      tv = fmaxf(tv, x[e]);
      lt.push(x[e], i);
    }
    lse_add4(mt, st, x[0], x[1], x[2], x[3]);
  }
  for (int c = (a.ts_lo >> 2) + tid; 4 * c < a.ts_hi; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * c + e;
      x[e] = (timestamp_on(a, i) && v[e] == v[e]) ? v[e] : -INFINITY;
      ls.push(x[e], i);
    }
    lse_add4(m, s, x[0], x[1], x[2], x[3]);
  }
  // ---- reductions: value pairs merged in a fixed order (lanes by xor butterfly, then waves 0..3)
  tv = wave_max(tv);
  lse_wave_reduce(m, s);
  lse_wave_reduce(mt, st);
  // lists 0..3: the waves' text lists, 4..7: their timestamp lists
  __shared__ float s_tv[4], s_m[4], s_s[4], s_mt[4], s_st[4];
  __shared__ float s_lv[8][kM];
  __shared__ int s_li[8][kM];
  // (the waves' values go to LDS before the list rounds and thread 0 reads its own back: nothing but the lists is live across the
  // rounds, where the register count of this kernel peaks)
  if (lane == 0) { s_tv[wave] = tv; s_m[wave] = m; s_s[wave] = s; s_mt[wave] = mt; s_st[wave] = st; }
  wave_top(lt, M, s_lv[wave], s_li[wave], lane);
  wave_top(ls, M, s_lv[4 + wave], s_li[4 + wave], lane);
  __syncthreads();
  if (tid == 0) {
    tv = s_tv[0]; m = s_m[0]; s = s_s[0]; mt = s_mt[0]; st = s_st[0];
    for (int w = 1; w < 4; ++w) {
      tv = fmaxf(tv, s_tv[w]);
      lse_merge(m, s, s_m[w], s_s[w]);
      lse_merge(mt, st, s_mt[w], s_st[w]);
    }
    const bool rule5 = rule5_fires(m, s, tv);  // A = the timestamps alone
    final_set_merge(rule5, m, s, mt, st);
    // merge of the lists that feed the result, heads compared in the fixed order 0..7 (lowest id on equal values)
    int hp[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) hp[w] = 0;
    int count = 0;
    for (int r = 0; r < M; ++r) {
      float bv = -INFINITY;
      int bi = kNoId, bw = -1;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        if (w < 4 && rule5) continue;
        if (hp[w] >= M) continue;
        const float v = s_lv[w][hp[w]];
        const int i = s_li[w][hp[w]];
        if (i != kNoId && (bw < 0 || v > bv || (v == bv && i < bi))) { bv = v; bi = i; bw = w; }
      }
      if (bw < 0) break;
#pragma unroll
      for (int w = 0; w < 8; ++w)
        if (w == bw) ++hp[w];
      p.cand_id[(long)b * M + r] = bi;
      p.cand_logprob[(long)b * M + r] = logprob_of(bv, m, s);
      ++count;
    }
    for (int r = count; r < M; ++r) { p.cand_id[(long)b * M + r] = E; p.cand_logprob[(long)b * M + r] = -INFINITY; }
    p.n_cand[b] = count;
  }
}

// One wave per clip. e = rank * M + position numbers the clip's candidates in (parent rank, position) order, so "beats" is
// (greater score) or (equal score and lower e): the order of a stable descending sort over openai-whisper's insertion order.
__global__ __launch_bounds__(64) void beam_select_kernel(BeamSelectParams p) {
  constexpr int kMaxE = kBeamMax * kBeamMaxCand;  // 72
  const int lane = threadIdx.x;
  const int clip = blockIdx.x;
  const int K = p.beam, M = K + 1, E = p.eot, n = p.n;
  const int r0 = clip * K;  // first rank / slot of the clip's group
  if (p.complete[clip]) {   // frozen: nothing of it changes; the reorder launch leaves its slots alone
    if (lane < K) {
      p.src[r0 + lane] = r0 + lane;
      p.slot_score[p.slot[r0 + lane]] = p.S[r0 + lane];  // (by slot what S is by rank, for callers that hand in no slot_score)
    }
    return;
  }
  __shared__ float s_score[kMaxE];
  __shared__ int s_tok[kMaxE];
  __shared__ int s_sorted[kMaxE];  // walk position -> e
  __shared__ float s_S[kBeamMax];
  __shared__ int s_slot[kBeamMax];         // old rank -> slot (global)
  __shared__ int s_new_parent[kBeamMax];   // new rank -> old rank
  __shared__ float s_new_S[kBeamMax];
  __shared__ int s_new_tok[kBeamMax];
  __shared__ int s_new_slot[kBeamMax];
  __shared__ int s_kept[kBeamMax];         // local slot -> new rank that stays there, or -1
  __shared__ int s_fin_parent[kBeamMax];   // newly finished records in walk order: the parent's old rank, the score
  __shared__ float s_fin_score[kBeamMax];
  __shared__ int s_counts[3];              // candidates, live ranks after the walk, newly finished records
  if (lane < K) { s_S[lane] = p.S[r0 + lane]; s_slot[lane] = p.slot[r0 + lane]; }
  __syncthreads();
  // ---- scores
  const int nE = K * M;
  for (int e = lane; e < kMaxE; e += 64) {
    float sc = 0.f;
    int tok = -1;  // -1: no candidate here
    if (e < nE) {
      const int j = e / M, q = e - j * M;
      const int slot = s_slot[j];
      if (s_S[j] != -INFINITY && q < p.n_cand[slot]) {
        sc = s_S[j] + p.cand_logprob[(long)slot * M + q];  // the float32 sum of the contract
        tok = p.cand_id[(long)slot * M + q];
      }
    }
    s_score[e] = sc;
    s_tok[e] = tok;
  }
  __syncthreads();
  // ---- order: a candidate's walk position is the number of candidates that beat it
  int total = 0;
  for (int e = lane; e < kMaxE; e += 64) {
    if (e >= nE || s_tok[e] < 0) continue;
    const float sc = s_score[e];
    int pos = 0;
    for (int f = 0; f < nE; ++f)
      if (s_tok[f] >= 0 && (s_score[f] > sc || (s_score[f] == sc && f < e))) ++pos;
    s_sorted[pos] = e;
  }
  for (int f = 0; f < nE; ++f) total += s_tok[f] >= 0 ? 1 : 0;
  __syncthreads();
  // ---- walk by prefix counts: position w holds a non-eot candidate that becomes rank (non-eot before w) while that is < K;
  // an eot candidate with fewer than K non-eot before it is newly finished, the (eot before w)-th of this step
  for (int w = lane; w < total; w += 64) {
    const int e = s_sorted[w];
    int before = 0, eots = 0;
    for (int u = 0; u < w; ++u) {
      const bool is_eot = s_tok[s_sorted[u]] == E;
      before += is_eot ? 0 : 1;
      eots += is_eot ? 1 : 0;
    }
    if (before >= K) continue;  // behind the stop
    if (s_tok[e] != E) {
      s_new_parent[before] = e / M; s_new_S[before] = s_score[e]; s_new_tok[before] = s_tok[e];
    } else if (eots < K) {  // (more than K can never be appended)
      s_fin_parent[eots] = e / M; s_fin_score[eots] = s_score[e];
    }
  }
  if (lane == 0) {
    int live = 0, fin = 0;
    for (int w = 0; w < total && live < K; ++w) {
      if (s_tok[s_sorted[w]] == E) ++fin; else ++live;
    }
    s_counts[0] = total; s_counts[1] = live; s_counts[2] = min(fin, K);
  }
  __syncthreads();
  const int live = s_counts[1], fin = s_counts[2];
  // ---- slots: a surviving parent's best child stays in the parent's slot; the other children, then the dead ranks, take the
  // slots of parents without children in ascending slot order. Ranks decide, never slot numbers.
  if (lane == 0) {
    for (int t = 0; t < K; ++t) s_kept[t] = -1;
    for (int r = 0; r < K; ++r) {
      s_new_slot[r] = -1;
      if (r >= live) { s_new_S[r] = -INFINITY; s_new_tok[r] = E; s_new_parent[r] = -1; continue; }
      const int t = s_slot[s_new_parent[r]] - r0;
      if (s_kept[t] < 0) { s_kept[t] = r; s_new_slot[r] = r0 + t; }
    }
    int t = 0;
    for (int r = 0; r < K; ++r) {
      if (s_new_slot[r] >= 0) continue;
      while (s_kept[t] >= 0) ++t;
      s_kept[t] = r;
      s_new_slot[r] = r0 + t;
    }
  }
  __syncthreads();
  // ---- the pool: newly finished records in walk order while it holds fewer than K (ids: the parent's history [0, n))
  const int pool0 = p.pool_n[clip];
  const int n_app = min(fin, K - pool0);
  for (int a = 0; a < n_app; ++a) {
    const int* from = p.hist + (long)s_slot[s_fin_parent[a]] * p.hist_stride;
    int* to = p.pool_ids + ((long)r0 + pool0 + a) * p.hist_stride;
    for (int i = lane; i < n; i += 64) to[i] = from[i];
    if (lane == 0) { p.pool_len[r0 + pool0 + a] = n; p.pool_score[r0 + pool0 + a] = s_fin_score[a]; }
  }
  // ---- the new ranks
  if (lane < K) {
    const int r = lane, slot = s_new_slot[r];
    p.S[r0 + r] = s_new_S[r];
    p.slot[r0 + r] = slot;
    p.slot_score[slot] = s_new_S[r];
    p.hist[(long)slot * p.hist_stride + n] = s_new_tok[r];  // index n: nobody reads it in this launch
    p.src[slot] = r < live ? s_slot[s_new_parent[r]] : slot;
  }
  if (lane == 0) {
    p.pool_n[clip] = pool0 + n_app;
    if (pool0 + n_app >= K || live == 0) {
      p.complete[clip] = 1;
      atomicAdd(p.n_complete, 1);
    }
  }
}

// grid (slots, n_layer * n_head): the whole 64-key blocks that cover keys [0, off] of one (slot, layer, head), K and V alike
// (decode_layout.hpp: block b of a head is elements [b, b + 1) * kKvBlockElems in both layouts); workgroups of y == 0 also the
// history [0, n). No slot is both read and written in one launch (beam_select_kernel's slot assignment).
__global__ __launch_bounds__(256) void beam_reorder_kernel(BeamReorderParams p) {
  const int slot = blockIdx.x, from = p.src[slot];
  if (from == slot) return;
  const int tid = threadIdx.x;
  if (blockIdx.y == 0) {
    const int* hs = p.hist + (long)from * p.hist_stride;
    int* hd = p.hist + (long)slot * p.hist_stride;
    for (int i = tid; i < p.n; i += 256) hd[i] = hs[i];
  }
  const int l = blockIdx.y / p.n_head, h = blockIdx.y - l * p.n_head;
  const int blocks = min(p.off / layout::kKvBlockKeys + 1, p.n_ctx_pad / layout::kKvBlockKeys);
  const long head = layout::kv_head_elems(p.n_ctx_pad);
  const long src = ((long)l * p.cap + from) * p.kv_batch_stride + h * head;
  const long dst = ((long)l * p.cap + slot) * p.kv_batch_stride + h * head;
  const int pieces = blocks * (layout::kKvBlockElems / 8);  // 16 bytes = 8 elements
  const u32x4* ks = reinterpret_cast<const u32x4*>(p.k + src);
  const u32x4* vs = reinterpret_cast<const u32x4*>(p.v + src);
  u32x4* kd = reinterpret_cast<u32x4*>(p.k + dst);
  u32x4* vd = reinterpret_cast<u32x4*>(p.v + dst);
  for (int i = tid; i < pieces; i += 256) {
    const u32x4 a = ks[i], c = vs[i];
    kd[i] = a;
    vd[i] = c;
  }
}

// grid (destinations, n_layer, 32): slot src of every layer -> slots dst0 .. dst0 + n_dst - 1 (src itself skipped), K and V alike
__global__ __launch_bounds__(256) void beam_spread_cross_kernel(h16* k, h16* v, long layer_stride, long slot_elems, int src, int dst0) {
  const int dst = dst0 + blockIdx.x;
  if (dst == src) return;
  const long base = (long)blockIdx.y * layer_stride;
  const u32x4* ks = reinterpret_cast<const u32x4*>(k + base + src * slot_elems);
  const u32x4* vs = reinterpret_cast<const u32x4*>(v + base + src * slot_elems);
  u32x4* kd = reinterpret_cast<u32x4*>(k + base + dst * slot_elems);
  u32x4* vd = reinterpret_cast<u32x4*>(v + base + dst * slot_elems);
  const long pieces = slot_elems / 8;
  for (long i = (long)blockIdx.z * 256 + threadIdx.x; i < pieces; i += 256L * gridDim.z) {
    const u32x4 a = ks[i], c = vs[i];
    kd[i] = a;
    vd[i] = c;
  }
}

void launch_beam_candidates(const BeamCandParams& p, hipStream_t s) {
  if (p.stride % 4 != 0 || p.stride < p.n_vocab || p.ts_begin <= p.eot || p.ts_begin > p.n_vocab || p.n_cand_max < 1 || p.n_cand_max > kBeamMaxCand ||
      p.beam < 1 || !p.hist || !p.cand_id || !p.cand_logprob || !p.n_cand) {
    fprintf(stderr, "[ax_whisper] launch_beam_candidates: unsupported row stride %ld / ids (eot %d, T %d, vocab %d) / %d candidates\n", p.stride,
            p.eot, p.ts_begin, p.n_vocab, p.n_cand_max);
    abort();
  }
  hipLaunchKernelGGL(beam_candidates_kernel, dim3(p.n_slots), dim3(256), 0, s, p);
}

void launch_beam_select(const BeamSelectParams& p, hipStream_t s) {
  if (p.beam < 1 || p.beam > kBeamMax || p.n < 0 || p.n >= p.hist_stride) {
    fprintf(stderr, "[ax_whisper] launch_beam_select: beam %d / history length %d of %d unsupported\n", p.beam, p.n, p.hist_stride);
    abort();
  }
  hipLaunchKernelGGL(beam_select_kernel, dim3(p.n_clips), dim3(64), 0, s, p);
}

void launch_beam_reorder(const BeamReorderParams& p, hipStream_t s) {
  if (p.n_ctx_pad % layout::kKvBlockKeys != 0 || p.off < 0 || p.n < 0 || p.n > p.hist_stride || p.n_slots > p.cap) {
    fprintf(stderr, "[ax_whisper] launch_beam_reorder: offset %d / history length %d / context %d unsupported\n", p.off, p.n, p.n_ctx_pad);
    abort();
  }
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(p.n_slots, p.n_layer * p.n_head), dim3(256), 0, s, p);
}

void launch_beam_spread_cross(h16* k, h16* v, long layer_stride, long slot_elems, int n_layer, int src, int dst0, int n_dst, hipStream_t s) {
  if (slot_elems % 8 != 0 || n_dst < 1) {
    fprintf(stderr, "[ax_whisper] launch_beam_spread_cross: unsupported slot size %ld\n", slot_elems);
    abort();
  }
  hipLaunchKernelGGL(beam_spread_cross_kernel, dim3(n_dst, n_layer, 32), dim3(256), 0, s, k, v, layer_stride, slot_elems, src, dst0);
}

}  // inline namespace AXW_NS
}  // namespace axw
