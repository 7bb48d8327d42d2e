// decode_persistent.hip — the whole greedy decode loop of ONE clip as a single persistent launch (gfx950).
//
// Replaces, for batch 1, the per-token sequence Whisper::run_decoder (cpp/src/Whisper.cpp:290-346) + argmax (:42-45)
// + the host loop (:207-222) = the decoder graph TextDecoderTensorCache.forward (model_convert/export_onnx.py:312-387)
// with its attention (:103-150, :221-230). Same arithmetic as the launch-per-phase path (decode_gemv.hip,
// decoder.hip): h16 weights x fp32 activations with fp32 FMA, fp32 LayerNorm/softmax, h16 self/cross K/V.
//
// Why: at batch 1 a decoder step is a chain of ~100 dependent phases that each move only a few MB, so the chain is
// bound by per-phase latency, not by HBM. As separate graph nodes a phase costs ~4.4 us (kernel
// boundary + wave start + activation round trip + drain). Here one 1024-thread workgroup per CU stays resident for
// the whole utterance and the phases hand their outputs over INSIDE the launch:
//   * every output element travels as one 8-byte {tag, value} granule; a producer assembles its rows in LDS and ONE
//     wave stores them with ONE sc1 (write-through) instruction (a full 128-byte line), consumers poll pairs of
//     granules with 16-byte sc1 loads — the data is the flag, no fence, no separate barrier
//     (cdna_hip_programming.md §6 Guideline 16 form R2; tags = step * n_layer + layer + 1, never 0, buffers zeroed
//     before every launch);
//   * the waves of a workgroup have fixed ROLES: waves 0-7 ("pollers") gather granules, keep the residual stream in
//     registers and do LayerNorm; waves 8-15 ("compute") own the weight rows, the attention blocks and every
//     bulk load. Vector-memory results return to a wave in issue order, so a wave that polls must have no long load
//     in flight — with the roles split, a poll never queues behind a weight or K/V load, and the compute waves request
//     the rows of the NEXT phase right after publishing the current one, a whole hand-off ahead of their use;
//   * the self-attention K/V cache of one (layer, head) lives in the LDS of the workgroup that owns that head for
//     the whole utterance (448 keys x 64 x 2 x h16 = 112 KB): it never touches HBM. Workgroups that own no head
//     use the same LDS region to stage cross-attention K/V tiles by LDS-DMA one layer before their use;
//   * every workgroup keeps its own copy of the residual stream, so a LayerNorm needs no extra hand-off;
//   * the token feedback (argmax merge, SOT forcing, eot / context stop, embedding of the next token) is computed
//     redundantly by every workgroup from the gathered argmax partials: the loop never returns to the host.
// Every spin is bounded: a lane that waits too long raises a flag, its workgroup sets an error word and leaves; the
// others see the word (or time out themselves) and leave too, so the grid always drains. The host then falls back.
#include "decode_persistent_common.hpp"
#include "decode_persistent_rules.hpp"

namespace axw {
inline namespace AXW_NS {

// ---------------------------------------------------------------------------------------- query fold (round 5)
// A layer of the launch was eight dependent all-to-all hand-offs; three of them carried the self-attention output to the
// cross-attention units:   att -> [hop] -> out-projection rows -> y1 -> [hop] -> LayerNorm(x0 + y1) -> query rows -> [hop]
// The query is linear in everything but the LayerNorm statistics (export_onnx.py:221-230, 238-261):
//   cq_j = r (A0_j + (M a)_j + d_j - mu s_j) + c_j,    x1 = x0 + W_o a + b_o,  mu / r = mean / rstd of x1
//   A0 = W_cq (g . x0)   — needs only the layer's input: computed by the row producers WHILE self-attention runs
//   M  = W_cq diag(g) W_o (fp32, built once at load), d = W_cq (g . b_o), s = W_cq g, c = W_cq beta + b_cq
// so the 16-row producers of y1 also produce T = A0 + M a + d for the same 16 rows and the two sums of their x1 slice, and
// a cross-attention unit finishes its head's query from 64 T granules + 2 x (number of producers) statistics: the middle
// hop, the LayerNorm stage (two workgroup barriers in every workgroup) and the query-row phase are gone; y1 is added to
// the residual copies together with y2 (same order of additions: the stream is bit-identical to the unfolded launch).
// LayerNorm folded into the rows it feeds: W LN(x) + b = r (W (g . x) - mu s) + c with s = W g, c = W beta + b, so the pollers
// hand the compute waves g . x and the two sums behind ONE workgroup barrier instead of statistics, barrier, normalised
// vector, barrier; every compute wave derives mu and r from the eight partial sums itself.
__global__ void qfold_vec_kernel(const h16* __restrict__ wl, const float* __restrict__ fl, float* __restrict__ qf, int D) {
  const int l = blockIdx.y;
  const long DD = (long)D * D;
  const h16* WL = wl + (long)l * DecArena::w_stride(D);
  const float* F = fl + (long)l * DecArena::f_stride(D);
  float* out = qf + (long)l * qfold_stride(D) + DD;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < 3 * D) {
    const h16* w = WL + DecArena::W_QKV * DD + (long)j * D;
    const float *g = F + DecArena::F_ATTN_LN_W * D, *be = F + DecArena::F_ATTN_LN_B * D;
    double ss = 0.0, cc = 0.0;
    for (int i = 0; i < D; ++i) { const double wv = (double)(float)w[i]; ss += wv * (double)g[i]; cc += wv * (double)be[i]; }
    out[QF_SQKV * D + j] = (float)ss;
    out[QF_CQKV * D + j] = (float)(cc + (double)F[DecArena::F_B_QKV * D + j]);
  }
  if (j < 4 * D) {
    const h16* w = WL + DecArena::W_FC1 * DD + (long)j * D;
    const float *g = F + DecArena::F_MLP_LN_W * D, *be = F + DecArena::F_MLP_LN_B * D;
    double ss = 0.0, cc = 0.0;
    for (int i = 0; i < D; ++i) { const double wv = (double)(float)w[i]; ss += wv * (double)g[i]; cc += wv * (double)be[i]; }
    out[QF_SFC1 * D + j] = (float)ss;
    out[QF_CFC1 * D + j] = (float)(cc + (double)F[DecArena::F_B_FC1 * D + j]);
  }
}


// M = W_cq diag(g) W_o in double, one thread per element; d, s, c by the first D threads of block row 0
__global__ void qfold_build_kernel(const h16* __restrict__ wl, const float* __restrict__ fl, float* __restrict__ qf, int D) {
  const int l = blockIdx.z;
  const long DD = (long)D * D;
  const h16* wq = wl + (long)l * DecArena::w_stride(D) + DecArena::W_CQ * DD;
  const h16* wo = wl + (long)l * DecArena::w_stride(D) + DecArena::W_O * DD;
  const float* F = fl + (long)l * DecArena::f_stride(D);
  const float *g = F + DecArena::F_CROSS_LN_W * D, *be = F + DecArena::F_CROSS_LN_B * D, *bo = F + DecArena::F_B_O * D, *bq = F + DecArena::F_B_CQ * D;
  float* out = qf + (long)l * qfold_stride(D);
  const int k = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (k >= D) return;
  double acc = 0.0;
  for (int i = 0; i < D; ++i) acc += (double)(float)wq[(long)j * D + i] * (double)g[i] * (double)(float)wo[(long)i * D + k];
  out[(long)j * D + k] = (float)acc;
  if (k == 0) {
    double dd = 0.0, ss = 0.0, cc = 0.0;
    for (int i = 0; i < D; ++i) {
      const double w = (double)(float)wq[(long)j * D + i];
      dd += w * (double)g[i] * (double)bo[i];
      ss += w * (double)g[i];
      cc += w * (double)be[i];
    }
    out[DD + j] = (float)dd;
    out[DD + D + j] = (float)ss;
    out[DD + 2 * D + j] = (float)(cc + (double)bq[j]);
  }
}
void launch_qfold_build(const h16* wl, const float* fl, float* qf, int d_model, int n_layer, hipStream_t s) {
  qfold_build_kernel<<<dim3((d_model + 127) / 128, d_model, n_layer), 128, 0, s>>>(wl, fl, qf, d_model);
  qfold_vec_kernel<<<dim3((4 * d_model + 127) / 128, n_layer), 128, 0, s>>>(wl, fl, qf, d_model);
}
size_t qfold_floats(int d_model, int n_layer) { return (size_t)n_layer * (size_t)qfold_stride(d_model); }

// ---------------------------------------------------------------------------------------- the kernel
// d_model = 8*LD*CD (rows with K = d: LD lanes x CD 16-byte chunks), 4*d_model = 8*LF*CF.
// QF: the query fold above (d_model <= 768: the fp32 rows of M cost 2 * CD more registers per lane)
//
// Resident vocabulary rows (round 7). The vocabulary projection is the one phase of a step that is bound by bytes: every
// workgroup streams the same ~N / P rows of the tied embedding from HBM at every step, while its poller waves hold two floats
// of residual stream per lane and spin. So the pollers load the TAIL of the workgroup's range once per launch — kVocabRes<>
// passes of PL / LD rows in the lane layout of rows_load<LD, CD> — and compute those logits from their registers behind the
// final LayerNorm, with the same rows_dot<LD, CD> (same element order, same group_sum: every logit keeps its bits); the compute
// waves stream only the head of the range and compute wave 0 folds the pollers' eight candidates into the workgroup's pair
// (first max wins by index, so who computed a row cannot change the token). PersistParams::vocab_resident == 0: none.
// Passes per instantiation: what the pollers' registers hold without a spill. At d_model 768 a pass is 12 registers per lane and
// the poller loop itself needs ~50 of the 128: six passes (96 of a workgroup's ~203 rows); the seventh spills 8 registers, and
// the timeline build, which has a few registers less to give, keeps five. Rows wider than 3 chunks keep none.
template <int CD, bool PROF>
constexpr int kVocabRes = CD > 3 ? 0 : PROF ? 5 : 6;
//
// RULES = 1 (decode_persistent_rules.hpp): the launch of timestamp and scored mode. The prefix is [sot, language,
// transcribe]; both row loops of the vocabulary phase keep a RulesRec per lane under the step's allowed sets instead of one
// candidate; compute wave 0 folds the sixteen wave records and publishes the workgroup's eight words at O_REC with one store
// instruction; the pollers gather the P records in the round trip that carried the argmax pairs, and every workgroup decides the
// token with decode_rules.hpp's functions. The history's four values travel in registers. Scored mode (PersistParams::ts_logprob)
// also runs the vocabulary phase at step 0 over the whole row: the no-speech value. RULES = 0 compiles none of it.
template <int LD, int CD, int LF, int CF, bool PROF, bool QF, int RULES>
__global__ __launch_bounds__(PT) void decode_persistent_kernel(PersistParams p) {
  AXW_PERSIST_SHAPES
  // (the rules' row loop needs the registers of one resident pass: as many passes as the timeline build keeps)
  constexpr int NRES = kVocabRes<CD, PROF || RULES != 0>, VCAP = NRES * (PL / LD);  // resident passes, rows
  constexpr int XG = D, X0R = 2 * D, A0S = 3 * D;  // QF: act[XG..) = g_cross . x0, act[X0R..) = x0 (written with the QKV LayerNorm, read by
                                                  // the row producers), act[A0S + slot] = A0 of the slot's row (free until the partial records)
  AXW_PERSIST_LDS(4)  // red[2*NPW]: the stage's mean (QF: the statistics' shift), red[2*NPW + 1]: the shift the sums are relative to
  AXW_PERSIST_IDS
  const __amdgpu_buffer_rsrc_t GR = __builtin_amdgcn_make_buffer_rsrc((void*)p.gran, 0, p.gran_bytes, 0x27000);
  AXW_PERSIST_ROLES
  AXW_PERSIST_INIT
#define AXW_TL(IDX) \
  if (PROF && tl_on && (tid == 0 || tid == PL)) prof_acc[32 + (IDX)] = wall_clock64();
  int tok = AXW_COLD(sot)[0];
  int n_out = 0, n_done = 0, steps_run = 0;
  // steps whose logits are dropped (the prefix but its last id), and whether a step runs the vocabulary phase (scored rules: step 0
  // as well, the no-speech row). Macros: the plain instantiations keep their literals.
#define AXW_NSKIP (RULES ? AXW_COLD(n_prefix) - 1 : 3)
#define AXW_VOCAB_STEP(STEP) (RULES ? ((STEP) >= AXW_COLD(n_prefix) - 1 || ((STEP) == 0 && AXW_COLD(no_speech) != nullptr)) : (STEP) >= 3)
#define AXW_SKIP_STEP(STEP) (RULES ? !AXW_VOCAB_STEP(STEP) : (STEP) < 3)
  [[maybe_unused]] constexpr int O_REC = O_STAT + D;  // RULES: workgroup wg's record, granules O_REC + 8 wg ..+ 7
  [[maybe_unused]] unsigned *rec_c = nullptr, *rec_p = nullptr, *rec_g = nullptr, *sup = nullptr;
  [[maybe_unused]] RulesState hist{-1, false, false};
  if constexpr (RULES) {
    rec_c = reinterpret_cast<unsigned*>(prof_acc + 64) + 32;  // behind the plain carve-up (kRulesLdsBytes)
    rec_p = rec_c + NCW * kRecWords;
    rec_g = rec_p + NPW * kRecWords;
    sup = rec_g + NPW * 4;
    // the suppress mask's words over this workgroup's rows, once per launch (zeros without a set: one code path)
    if (tid < kRulesSupWords) {
      const unsigned N = (unsigned)AXW_COLD(n_vocab);
      const int wi = (int)(((unsigned)rwg * N / (unsigned)P) >> 5) + tid;
      const unsigned* mask = AXW_COLD(suppress);
      sup[tid] = (mask && wi <= (int)((N - 1) >> 5)) ? mask[wi] : 0u;
    }
    __syncthreads();
  }
  // RULES: what the row loops of `step` need; v0: the workgroup's first row
  [[maybe_unused]] auto rules_step = [&](int step, int v0) -> RulesStep {
    RulesStep q;
    const int T = AXW_COLD(ts_begin), skip = AXW_NSKIP;
    q.E = AXW_COLD(eot);
    q.no_speech_id = AXW_COLD(no_speech_id);
    q.w0 = v0 >> 5;
    q.whole = step < skip;
    q.a = allowed_sets_from_state(step - skip, hist.last_ts, hist.last_is_ts, hist.penult_is_ts, T, q.E, AXW_COLD(n_vocab));
    return q;
  };
  // RULES: where the step's row is dumped (teacher forcing), nullptr: nowhere
  [[maybe_unused]] auto rules_dump = [&](int step) -> float* {
    const int skip = AXW_NSKIP;
    if (step < skip) return AXW_COLD(logits0_dump);
    return AXW_COLD(logits_dump) ? AXW_COLD(logits_dump) + (long)(step - skip) * AXW_COLD(n_vocab) : nullptr;
  };

  if (poller) {
    // ======================================================================================= pollers
    float x[GD];        // residual stream, element tid + k*PL
    float lg[GD], lb[GD];
    float shift = 0.f;  // LayerNorm variance shift (previous mean): sums stay small without a second pass
    AXW_POLLER_PREFETCH
    // resident vocabulary rows: slot tid / LD keeps rows vb + slot (+ k * PL / LD) of [vb, v1) = the last min(VCAP, rows) of the
    // workgroup's range (RowSet::prefetch's even deal). Nothing of it is in flight when the first poll is issued.
    // Kept as single registers behind an opaque asm, not as the loads' 4-register tuples: tuples that live across the whole step
    // loop fragment the register file (spills from the 4th pass on), and rows the compiler can see through are unpacked to fp32
    // ONCE in front of the loop and kept that way — twice the registers.
    unsigned vres[NRES > 0 ? NRES : 1][4 * CD];
    auto vocab_tail = [&](int& v0, int& vb, int& v1) {
      const unsigned N = (unsigned)AXW_COLD(n_vocab);
      v0 = (int)((unsigned)rwg * N / (unsigned)P);
      v1 = (int)((unsigned)(rwg + 1) * N / (unsigned)P);
      vb = AXW_COLD(vocab_resident) ? (v1 - v0 > VCAP ? v1 - VCAP : v0) : v1;
    };
    if constexpr (NRES > 0) {  // (loaded with the switch off as well: a few rows once per launch, and no second code path)
      int v0, vb, v1;
      vocab_tail(v0, vb, v1);
      if (vb == v1) vb = v0;
#pragma unroll
      for (int k = 0; k < NRES; ++k) {
        const int row = vb + k * (PL / LD) + tid / LD;
        u32x4 w[CD];
        rows_load<LD, CD>(w, AXW_COLD(tok_emb), D, row < v1 ? row : v0, tid);
#pragma unroll
        for (int i = 0; i < 4 * CD; ++i) { vres[k][i] = w[i / 4][i % 4]; asm volatile("" : "+v"(vres[k][i])); }
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    }
    // the pairs of a d-wide vector that starts at granule `base`
#define AXW_PAIRS_D(BASE) [&](int j) { const int pr = tid + j * PL; return 2 * pr < D ? (BASE) + 2 * pr : -1; }

    // x += y, LayerNorm into act[0..D): two workgroup barriers
    // QF: the stage of a LayerNorm that is folded into its rows (QKV, mlp.0): g . x and the two sums, ONE barrier. The caller has
    // added the gathered update to x. Writing act before the barrier is safe: the update that was just gathered (or, in the first
    // layer, the barrier at the end of the previous step) lies behind every read of act by this workgroup's compute waves.
#define AXW_RAW_STAGE(FAIL, CODE, XGW)                                                      \
  {                                                                                          \
    float s1 = 0.f, s2 = 0.f;                                                                \
    _Pragma("unroll") for (int k = 0; k < GD; ++k) {                                         \
      const int i = el(k);                                                                   \
      if (i < D) {                                                                           \
        const float t = x[k] - shift;                                                        \
        s1 += t; s2 += t * t;                                                                \
        act[i] = x[k] * lg[k];                                                               \
        if (XGW) { act[XG + i] = x[k] * g2[k]; act[X0R + i] = x[k]; }                        \
      }                                                                                      \
    }                                                                                        \
    s1 = wsum(s1); s2 = wsum(s2);                                                            \
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = s1; red[2 * (tid >> 6) + 1] = s2; }         \
    if (tid == 0) red[2 * NPW + 1] = shift;                                                  \
    if (FAIL) ctl[0] = 1;                                                                    \
    AXW_BARRIER_CHECK(CODE)                                                                  \
    float t1 = 0.f;                                                                          \
    _Pragma("unroll") for (int w2 = 0; w2 < NPW; ++w2) t1 += red[2 * w2];                    \
    shift += t1 / D;                                                                         \
    if (tid == 0) red[2 * NPW] = shift;                                                      \
  }
#define AXW_LN_STAGE(Y, ADD, FAIL, CODE) AXW_LN_STAGE_X(Y, ADD, FAIL, CODE, false)
    // XGW (QF, row producers, QKV stage): also leave g_cross . x and x itself in act[XG..), act[X0R..) — behind the stage's
    // first barrier, when the compute waves have left the previous phase (mlp.2 reads all of act)
#define AXW_LN_STAGE_X(Y, ADD, FAIL, CODE, XGW)                                             \
  {                                                                                          \
    float s1 = 0.f, s2 = 0.f;                                                                \
    _Pragma("unroll") for (int k = 0; k < GD; ++k) {                                         \
      if (el(k) < D) {                                                                       \
        if (ADD) x[k] += __uint_as_float(Y[k]);                                              \
        const float t = x[k] - shift;                                                        \
        s1 += t; s2 += t * t;                                                                \
      }                                                                                      \
    }                                                                                        \
    s1 = wsum(s1); s2 = wsum(s2);                                                            \
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = s1; red[2 * (tid >> 6) + 1] = s2; }         \
    if (FAIL) ctl[0] = 1;                                                                    \
    AXW_BARRIER_CHECK(CODE)                                                                  \
    float t1 = 0.f, t2 = 0.f;                                                                \
    _Pragma("unroll") for (int w2 = 0; w2 < NPW; ++w2) { t1 += red[2 * w2]; t2 += red[2 * w2 + 1]; } \
    const float dm = t1 / D, var = fmaxf(t2 / D - dm * dm, 0.f);                             \
    const float mean = shift + dm, rstd = rsqrtf(var + 1e-5f);                               \
    if (QF && tid == 0) red[2 * NPW] = mean;                                                 \
    _Pragma("unroll") for (int k = 0; k < GD; ++k) {                                         \
      const int i = el(k);                                                                   \
      if (i < D) act[i] = (x[k] - mean) * rstd * lg[k] + lb[k];                              \
      if (QF && (XGW) && i < D) { act[XG + i] = x[k] * g2[k]; act[X0R + i] = x[k]; }         \
    }                                                                                        \
    shift = mean;                                                                            \
    wg_barrier();                                                                            \
  }

    for (int step = 0; step < p.total_steps; ++step) {
      AXW_EMBED(x, tok)
      ln_prefetch(p.fl + DecArena::F_ATTN_LN_W * D, p.fl + DecArena::F_ATTN_LN_B * D);

      for (int l = 0; l < L; ++l) {
        asm volatile("" : "+v"(tid));
        const bool tl_on = step == p.total_steps / 2 && l == L / 2;
        const float* FL = p.fl + (long)l * DecArena::f_stride(D);
        const unsigned tag = (unsigned)(step * L + l + 1);
        // ---- QKV
        {
          unsigned y[GD];
          bool fail = false;
          if (l > 0) fail = gather2<GPD>(GR, tag - 1, y, p.err, ctl, AXW_PAIRS_D(O_Y3));
          AXW_STAMP(0)
          AXW_TL(0)
          if constexpr (QF) {
            if (l > 0) {
#pragma unroll
              for (int k = 0; k < GD; ++k) if (el(k) < D) x[k] += __uint_as_float(y[k]);
            }
            AXW_RAW_STAGE(fail, 0x100 + l, in_o)
            ln_prefetch(FL + DecArena::F_MLP_LN_W * D, FL + DecArena::F_MLP_LN_B * D);
          } else {
            AXW_LN_STAGE_X(y, l > 0, fail, 0x100 + l, in_o)
            ln_prefetch(FL + DecArena::F_CROSS_LN_W * D, FL + DecArena::F_CROSS_LN_B * D);
          }
          AXW_STAMP(1)
          AXW_TL(1)
        }
        // ---- self-attention owner: collect q, k, v of the head; append k, v to the LDS cache
        if (l == sa_layer) {
          unsigned v[2];  // lanes 0-31: q, 32-63: k, 64-95: v of the head, two adjacent dims each
          const bool fail = gather2<1>(GR, tag, v, p.err, ctl, [&](int) { return tid < 96 ? O_QKV + (tid >> 5) * D + sa_head * 64 + 2 * (tid & 31) : -1; });
          if (tid < 32) {  // the query: dims 2 tid, 2 tid + 1 as one packed (hi, lo) pair
            unsigned hi, lo;
            h16split2(__uint_as_float(v[0]), __uint_as_float(v[1]), hi, lo);
            qs[tid] = hi;
            qs[32 + tid] = lo;
          } else if (tid < 96) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const int dd = 2 * (tid & 31) + e;
              const float val = __uint_as_float(v[e]);
              if (tid < 64)  // K row `step`, blocked [blk][d/8][key%64][8]
                sK[layout::k_index(step, dd)] = (h16)val;
              else           // V row `step`, TRANSPOSED per block: [blk][key%64 / 8][dim][8 keys]
                sV[layout::vt_index(step, dd)] = (h16)val;
            }
          }
          if (fail) ctl[0] = 1;
          AXW_STAMP(2)
          AXW_BARRIER_CHECK(0x200 + l)
          AXW_STAMP(3)
        }
        // ---- attention output projection
        if (in_o) {
          unsigned y[GD];
          const bool fail = gather2<GPD>(GR, tag, y, p.err, ctl, AXW_PAIRS_D(O_ATT));
#pragma unroll
          for (int k = 0; k < GD; ++k) { const int i = el(k); if (i < D) act[i] = __uint_as_float(y[k]); }
          if (fail) ctl[0] = 1;
          AXW_STAMP(4)
          AXW_TL(2)
          AXW_BARRIER_CHECK(0x300 + l)
        }
        // ---- cross-attention query
        if constexpr (!QF) {
          unsigned y[GD];
          const bool fail = gather2<GPD>(GR, tag, y, p.err, ctl, AXW_PAIRS_D(O_Y1));
          AXW_STAMP(5)
          AXW_TL(3)
          AXW_LN_STAGE(y, true, fail, 0x400 + l)
          ln_prefetch(FL + DecArena::F_MLP_LN_W * D, FL + DecArena::F_MLP_LN_B * D);
          AXW_STAMP(6)
          AXW_TL(4)
        }
        // ---- cross-attention unit: collect the head's query
        const int cu = ca_unit_of(step * L + l, NU, wg, NS);
        if (cu >= 0) {
          const int ca_head = cu / kCrossSplit;
          if constexpr (QF) {
            const bool fail = qfold_unit_query<D, NP_D>(GR, tag, tid, O_CQ, O_STAT, AXW_COLD(qf) + (long)l * qfold_stride(D) + (long)D * D,
                                                        ca_head, shift, qs, p.err, ctl);
            if (fail) ctl[0] = 1;
            AXW_TL(3)
          } else {
            unsigned v[2];
            const bool fail = gather2<1>(GR, tag, v, p.err, ctl, [&](int) { return tid < 32 ? O_CQ + ca_head * 64 + 2 * tid : -1; });
            if (tid < 32) {
              unsigned hi, lo;
              h16split2(__uint_as_float(v[0]), __uint_as_float(v[1]), hi, lo);
              qs[tid] = hi;
              qs[32 + tid] = lo;
            }
            if (fail) ctl[0] = 1;
          }
          AXW_STAMP(7)
          AXW_BARRIER_CHECK(0x500 + l)
          AXW_STAMP(8)
        }
        // ---- cross-attention output projection: merge the partials of every head
        if (in_o) {
          if constexpr (kCoMergeInGather && QF) {
            // Merge inside the gather (co_gather_merge): the compute waves poll the records, merge in registers and write
            // act[0..D) BEFORE the stage's one barrier; the pollers only meet them there. That write is safe with the query fold:
            // a cross-attention unit needs the statistics line of EVERY row producer for its query, and a producer publishes that
            // line through its compute wave that arrives LAST, behind all its waves' reads of act[0..D) (W_o's rows and the rows
            // of M) — so every read of act by this workgroup lies causally behind any record a lane can have gathered. Not so
            // without the fold: a head's query rows come from four producers only, so the unfolded launch keeps the LDS form,
            // whose writes in front of the barrier go to pbuf. A lane that gives up sets ctl[0] before the check barrier: a
            // merge of unfinished data is discarded there. Stamps 9 / 10 and timeline points 5 / 6 behind the barrier: for the
            // pollers the records are gathered and merged at the same moment.
            AXW_BARRIER_CHECK(0x600 + l)
            AXW_STAMP(9)
            AXW_TL(5)
            AXW_STAMP(10)
            AXW_TL(6)
          } else {
            // the pollers collect the first NP1 granules of the partial records, the (idle) compute waves the rest
            unsigned y[2 * GP1];  // pair pi of the records: record pi / 33, granules 2 * (pi % 33), +1
            const bool fail = gather2<GP1>(GR, tag, y, p.err, ctl, [&](int j) { const int pi = tid + j * PL; return pi < NPP1 ? O_PART + (pi / (kPS / 2)) * kRec + 2 * (pi % (kPS / 2)) : -1; });
            float* pbuf = act + D;  // [H][kCrossSplit][66]
#pragma unroll
            for (int j = 0; j < GP1; ++j) {
              const int pi = tid + j * PL;
              if (pi < NPP1) { pbuf[2 * pi] = __uint_as_float(y[2 * j]); pbuf[2 * pi + 1] = __uint_as_float(y[2 * j + 1]); }
            }
            if (fail) ctl[0] = 1;
            AXW_STAMP(9)
            AXW_TL(5)
            AXW_BARRIER_CHECK(0x600 + l)
#pragma unroll
            for (int k = 0; k < GD; ++k) {
              const int i = tid + k * PL;
              if (i < D) {
                act[i] = merge_cross_records(pbuf, i);
              }
            }
            wg_barrier();
            AXW_STAMP(10)
            AXW_TL(6)
          }
        }
        // ---- mlp.0
        if constexpr (QF) {  // x += y1, then += y2: the unfolded launch's order of additions
          unsigned y[2 * GD];
          const bool fail = gather2<2 * GPD>(GR, tag, y, p.err, ctl, [&](int j) { const int pr = tid + (j % GPD) * PL; return 2 * pr < D ? (j < GPD ? O_Y1 : O_Y2) + 2 * pr : -1; });
#pragma unroll
          for (int k = 0; k < GD; ++k) if (el(k) < D) x[k] = (x[k] + __uint_as_float(y[k])) + __uint_as_float(y[GD + k]);
          AXW_STAMP(11)
          AXW_TL(7)
          AXW_RAW_STAGE(fail, 0x700 + l, false)
          if (l + 1 < L) ln_prefetch(FL + DecArena::f_stride(D) + DecArena::F_ATTN_LN_W * D, FL + DecArena::f_stride(D) + DecArena::F_ATTN_LN_B * D);
          else ln_prefetch(AXW_COLD(ln_w), AXW_COLD(ln_b));
          g2_prefetch(l + 1 < L ? l + 1 : 0);
          AXW_STAMP(12)
          AXW_TL(8)
        } else {
          unsigned y[GD];
          const bool fail = gather2<GPD>(GR, tag, y, p.err, ctl, AXW_PAIRS_D(O_Y2));
          AXW_STAMP(11)
          AXW_TL(7)
          AXW_LN_STAGE(y, true, fail, 0x700 + l)
          if (l + 1 < L) ln_prefetch(FL + DecArena::f_stride(D) + DecArena::F_ATTN_LN_W * D, FL + DecArena::f_stride(D) + DecArena::F_ATTN_LN_B * D);
          else ln_prefetch(AXW_COLD(ln_w), AXW_COLD(ln_b));
          AXW_STAMP(12)
          AXW_TL(8)
        }
        // ---- mlp.2: the 4d-wide hidden vector is the largest hand-off; the pollers collect its first half, the compute
        //      waves (idle until it is complete, their rows already in registers) the second half
        if (in_f2) {
          constexpr int GH = (F / 4 + PL - 1) / PL;  // pairs per lane of the first half
          unsigned y[2 * GH];
          const bool fail = gather2<GH>(GR, tag, y, p.err, ctl, [&](int j) { const int pi = tid + j * PL; return pi < F / 4 ? O_HID + 2 * pi : -1; });
#pragma unroll
          for (int j = 0; j < GH; ++j) {
            const int pi = tid + j * PL;
            if (pi < F / 4) { act[2 * pi] = __uint_as_float(y[2 * j]); act[2 * pi + 1] = __uint_as_float(y[2 * j + 1]); }
          }
          if (fail) ctl[0] = 1;
          AXW_STAMP(13)
          AXW_TL(9)
          AXW_BARRIER_CHECK(0x800 + l)
        }
      }  // layers

      steps_run = step + 1;
      asm volatile("" : "+v"(tid));
      if (AXW_SKIP_STEP(step)) {  // SOT steps: feed the next forced token, logits are discarded (Whisper.cpp:214-217)
        tok = AXW_COLD(sot)[step + 1];
        if constexpr (QF) wg_barrier();  // the next step's first stage writes act before its barrier: nobody may still be reading it
        continue;
      }
      // ---- final LayerNorm for the vocabulary projection, then merge the argmax partials of every workgroup
      {
        unsigned y[GD];
        const bool fail = gather2<GPD>(GR, (unsigned)(step * L + L), y, p.err, ctl, AXW_PAIRS_D(O_Y3));
        AXW_LN_STAGE(y, true, fail, 0x900)
        if constexpr (NRES > 0) {  // the resident rows' logits: act is the normalised vector until the next step's first stage
          int v0, vb, v1;
          vocab_tail(v0, vb, v1);
          if (vb < v1) {
            float* dump = RULES ? rules_dump(step) : AXW_COLD(logits_dump) ? AXW_COLD(logits_dump) + (long)(step - 3) * AXW_COLD(n_vocab) : nullptr;
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            [[maybe_unused]] RulesRec rec = rules_rec_empty();
            [[maybe_unused]] RulesStep rq{};
            if constexpr (RULES) rq = rules_step(step, v0);
#pragma unroll
            for (int k = 0; k < NRES; ++k) {
              u32x4 w[CD];
#pragma unroll
              for (int i = 0; i < 4 * CD; ++i) {  // a COPY behind the asm: a resident register that the loop redefined would travel as a phi
                unsigned t;
                asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(vres[k][i]));
                w[i / 4][i % 4] = t;
              }
              int tid2 = tid;
              asm volatile("" : "+v"(tid2));  // the activations are re-read from LDS in every pass, not held (24 registers) across the passes
              const float acc = rows_dot<LD, CD>(w, act, tid2);
              const int row = vb + k * (PL / LD) + tid / LD;
              if (tid % LD == 0 && row < v1) {
                if (dump) dump[row] = acc;
                if constexpr (RULES) rules_rec_row(rec, rq, sup, acc, row);
                else if (acc > bv) { bv = acc; bi = row; }
              }
            }
            if constexpr (RULES) {  // one record per poller wave
              rules_rec_wave_reduce(rec);
              if ((tid & 63) == 0) rules_rec_store(rec_p + (tid >> 6) * kRecWords, rec);
            } else {
              wave_argmax(bv, bi);
              // one candidate per poller wave in pscr (free between the attention phases); am_v[0..8) is not: the pollers write
              // the grid's merge there behind B3, while compute wave 0 may still be folding
              if ((tid & 63) == 0) { pscr[tid >> 6] = bv; reinterpret_cast<int*>(pscr)[NPW + (tid >> 6)] = bi; }
            }
          }
        }
        AXW_STAMP(14)
        wg_barrier();  // B3: the compute waves have their workgroup argmax
        if constexpr (RULES) {
          // lanes t < 256: (tv, ti), (sv, si) of workgroup t; lanes 256 + t: (mt, st), (m, s) of workgroup t — two pairs per lane, the
          // round trip of the argmax pairs. Waves 0-3 reduce winners, waves 4-7 logsumexp pairs; wave results to rec_g.
          unsigned v[4];
          const int gw = tid & 255;
          const bool fail2 = gather2<2>(GR, (unsigned)(step + 1), v, p.err, ctl, [&](int k) { return gw < P ? O_REC + kRecWords * gw + (tid >> 8) * 4 + 2 * k : -1; });
          float r0 = __uint_as_float(v[0]), r2 = __uint_as_float(v[2]);
          if (tid < 256) {
            int i0 = (int)v[1], i1 = (int)v[3];
            if (gw >= P) { r0 = -INFINITY; i0 = 0x7fffffff; r2 = -INFINITY; i1 = 0x7fffffff; }
            wave_argmax(r0, i0);
            wave_argmax(r2, i1);
            if ((tid & 63) == 0) { unsigned* o = rec_g + 4 * (tid >> 6); o[0] = __float_as_uint(r0); o[1] = (unsigned)i0; o[2] = __float_as_uint(r2); o[3] = (unsigned)i1; }
          } else {
            float r1 = __uint_as_float(v[1]), r3 = __uint_as_float(v[3]);
            if (gw >= P) { r0 = -INFINITY; r1 = 0.f; r2 = -INFINITY; r3 = 0.f; }
            lse_wave_reduce_dpp(r0, r1);
            lse_wave_reduce_dpp(r2, r3);
            if ((tid & 63) == 0) { unsigned* o = rec_g + 4 * (tid >> 6); o[0] = __float_as_uint(r0); o[1] = __float_as_uint(r1); o[2] = __float_as_uint(r2); o[3] = __float_as_uint(r3); }
          }
          if (fail2) ctl[0] = 1;
          AXW_STAMP(15)
          AXW_BARRIER_CHECK(0xA00)  // B4
        } else {
          unsigned v[2];  // {value, row index} of workgroup tid: one pair
          const bool fail2 = gather2<1>(GR, (unsigned)(step + 1), v, p.err, ctl, [&](int) { return tid < P ? O_AMAX + 2 * tid : -1; });
          // first max wins (Whisper.cpp:42-45)
          float cv = tid < P ? __uint_as_float(v[0]) : -INFINITY;
          int ci = tid < P ? (int)v[1] : 0x7fffffff;
          wave_argmax(cv, ci);  // DPP + row swaps: the __shfl_xor form is twelve dependent ds_bpermute round trips on the token's path
          if ((tid & 63) == 0) { am_v[tid >> 6] = cv; am_i[tid >> 6] = ci; }
          if (fail2) ctl[0] = 1;
          AXW_STAMP(15)
          AXW_BARRIER_CHECK(0xA00)  // B4
        }
      }
      // (declared here, in front of both branches, as the plain launch always had them: the plain instantiations keep their code)
      [[maybe_unused]] float cv = RULES ? 0.f : am_v[0];
      int best_idx = RULES ? 0 : am_i[0];
      if constexpr (RULES) {
        const RulesRec g = rules_rec_grid(rec_g);
        wg_barrier();  // B5: rec_g is free again
        if (step < AXW_NSKIP) {  // the step that fed sot: the no-speech value, then on with the prefix
          if (wg == 0 && tid == 0) AXW_COLD(no_speech)[0] = rules_no_speech_logprob(g);
          tok = AXW_COLD(sot)[step + 1];
          continue;
        }
        const RulesDecision dec = rules_decide(g, AXW_COLD(eot));
        best_idx = dec.id;
        const int nh = step - AXW_NSKIP;  // the history's length
        if (wg == 0 && tid == 0 && AXW_COLD(ts_logprob) && nh < AXW_COLD(ts_stride)) {
          AXW_COLD(ts_logprob)[nh] = dec.logprob;
          AXW_COLD(ts_decision)[nh] = dec.id;
        }
      } else {
        for (int w2 = 1; w2 < NPW; ++w2)
          if (am_v[w2] > cv || (am_v[w2] == cv && am_i[w2] < best_idx)) { cv = am_v[w2]; best_idx = am_i[w2]; }
        // no logit compared greater than -inf (all NaN / -inf: non-finite audio): std::max_element returns index 0
        // (Whisper.cpp:42-45); never let the "no candidate" index reach the embedding lookup
        if ((unsigned)best_idx >= (unsigned)AXW_COLD(n_vocab)) best_idx = 0;
        wg_barrier();  // B5: am_v/am_i are free again
      }
      const int gi = RULES ? step - AXW_NSKIP : step - 3;
      if (AXW_COLD(forced)) {
        if (wg == 0 && tid == 0 && AXW_COLD(argmax_dump) && gi <= AXW_COLD(n_forced)) AXW_COLD(argmax_dump)[gi] = best_idx;
        if (gi < AXW_COLD(n_forced)) tok = AXW_COLD(forced)[gi];
      } else {
        if (best_idx == AXW_COLD(eot) || step + 1 >= AXW_COLD(n_ctx) || n_out >= AXW_COLD(max_new)) { n_done = 1; break; }
        if (wg == 0 && tid == 0) AXW_COLD(out_ids)[n_out] = best_idx;
        ++n_out;
        tok = best_idx;
      }
      if constexpr (RULES) rules_state_push(hist, tok, AXW_COLD(ts_begin));
    }
#undef AXW_LN_STAGE
#undef AXW_LN_STAGE_X
#undef AXW_RAW_STAGE
#undef AXW_PAIRS_D
  } else {
    // ======================================================================================= compute waves
    // The pollers spin; without a priority the arbiter gives their loops the same share of the issue slots as the
    // waves that do the work (measured: decode 178 -> 158 ms for Whisper-small with this one instruction).
    __builtin_amdgcn_s_setprio(3);
    int ctid = tid - PL;
    // Which workgroups produce the rows of a phase. A hand-off is faster the fewer workgroups publish into it
    // (12 producers: 0.9 us, 256: 2-2.7 us), so a layer's rows go to as few producers as one full pass each allows
    // (16 rows for K = d). Every workgroup must still publish in at least one all-to-all phase of every layer — that
    // is what bounds how far any consumer can lag behind a producer that reuses a buffer one layer later — so the
    // 4d-wide layer (first workgroups) and the 3d-wide one (last workgroups) are packed only if together they cover
    // the grid; otherwise the 4d-wide layer keeps the even deal over all workgroups.
    constexpr int SLD = CT / LD, NP_Q = (3 * D + SLD - 1) / SLD, NP_F = (F + SLD - 1) / SLD;
    const int pk_qkv = NP_Q <= P ? P - NP_Q : -1;
    // The 4d-wide layer's producers start BEHIND the NP_D workgroups that produce the three d-wide layers (those are
    // the busiest: their mlp.0 rows could only be requested after their cross-attention-output publish, ~2 us before
    // use, and arrived late — every consumer of the hidden vector waited for them: 1.2 us of skew per layer).
    const int pk_f = (NP_D + NP_F <= P && NP_Q <= P && NP_D + NP_F + NP_Q >= P) ? NP_D : ((NP_F <= P && NP_Q <= P && NP_F + NP_Q >= P) ? 0 : -1);
    const bool is_fc1 = pk_f < 0 || (rwg >= pk_f && rwg < pk_f + NP_F);
    // its mlp.2 rows can be requested a phase earlier (no mlp.0 rows in the way); not for wide models: 10 chunks per lane
    // held across the mlp.0 phase do not fit the register budget (the d=1280 instantiation went to scratch)
    constexpr bool kEarlyFc2 = CF <= 6;
    const bool early_fc2 = kEarlyFc2 && in_f2 && !is_fc1;
    const int pk_d = 0;  // d rows in passes of CT/LD (or CT/LF) rows: never more producers than workgroups (P <= d)
    // two register sets for the d-wide layers are enough: a phase computes from one while the next phase's rows land
    // in the other (qkv A, o B, cq A, co B, mlp.0 A, [mlp.2 F], next qkv / vocabulary A)
    RowSet<LD, CD> ra, rb;
    RowSet<LF, CF> rs_fc2;
    // QKV rows of layer `ly`: with their LayerNorm folded in (QF) or with their plain bias
    auto qkv_prefetch = [&](int ly) {
      const h16* w = p.wl + (long)ly * DecArena::w_stride(D);
      if constexpr (QF) {
        const float* v = AXW_COLD(qf) + (long)ly * qfold_stride(D) + (long)D * D;
        ra.prefetch_ln(w, v + QF_SQKV * D, v + QF_CQKV * D, D, 3 * D, rwg, P, ctid, pk_qkv);
      } else {
        ra.prefetch(w, p.fl + (long)ly * DecArena::f_stride(D) + DecArena::F_B_QKV * D, D, 3 * D, rwg, P, ctid, pk_qkv);
      }
    };
    // mean and rstd of the stage the pollers have just closed: the eight partial sums + the shift they are relative to
    auto stage_stats = [&](float& mean, float& rstd) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < NPW; ++w2) { t1 += red[2 * w2]; t2 += red[2 * w2 + 1]; }
      const float dm = t1 / D, var = fmaxf(t2 / D - dm * dm, 0.f);
      mean = red[2 * NPW + 1] + dm;
      rstd = rsqrtf(var + 1e-5f);
    };
    qkv_prefetch(0);
    {  // the first layer's cross-attention unit has no previous layer to hide behind
      const int cu0 = ca_unit_of(0, NU, wg, NS);
      if (cu0 >= 0) {
        const int lane = ctid & 63, cw = __builtin_amdgcn_readfirstlane(ctid >> 6);
        const long off = (cu0 / kCrossSplit) * layout::kv_head_elems(kCrossKeysPad) + layout::kv_chunk_offset((cu0 % kCrossSplit) * NCW + cw, 0, 0);
        stage_cross_kv(p.cross_k + off, p.cross_v + off, sK + layout::kv_chunk_offset(cw, 0, 0), sV + layout::kv_chunk_offset(cw, 0, 0), 0, 16, lane);
      }
    }

    for (int step = 0; step < p.total_steps; ++step) {
      for (int l = 0; l < L; ++l) {
        asm volatile("" : "+v"(ctid));
        const bool tl_on = step == p.total_steps / 2 && l == L / 2;
        const int lane = ctid & 63, cw = __builtin_amdgcn_readfirstlane(ctid >> 6);
        constexpr long DD = (long)D * D;
        const h16* WL = p.wl + (long)l * DecArena::w_stride(D);
        const float* FL = p.fl + (long)l * DecArena::f_stride(D);
        const h16 *w_qkv = WL + DecArena::W_QKV * DD, *w_o = WL + DecArena::W_O * DD, *w_cq = WL + DecArena::W_CQ * DD,
                   *w_co = WL + DecArena::W_CO * DD, *w_fc1 = WL + DecArena::W_FC1 * DD, *w_fc2 = WL + DecArena::W_FC2 * DD;
        const float *b_qkv = FL + DecArena::F_B_QKV * D, *b_o = FL + DecArena::F_B_O * D, *b_cq = FL + DecArena::F_B_CQ * D,
                    *b_co = FL + DecArena::F_B_CO * D, *b_fc1 = FL + DecArena::F_B_FC1 * D, *b_fc2 = FL + DecArena::F_B_FC2 * D;
        const unsigned tag = (unsigned)(step * L + l + 1);
        const int cu = ca_unit_of(step * L + l, NU, wg, NS);
        // Cross K/V tiles are constant during the utterance: the unit this workgroup runs in the NEXT layer is staged
        // into LDS now (LDS-DMA, 16 x 1 KiB per wave), a few instructions after each publish of this layer, so that no
        // publish waits behind a burst of DMA requests. Units of one workgroup are at least two layers apart (ca_unit_of).
        const int ln = l + 1 < L ? l + 1 : 0;
        const int cun = ca_unit_of(step * L + l + 1, NU, wg, NS);
        auto kv_piece = [&](int i0, int i1) {
          if (cun < 0) return;
          const int kb = (cun % kCrossSplit) * NCW + cw;  // 64-key block of this wave (24 blocks = t_pad 1536)
          const long off = (long)ln * p.cross_layer_stride + (cun / kCrossSplit) * layout::kv_head_elems(kCrossKeysPad) + layout::kv_chunk_offset(kb, 0, 0);
          stage_cross_kv(p.cross_k + off, p.cross_v + off, sK + layout::kv_chunk_offset(cw, 0, 0), sV + layout::kv_chunk_offset(cw, 0, 0), i0, i1, lane);
        };
        // ---- QKV rows (export_onnx.py:245-247)
        AXW_BARRIER_CHECK(0x100 + l)
        float res[2];
        if constexpr (QF) {
          AXW_STAMP(16)
          AXW_TL(18)
          float mean, rstd;
          stage_stats(mean, rstd);
          const float* v = AXW_COLD(qf) + (long)l * qfold_stride(D) + (long)D * D;
          ra.run_ln(w_qkv, v + QF_SQKV * D, v + QF_CQKV * D, D, act, ctid, res, mean, rstd);
        } else {
          wg_barrier();
          AXW_STAMP(16)
          AXW_TL(18)
          ra.run(w_qkv, b_qkv, D, act, ctid, res);
        }
        ra.publish(ctid, res, pk, ctl + 2, G + O_QKV, tag, [](float v) { return v; });
        if constexpr (QF) {
          // row producers: A0 = W_cq (g . x0) of this slot's row NOW — the self-attention owners' q, k, v are still travelling
          // (x0 has been in LDS since the QKV stage) — then W_o's rows and the rows of M into the registers W_cq's rows leave.
          // W_cq's rows are requested first: results return in issue order, and an owner's publish of its attention vector
          // waits for every load issued before it
          if (in_o) {
            ra.prefetch(w_cq, nullptr, D, D, rwg, P, ctid, pk_d);
            float ra0[2];
            ra.run(w_cq, nullptr, D, act + XG, ctid, ra0);
            if (ctid % LD == 0) act[A0S + ctid / LD] = ra0[0];  // parked in LDS: the attention blocks of an owner need the registers
          }
        }
        rb.prefetch(w_o, b_o, D, D, rwg, P, ctid, pk_d);  // (unconditional: a set assigned on one path only stays live around the step loop)
        kv_piece(0, 2);
        AXW_STAMP(17)
        AXW_TL(10)
        // ---- self-attention of one head over keys 0..step (export_onnx.py:103-147: the -60000 mask + the separate
        //      current-token column of the reference equal causal attention)
        if (l == sa_layer) {
          AXW_BARRIER_CHECK(0x200 + l)
          const int nblk = (step >> 6) + 1;
          if (cw < nblk)
            attn_block<true>(sK + cw * layout::kKvBlockElems, sV + cw * layout::kKvBlockElems, qs, cw * 64 + lane <= step, pscr + cw * 64, wpart + cw * kPS, lane);
          // no second workgroup barrier: the compute wave that arrives last merges the block partials and publishes
          __builtin_amdgcn_wave_barrier();
          int old = 0;
          if (lane == 0) old = __hip_atomic_fetch_add(ctl + 3, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
          old = __builtin_amdgcn_readfirstlane(old);
          if ((old + 1) % NCW == 0) {
            float m, lt, ov;
            merge_partials(wpart, nblk, lane, &m, &lt, &ov);
            gput(G + O_ATT + sa_head * 64 + lane, tag, ov / lt);
          }
          AXW_STAMP(18)
          AXW_TL(11)
        }
        // ---- attention output projection
        if constexpr (QF) {
          if (in_o) {
            // the rows of M: behind the self-attention section (24 registers that the attention blocks need), and behind an
            // owner's publish of its attention vector (a store waits for every load issued before it)
            const float* qfl = AXW_COLD(qf) + (long)l * qfold_stride(D);
            const int slot = ctid / LD, row = rb.r0 + slot < rb.r1 ? rb.r0 + slot : rb.r0;
            RowSetF32<LD, CD> rm;  // this producer's rows of M = W_cq diag(g) W_o (scoped: a set that lived across the step loop was spilled)
            rm.prefetch(qfl, qfl + (long)D * D, D, row, rb.r0 + slot < rb.r1, ctid);
            AXW_BARRIER_CHECK(0x300 + l)
            AXW_STAMP(19)
            AXW_TL(19)
            // y1 rows as always, T = A0 + M a + d for the same rows, and the two sums of this slice of x1 = x0 + y1:
            // three lines, one store instruction each, all by the compute wave that arrives last
            rb.run(w_o, b_o, D, act, ctid, res);
            const float tq = rm.run(act, ctid);
            const int j = ctid % LD, nrows = rb.r1 - rb.r0;
            if (j == 0 && slot < nrows) {
              pk[slot] = res[0];
              pk[32 + slot] = tq + act[A0S + slot];
              pscr[slot] = (act[X0R + rb.r0 + slot] + res[0]) - red[2 * NPW];
            }
            qfold_publish(lane, pk, pscr, ctl + 2, G, O_CQ, O_STAT, O_Y1, rb.r0, nrows, rwg, tag);
            AXW_TL(13)
          }
          rb.prefetch(w_co, b_co, D, D, rwg, P, ctid, pk_d);
          kv_piece(2, 8);
          AXW_STAMP(20)
          AXW_TL(12)
        } else {
          if (in_o) {
            AXW_BARRIER_CHECK(0x300 + l)
            AXW_STAMP(19)
            AXW_TL(19)
            rb.run(w_o, b_o, D, act, ctid, res);
            rb.publish(ctid, res, pk, ctl + 2, G + O_Y1, tag, [](float v) { return v; });
          }
          ra.prefetch(w_cq, b_cq, D, D, rwg, P, ctid, pk_d);
          kv_piece(2, 5);
          AXW_STAMP(20)
          AXW_TL(12)
          // ---- cross-attention query (export_onnx.py:221-230)
          AXW_BARRIER_CHECK(0x400 + l)
          wg_barrier();
          AXW_STAMP(21)
          AXW_TL(20)
          ra.run(w_cq, b_cq, D, act, ctid, res);
          ra.publish(ctid, res, pk, ctl + 2, G + O_CQ, tag, [](float v) { return v; });
          rb.prefetch(w_co, b_co, D, D, rwg, P, ctid, pk_d);
          kv_piece(5, 8);
          AXW_STAMP(22)
          AXW_TL(13)
        }
        // ---- cross-attention over one third of the 1536 padded keys
        if (cu >= 0) {
          const int ca_head = cu / kCrossSplit, ca_split = cu % kCrossSplit;
          AXW_BARRIER_CHECK(0x500 + l)
          cross_unit_block(sK, sV, qs, pscr, wpart, ctl + 3, G + O_PART + (ca_head * kCrossSplit + ca_split) * kRec, tag, ca_split, p.n_audio_ctx, cw, lane);
          AXW_STAMP(23)
          AXW_TL(14)
        }
        // ---- cross-attention output projection
        if (in_o) {
          if constexpr (kCoMergeInGather && QF) {  // the merge tasks (see the pollers), one barrier
            const bool fail = co_gather_merge<D>(GR, tag, O_PART, ctid, act, p.err, ctl);
            if (fail) ctl[0] = 1;
            AXW_BARRIER_CHECK(0x600 + l)
          } else {
            {
              unsigned y[2 * GP2];
              const bool fail = gather2<GP2>(GR, tag, y, p.err, ctl, [&](int j) { const int pi = NPP1 + ctid + j * CT; return pi < NPP ? O_PART + (pi / (kPS / 2)) * kRec + 2 * (pi % (kPS / 2)) : -1; });
              float* pbuf = act + D;
#pragma unroll
              for (int j = 0; j < GP2; ++j) {
                const int pi = NPP1 + ctid + j * CT;
                if (pi < NPP) { pbuf[2 * pi] = __uint_as_float(y[2 * j]); pbuf[2 * pi + 1] = __uint_as_float(y[2 * j + 1]); }
              }
              if (fail) ctl[0] = 1;
            }
            AXW_BARRIER_CHECK(0x600 + l)
            wg_barrier();
          }
          AXW_STAMP(24)
          AXW_TL(21)
          rb.run(w_co, b_co, D, act, ctid, res);
          rb.publish(ctid, res, pk, ctl + 2, G + O_Y2, tag, [](float v) { return v; });
        }
        if constexpr (QF) {
          const float* v = AXW_COLD(qf) + (long)l * qfold_stride(D) + (long)D * D;
          ra.prefetch_ln(w_fc1, v + QF_SFC1 * D, v + QF_CFC1 * D, D, F, rwg, P, ctid, pk_f);
        } else {
          ra.prefetch(w_fc1, b_fc1, D, F, rwg, P, ctid, pk_f);
        }
        if constexpr (kEarlyFc2) {
          if (early_fc2) rs_fc2.prefetch(w_fc2, b_fc2, F, D, rwg, P, ctid, pk_d);
        }
        kv_piece(8, 11);
        AXW_STAMP(25)
        AXW_TL(15)
        // ---- mlp.0 + GELU (export_onnx.py:298)
        AXW_BARRIER_CHECK(0x700 + l)
        if constexpr (QF) {
          AXW_STAMP(26)
          AXW_TL(22)
          float mean, rstd;
          stage_stats(mean, rstd);
          const float* v = AXW_COLD(qf) + (long)l * qfold_stride(D) + (long)D * D;
          ra.run_ln(w_fc1, v + QF_SFC1 * D, v + QF_CFC1 * D, D, act, ctid, res, mean, rstd);
        } else {
          wg_barrier();
          AXW_STAMP(26)
          AXW_TL(22)
          ra.run(w_fc1, b_fc1, D, act, ctid, res);
        }
        ra.publish(ctid, res, pk, ctl + 2, G + O_HID, tag, [](float v) { return gelu_erf(v); });
        if (!early_fc2) rs_fc2.prefetch(w_fc2, b_fc2, F, D, rwg, P, ctid, pk_d);
        kv_piece(11, 13);
        AXW_STAMP(27)
        AXW_TL(16)
        // ---- mlp.2
        if (in_f2) {
          {
            constexpr int GH = (F / 4 + CT - 1) / CT;
            unsigned y[2 * GH];
            const bool fail = gather2<GH>(GR, tag, y, p.err, ctl, [&](int j) { const int pi = ctid + j * CT; return pi < F / 4 ? O_HID + F / 2 + 2 * pi : -1; });
#pragma unroll
            for (int j = 0; j < GH; ++j) {
              const int pi = ctid + j * CT;
              if (pi < F / 4) { act[F / 2 + 2 * pi] = __uint_as_float(y[2 * j]); act[F / 2 + 2 * pi + 1] = __uint_as_float(y[2 * j + 1]); }
            }
            if (fail) ctl[0] = 1;
          }
          AXW_BARRIER_CHECK(0x800 + l)
          AXW_STAMP(28)
          AXW_TL(23)
          rs_fc2.run(w_fc2, b_fc2, F, act, ctid, res);
          rs_fc2.publish(ctid, res, pk, ctl + 2, G + O_Y3, tag, [](float v) { return v; });
          AXW_STAMP(31)
        }
        // next consumer of the residual stream: the next layer's QKV rows, the vocabulary projection, or the next step
        if (l + 1 < L) qkv_prefetch(l + 1);
        else if (AXW_VOCAB_STEP(step)) ra.prefetch(AXW_COLD(tok_emb), nullptr, D, AXW_COLD(n_vocab), rwg, P, ctid);
        else qkv_prefetch(0);
        kv_piece(13, 16);
        AXW_STAMP(29)
        AXW_TL(17)
      }  // layers

      steps_run = step + 1;
      asm volatile("" : "+v"(ctid));
      if (AXW_SKIP_STEP(step)) {
        tok = AXW_COLD(sot)[step + 1];
        if constexpr (QF) wg_barrier();
        continue;
      }
      // ---- logits = token_embedding . ln(x)  (tied embedding, export_onnx.py:364-385) + argmax (first max wins, Whisper.cpp:42-45)
      {
        constexpr int SD = CT / LD;
        const int lane = ctid & 63, cw = __builtin_amdgcn_readfirstlane(ctid >> 6);
        const int N = AXW_COLD(n_vocab);
        const int slot = ctid / LD, j = ctid % LD;
        AXW_BARRIER_CHECK(0x900)
        wg_barrier();
        // activations of this lane's chunks stay in registers over all passes (wide models: re-read from LDS per pass,
        // the registers are needed for the rows in flight)
        constexpr bool kActInRegs = CD <= 3;
        float4 a[kActInRegs ? CD : 1][2];
        if constexpr (kActInRegs) {
#pragma unroll
          for (int i = 0; i < CD; ++i) {
            a[i][0] = *reinterpret_cast<const float4*>(act + (j + LD * i) * 8);
            a[i][1] = *reinterpret_cast<const float4*>(act + (j + LD * i) * 8 + 4);
          }
        }
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        float* dump = RULES ? rules_dump(step) : AXW_COLD(logits_dump) ? AXW_COLD(logits_dump) + (long)(step - 3) * N : nullptr;
        // the pollers hold the last `nres` rows of the range (vocab_tail): stream the rest
        const int nres = NRES > 0 && AXW_COLD(vocab_resident) ? (ra.r1 - ra.r0 > VCAP ? VCAP : ra.r1 - ra.r0) : 0;
        const int r0 = ra.r0, r1 = ra.r1 - nres;
        [[maybe_unused]] RulesRec rec = rules_rec_empty();
        [[maybe_unused]] RulesStep rq{};
        if constexpr (RULES) rq = rules_step(step, ra.r0);
        auto consume = [&](const u32x4 (&wr)[CD], int row) {
          float acc;
          if constexpr (kActInRegs) acc = rows_dot_reg<LD, CD>(wr, a);
          else acc = rows_dot<LD, CD>(wr, act, ctid);
          if (j == 0) {
            if (dump) dump[row] = acc;
            if constexpr (RULES) rules_rec_row(rec, rq, sup, acc, row);
            else if (acc > bv) { bv = acc; bi = row; }
          }
        };
        if constexpr (CD <= 3) {  // two passes ahead: ra.w holds pass 0, wn pass 1
          u32x4 wn[CD];
          {
            const int nrow = r0 + slot + SD;
            rows_load<LD, CD, kVocabNT>(wn, AXW_COLD(tok_emb), D, nrow < r1 ? nrow : r0, ctid);
          }
          for (int row = r0 + slot; row < r1; row += SD) {
            u32x4 wr[CD];
#pragma unroll
            for (int i = 0; i < CD; ++i) { wr[i] = ra.w[i]; ra.w[i] = wn[i]; }
            const int nrow = row + 2 * SD;
            rows_load<LD, CD, kVocabNT>(wn, AXW_COLD(tok_emb), D, nrow < r1 ? nrow : r0, ctid);
            consume(wr, row);
          }
        } else {  // wide rows: one pass ahead (register budget)
          for (int row = r0 + slot; row < r1; row += SD) {
            u32x4 wr[CD];
#pragma unroll
            for (int i = 0; i < CD; ++i) wr[i] = ra.w[i];
            const int nrow = row + SD;
            rows_load<LD, CD, kVocabNT>(ra.w, AXW_COLD(tok_emb), D, nrow < r1 ? nrow : r0, ctid);
            consume(wr, row);
          }
        }
        // the next step's first rows: requested before the token is even known
        qkv_prefetch(0);
        if constexpr (RULES) {
          // one record per compute wave (lanes with j != 0 hold the empty one); behind B3 compute wave 0 folds them with the poller
          // waves' and publishes the workgroup's eight words: lanes 0-7, one store instruction
          rules_rec_wave_reduce(rec);
          if (lane == 0) rules_rec_store(rec_c + cw * kRecWords, rec);
          wg_barrier();  // B3 (all waves)
          if (cw == 0) {
            const RulesRec wr = rules_rec_fold(rec_c, rec_p, nres > 0, lane);
            if (lane < kRecWords) gput_u(G + O_REC + kRecWords * wg + lane, (unsigned)(step + 1), rules_rec_word(wr, lane));
          }
          AXW_STAMP(30)
          AXW_BARRIER_CHECK(0xA00)  // B4
        } else {
          // workgroup argmax: lanes with j == 0 hold candidates; the lower index wins ties
          if (j != 0) { bv = -INFINITY; bi = 0x7fffffff; }
          wave_argmax(bv, bi);
          if (lane == 0) { am_v[8 + cw] = bv; am_i[8 + cw] = bi; }
          // compute waves only: named exchange through LDS, then wave 0 publishes. The pollers sit at B3 meanwhile.
          wg_barrier();  // B3 (all waves)
          if (ctid == 0) {
            for (int w2 = 1; w2 < NCW; ++w2)
              argmax_take(bv, bi, am_v[8 + w2], am_i[8 + w2]);
            if (nres > 0) {  // the poller waves' candidates over the resident rows
              for (int w2 = 0; w2 < NPW; ++w2) {
                const float pv = pscr[w2];
                const int pi = reinterpret_cast<const int*>(pscr)[NPW + w2];
                argmax_take(bv, bi, pv, pi);
              }
            }
            am_v[8] = bv; am_i[8] = bi;
          }
          __builtin_amdgcn_wave_barrier();
          if (ctid < 2)  // value and index of this workgroup's best row in ONE store instruction
            gput_u(G + O_AMAX + 2 * wg + ctid, (unsigned)(step + 1), ctid == 0 ? __float_as_uint(am_v[8]) : (unsigned)am_i[8]);
          AXW_STAMP(30)
          AXW_BARRIER_CHECK(0xA00)  // B4
        }
      }
      // (declared here, in front of both branches, as the plain launch always had them: the plain instantiations keep their code)
      [[maybe_unused]] float cv = RULES ? 0.f : am_v[0];
      int best_idx = RULES ? 0 : am_i[0];
      if constexpr (RULES) {  // as in the pollers' copy of this decision
        const RulesRec g = rules_rec_grid(rec_g);
        wg_barrier();  // B5
        if (step < AXW_NSKIP) {
          tok = AXW_COLD(sot)[step + 1];
          continue;
        }
        best_idx = rules_decide(g, AXW_COLD(eot)).id;
      } else {
        for (int w2 = 1; w2 < NPW; ++w2)
          if (am_v[w2] > cv || (am_v[w2] == cv && am_i[w2] < best_idx)) { cv = am_v[w2]; best_idx = am_i[w2]; }
        if ((unsigned)best_idx >= (unsigned)AXW_COLD(n_vocab)) best_idx = 0;  // as in the pollers' copy of this merge
        wg_barrier();  // B5
      }
      const int gi = RULES ? step - AXW_NSKIP : step - 3;
      if (AXW_COLD(forced)) {
        if (gi < AXW_COLD(n_forced)) tok = AXW_COLD(forced)[gi];
      } else {
        if (best_idx == AXW_COLD(eot) || step + 1 >= AXW_COLD(n_ctx) || n_out >= AXW_COLD(max_new)) { n_done = 1; break; }
        ++n_out;
        tok = best_idx;
      }
      if constexpr (RULES) rules_state_push(hist, tok, AXW_COLD(ts_begin));
    }
  }

  AXW_PERSIST_DRAIN
  if (wg == 0 && tid == 0) {
    AXW_COLD(n_out)[0] = n_out;
    AXW_COLD(state)->step = steps_run;
    AXW_COLD(state)->n_done = n_done;
  }
#undef AXW_TL
#undef AXW_NSKIP
#undef AXW_VOCAB_STEP
#undef AXW_SKIP_STEP
}

// ---------------------------------------------------------------------------------------- host side (both launches)
int decode_persistent_grid(int d_model, int n_cu) {
  int g = n_cu < d_model ? n_cu : d_model;  // every workgroup owns at least one row of the narrowest layer
  return g < 256 ? g : 256;                 // the argmax merge reads 2 granules per workgroup with 512 poller lanes
}
bool decode_persistent_supported(int d_model, int n_head, int n_layer, int n_cu) {
  if (n_head * 64 != d_model) return false;
  const int P = decode_persistent_grid(d_model, n_cu);
  // one (layer, head) self-attention cache per workgroup; the rest take the 3 * n_head cross-attention units of a layer
  if (P - n_layer * n_head < 2 * kCrossSplit * n_head) return false;  // and units of one workgroup >= 2 layers apart
  return persist_dispatch(d_model, [](auto) { return hipSuccess; }) == hipSuccess;
}
int decode_persistent_max_clips(int d_model, int n_head, int n_layer, int grid) {
  // every linear layer must be ONE pass of rows per workgroup (a second pass overwrites the rows the next clip still
  // needs): true up to d_model 768, not for 1280 (mlp.0: 20 rows per workgroup in passes of 16)
  if (d_model > 768) return 1;
  int nc = 1;
  // every workgroup that owns no self-attention head takes at most ONE cross-attention unit (a clip's head and key range) per
  // layer, and the later clips' vectors must fit what the K/V region leaves of the CU's 160 KB of LDS
  while (nc < 3 && grid - n_layer * n_head >= (nc + 1) * kCrossSplit * n_head && persist_lds_bytes(d_model, nc + 1) <= 160 * 1024) ++nc;
  return nc;
}
// rows per workgroup that the one-clip launch keeps in its poller waves (the production instantiation; a workgroup whose range
// is shorter keeps all of it: the smallest range of the even deal has n_vocab / grid rows)
int decode_persistent_vocab_resident_rows(int d_model, int n_vocab, int grid) {
  int cap = 0;
  (void)persist_dispatch(d_model, [&](auto sh) {
    using S = decltype(sh);
    cap = kVocabRes<S::CD, false> * (PL / S::LD);
    return hipSuccess;
  });
  const int rows = grid > 0 ? n_vocab / grid : 0;
  return cap < rows ? cap : rows;
}
// 16 d-wide buffers, the argmax pairs at 16 d (up to 512 granules), the fold's statistics at 16 d + 512 (one 16-granule line
// per row producer, at most d / 16 of them), the rules instantiation's records at 17 d + 512 (eight granules per workgroup, at most
// 256 of them), the error word last
size_t decode_persistent_gran_bytes(int d_model, int /*grid*/) { return ((size_t)16 * d_model + 512 + (size_t)d_model + 256 * kRecWords + 64) * 8; }
// the rules instantiation keeps the suppress mask's words over a workgroup's rows in LDS (decode_persistent_rules.hpp)
bool decode_persistent_rules_supported(int n_vocab, int grid) { return grid >= 1 && grid <= 256 && n_vocab / grid + 1 <= kRulesMaxRange; }

// the profiling stamps are a separate instantiation: the production kernel carries none of their code
template <int LD, int CD, int LF, int CF>
static hipError_t launch_one(const PersistParams& p, int grid, hipStream_t s) {
  constexpr int D = 8 * LD * CD;
  if (p.rules) {  // timestamp and scored mode: the rules instantiation (no timeline build of it)
    if (p.prof || p.n_prefix < 2 || p.n_prefix > 4 || !decode_persistent_rules_supported(p.n_vocab, grid) || p.ts_begin <= p.eot || p.ts_begin > p.n_vocab ||
        (p.ts_logprob && (!p.ts_decision || !p.no_speech || p.ts_stride < 1 || p.no_speech_id < 0 || p.no_speech_id >= p.n_vocab)))
      return hipErrorInvalidValue;
    if constexpr (D <= 768) {
      if (p.qf) return launch_persistent(decode_persistent_kernel<LD, CD, LF, CF, false, true, 1>, D, 1, p, grid, s, kRulesLdsBytes);
    }
    return launch_persistent(decode_persistent_kernel<LD, CD, LF, CF, false, false, 1>, D, 1, p, grid, s, kRulesLdsBytes);
  }
  if constexpr (D <= 768) {  // the query fold, when the engine built its arena (p.qf)
    if (p.qf)
      return launch_persistent(p.prof ? decode_persistent_kernel<LD, CD, LF, CF, true, true, 0> : decode_persistent_kernel<LD, CD, LF, CF, false, true, 0>, D, 1, p, grid, s);
  }
  return launch_persistent(p.prof ? decode_persistent_kernel<LD, CD, LF, CF, true, false, 0> : decode_persistent_kernel<LD, CD, LF, CF, false, false, 0>, D, 1, p, grid, s);
}

hipError_t launch_decode_persistent(const PersistParams& p, int d_model, int grid, hipStream_t s) {
  if (p.n_clip >= 2) return launch_decode_persistent2(p, d_model, grid, s);  // two or three clips: decode_persistent2.hip
  return persist_dispatch(d_model, [&](auto sh) {
    using S = decltype(sh);
    return launch_one<S::LD, S::CD, S::LF, S::CF>(p, grid, s);
  });
}

// What Init decides for a decoder shape on n_cu compute units, and who runs which cross-attention unit: the three functions
// above and the kernels' own ca_unit_of, on the host (AX_WHISPER_PersistentDecodePlan; no device is touched).
// plan4: grid, supported (0 / 1), clips per launch (0 when unsupported), workgroups without a self-attention head.
// units (optional) [n_slots][grid]: the unit of every workgroup in layer slots t0 .. t0 + n_slots - 1 of an n_clips launch.
int decode_persistent_plan(int d_model, int n_head, int n_layer, int n_cu, int n_clips, int t0, int n_slots, int* plan4, int* units) {
  if (d_model < 1 || n_head < 1 || n_layer < 1 || n_cu < 1 || !plan4) return -1;
  const int grid = decode_persistent_grid(d_model, n_cu);
  const bool ok = decode_persistent_supported(d_model, n_head, n_layer, n_cu);
  const int ns = grid - n_layer * n_head;
  plan4[0] = grid;
  plan4[1] = ok ? 1 : 0;
  plan4[2] = ok ? decode_persistent_max_clips(d_model, n_head, n_layer, grid) : 0;
  plan4[3] = ns;
  if (!units) return 0;
  if (!ok || n_clips < 1 || n_clips > plan4[2] || t0 < 0 || n_slots < 0) return -1;
  const int nu = n_clips * kCrossSplit * n_head;  // NU (one clip) / NUC (decode_persistent2.hip)
  for (int t = 0; t < n_slots; ++t)
    for (int wg = 0; wg < grid; ++wg) units[(long)t * grid + wg] = ca_unit_of(t0 + t, nu, wg, ns);
  return 0;
}

}  // inline namespace AXW_NS
}  // namespace axw
