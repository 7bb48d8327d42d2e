// beam_candidates_body.inc — the body of beam_candidates_kernel, included once per instantiation (as stream_rules_body.inc is): in
// decode_beam.hip with AXW_BEAM_REP false, where it is the kernel it was before there were repetition rules, instruction for
// instruction, and in decode_beam_rep.hip with AXW_BEAM_REP true and AXW_BEAM_RULES the handle's two values: the ban and seen images
// of decode_rules.hpp, built from the slot's own history (the hypothesis' ids) in the launch's dynamic LDS; the text loop scales the
// seen ids and tests the ban image. In scope: BeamCandParams p; the lists of decode_beam_candidates.hpp.
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
  [[maybe_unused]] RepImages ri{};
  if constexpr (AXW_BEAM_REP) ri = repetition_stage(p.suppress, AXW_BEAM_RULES, p.hist + (long)b * p.hist_stride, n, E);

  const float* row = p.logits + (long)b * p.stride;
  float tv = -INFINITY;                    // best unmasked id below T (rule 5's right-hand side)
  float m = -INFINITY, s = 0.f;            // online logsumexp over the unmasked timestamps
  float mt = -INFINITY, st = 0.f;          // ... over the unmasked text ids and eot
  TopList lt, ls;                          // text + eot / timestamps: rule 5 is only known after the reduction
  lt.clear();
  ls.clear();
  for (int c = (a.text_begin >> 2) + tid; 4 * c < a.text_end; c += 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * c);
    unsigned sup;
    if constexpr (AXW_BEAM_REP) {  // (the ban image holds the set's bits too)
      v = repetition_scale4(v, ri, c);
      sup = suppress_bits4(ri.ban, c);
    } else {
      sup = p.suppress ? suppress_bits4(p.suppress, c) : 0u;  // (measured: this loop loses nothing to the test inside it)
    }
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
