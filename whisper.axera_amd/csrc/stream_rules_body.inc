// stream_rules_body.inc — the body of stream_rules_kernel (decode_timestamps.hip), included once per instantiation: without a suppress
// set (AXW_STREAM_SET false, AXW_STREAM_MASK nullptr), where it is the kernel it was before there were sets, and with one. The
// branches of offset 0 and 1 do not look at the set. In scope: TsRulesArgs p, TsScoreParams q, StreamRulesParams t.
  const int b = blockIdx.x;
  if (p.done[b]) return;
  const int off = p.off[b];
  if (off >= p.n_prefix - 1) { rules_body<kRulesScored, AXW_STREAM_SET>(p, AXW_STREAM_MASK, q, TsSampleParams{}); return; }
  if (off != 0) return;
  const float* row = p.logits + (long)b * p.stride;
  row_logprob(row, p.n_vocab, q.no_speech_id, q.no_speech + b);
  if (!t.detect[b]) return;
  __shared__ float s_logit[kLangMax];
  const int tid = threadIdx.x, lane = tid & 63, n_lang = t.n_lang;
  if (tid < n_lang) s_logit[tid] = row[t.lang_tokens[tid]];
  __syncthreads();
  if (tid >= 64) return;
  const int j0 = lane, j1 = lane + 64;
  const float x0 = j0 < n_lang ? s_logit[j0] : NAN, x1 = j1 < n_lang ? s_logit[j1] : NAN;
  float m = -INFINITY;
  int idx = 0x7fffffff;
  argmax_take(m, idx, x0, j0);  // (a NaN compares false: never taken)
  argmax_take(m, idx, x1, j1);
  wave_argmax(m, idx);
  const float n_finite = wave_sum((fabsf(x0) < INFINITY ? 1.f : 0.f) + (fabsf(x1) < INFINITY ? 1.f : 0.f));
  const bool none = !(n_finite > 0.f) || idx >= n_lang;
  float lp0, lp1;
  if (none) {
    idx = t.fallback_index;
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
  if (j0 < n_lang) t.lang_logprob[(long)b * n_lang + j0] = lp0;
  if (j1 < n_lang) t.lang_logprob[(long)b * n_lang + j1] = lp1;
  if (lane == 0) {
    t.lang_out[b] = idx;
    t.slot_ctx[4 * b + 1] = t.lang_tokens[idx];
  }
