// decode_prefill.hip — prompt prefill of the decoder (DESIGN.md "Prompt conditioning"): the context positions in front of the
// first decision, [sot_prev, p_1 .. p_P, sot, language], as ONE pass over all of them instead of one decoder step per position.
//
// The rows of every prompted clip are contiguous in the pass's buffers ([rows][...], clip c at row0[c], len[c] = P_c + 3 rows);
// clips may differ in length. The linear layers are the encoder's GEMM and LayerNorm (gemm.hip); this file has what is left:
//   prefill_embed_kernel         x[row] = tok_emb[ctx[row]] + pos[row's position]                        fp32 [rows][d]
//   prefill_cache_store_kernel   the K and V columns of the QKV GEMM's output -> the self-attention cache of the clip's slot,
//                                rows [0, len): K blocked, V row-major (decode_layout.hpp)
//   prefill_attention_kernel     block attention of many queries over the decode layouts: causal over the slot's self cache, or over
//                                the n_audio_ctx keys of its cross cache                                   h16 [rows][d]
//   prefill_gather_rows_kernel   the final residual row of every clip's sot position (the no-speech row)   fp32 [clips][d]
//   prefill_handover_kernel      the decode state the next step starts from: off = len, tok = transcribe (or the clip's
//                                task id), n_out = 0, x_dec = tok_emb[tok] + pos[len], the no-speech value
// Out of scope here as in the engine: beam search, the Stream* slots and the persistent launches take no prompt.
//
// prefill_attention_kernel: workgroup = 4 waves = 64 queries of one (clip, head), 16 query rows per wave; keys in the 64-key blocks of
// the caches. S^T = K Q^T on v_mfma_f32_16x16x32 (A = 16 keys x 32 dims straight from the blocked K: one 16-byte piece per lane,
// B = the wave's Q rows, held in registers), so a lane has ONE query and 4 keys per tile: the row maximum and sum are lane-local
// plus two exchanges between the four 16-lane groups. The exponentiated tiles, narrowed to h16, are the B operand of O^T = V^T P^T
// with no lane movement; its A operand wants 8 keys of one dim per lane, so the row-major V block is transposed into LDS once per
// block and workgroup (64 dims x 64 keys, rows padded to 72 elements = 9 KiB; the 2-byte transposing stores are bank-conflicted,
// the 8-byte operand reads are not). K is read from global memory by every wave (L1/L2 serve the three repeats).
// The softmax is fp32 and online, the scale 1/8 folded with log2(e) into the exp2 argument (as encoder_attn.hip); the causal mask
// is applied in the diagonal block only, the key-count mask in the last block only.
#include "common.hpp"

namespace axw {
inline namespace AXW_NS {

__global__ __launch_bounds__(256) void prefill_embed_kernel(const h16* __restrict__ tok_emb, const float* __restrict__ pos,
                                                            const int* __restrict__ ctx, const int* __restrict__ row_pos,
                                                            float* __restrict__ x, int d) {
  const int r = blockIdx.x;
  const int t = ctx[r], i = row_pos[r];
  for (int c = threadIdx.x; c < d; c += 256) x[(long)r * d + c] = (float)tok_emb[(long)t * d + c] + pos[(long)i * d + c];
}

void launch_prefill_embed(const h16* tok_emb, const float* pos, const int* ctx, const int* row_pos, float* x, int rows, int d,
                          hipStream_t s) {
  if (rows < 1) return;
  hipLaunchKernelGGL(prefill_embed_kernel, dim3(rows), dim3(256), 0, s, tok_emb, pos, ctx, row_pos, x, d);
}

// one workgroup per row; a thread moves 16-byte pieces (8 dims of one head: contiguous in both layouts)
__global__ __launch_bounds__(256) void prefill_cache_store_kernel(PrefillStoreParams p) {
  const int r = blockIdx.x;
  const int key = p.row_pos[r];
  const long slot_base = (long)p.row_slot[r] * p.kv_slot_stride;
  const int d = p.d_model;
  const h16* src = p.qkv + (long)r * 3 * d + d;  // [K columns | V columns] of this row
  for (int e = threadIdx.x * 8; e < 2 * d; e += 256 * 8) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src + e);
    const int c = e < d ? e : e - d;
    const int head = c >> 6, dd = c & 63;
    const long base = slot_base + head * layout::kv_head_elems(p.n_ctx_pad);
    if (e < d) *reinterpret_cast<u32x4*>(p.k_cache + base + layout::k_index(key, dd)) = v;
    else *reinterpret_cast<u32x4*>(p.v_cache + base + layout::v_index(key, dd)) = v;
  }
}

void launch_prefill_cache_store(const PrefillStoreParams& p, hipStream_t s) {
  if (p.rows < 1) return;
  hipLaunchKernelGGL(prefill_cache_store_kernel, dim3(p.rows), dim3(256), 0, s, p);
}

constexpr int kVtStride = 72;  // elements per row of the transposed V block in LDS (64 keys + 8: 8-byte reads stay aligned)

__global__ __launch_bounds__(256) void prefill_attention_kernel(PrefillAttnParams p) {
  __shared__ __attribute__((aligned(16))) h16 Vt[64 * kVtStride];  // [dim][key] of the current block

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.z, head = blockIdx.y, qb = blockIdx.x;
  const int L = p.len[c];
  if (qb * 64 >= L) return;  // (the whole workgroup: clips of one launch differ in length)
  const int row0 = p.row0[c];
  const bool causal = p.n_keys < 0;
  const int n_keys = causal ? min(L, qb * 64 + 64) : p.n_keys;  // keys any query of this block may see
  const int n_blocks = (n_keys + 63) / 64;
  const int col = lane & 15, g = lane >> 4;
  const int qpos = qb * 64 + wave * 16 + col;  // this lane's query: column of the B operands and of every accumulator
  const h16* qrow = p.q + (long)(row0 + min(qpos, L - 1)) * p.ldq + head * 64;
  h16x8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const h16x8*>(qrow + ks * 32 + g * 8);

  const long head_base = (long)p.slot[c] * p.kv_slot_stride + head * layout::kv_head_elems(p.keys_pad);
  const h16* Kh = p.k + head_base;
  const h16* Vh = p.v + head_base;

  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float sc = 0.125f * 1.44269504088896340736f;  // (64^-0.25)^2 * log2(e)

  for (int kb = 0; kb < n_blocks; ++kb) {
    __syncthreads();  // every wave is done with the block before
    // V block, transposed: 512 pieces of 8 dims of one key; keys at or beyond n_keys as zeros (their probabilities are zeros, their
    // cache rows may hold anything)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int piece = tid + 256 * i, key = piece >> 3, ch = piece & 7;
      h16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (h16)0.f;
      if (kb * 64 + key < n_keys) v = *reinterpret_cast<const h16x8*>(Vh + layout::v_index(kb * 64 + key, ch * 8));
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * kVtStride + key] = v[e];
    }
    __syncthreads();

    // S^T = K Q^T: s[t][i] = score(key = kb*64 + t*16 + 4g + i, query = qpos), unscaled
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const h16x8 kf = *reinterpret_cast<const h16x8*>(Kh + layout::kv_chunk_offset(kb, ks * 4 + g, t * 16 + col));
        s[t] = AXW_MFMA_16x16x32(kf, qf[ks], s[t]);
      }
    }
    const bool diag = causal && kb == qb, last = kb == n_blocks - 1;
    if (diag || last) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = kb * 64 + t * 16 + 4 * g + i;
          if ((last && key >= n_keys) || (diag && key > qpos)) s[t][i] = -INFINITY;
        }
    }
    // online softmax, fp32, base 2 (every block holds at least one key its queries see: the running maximum is finite)
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) mt = fmaxf(mt, s[t][i]);
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);
    m_run = m_new;
    const float m_sc = m_new * sc;
    float ls = 0.f;
    h16x8 pf[2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[t][i], sc, -m_sc));
        ls += pv;
        pf[t >> 1][(t & 1) * 4 + i] = (h16)pv;
      }
    l_run = l_run * alpha + ls;  // this lane's 16 keys of every block; the four groups are added at the end
    // O^T = alpha O^T + V^T P^T: k-step kk takes tiles 2kk and 2kk+1, element j of lane group g is key (2kk + (j >> 2)) * 16 + 4g +
    // (j & 3) — the order the accumulators hold them in, so V^T is read in that order too
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[dt][i] *= alpha;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const h16* vr = Vt + (dt * 16 + col) * kVtStride + kk * 32 + 4 * g;
        const h16x4 v0 = *reinterpret_cast<const h16x4*>(vr), v1 = *reinterpret_cast<const h16x4*>(vr + 16);
        const h16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        o[dt] = AXW_MFMA_16x16x32(vf, pf[kk], o[dt]);
      }
    }
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  if (qpos < L) {
    const float inv = 1.f / l_run;
    h16* orow = p.out + (long)(row0 + qpos) * p.ldo + head * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {  // o[dt][i] = O[query][dim = dt*16 + 4g + i]
      h16x4 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i) pk[i] = (h16)(o[dt][i] * inv);
      *reinterpret_cast<h16x4*>(orow + dt * 16 + 4 * g) = pk;
    }
  }
}

void launch_prefill_attention(const PrefillAttnParams& p, hipStream_t s) {
  if (p.n_clips < 1 || p.max_len < 1) return;
  hipLaunchKernelGGL(prefill_attention_kernel, dim3((p.max_len + 63) / 64, p.n_head, p.n_clips), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void prefill_gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ rows,
                                                                  float* __restrict__ out, int d) {
  const int c = blockIdx.x;
  const long r = rows[c];
  for (int i = threadIdx.x; i < d; i += 256) out[(long)c * d + i] = x[r * d + i];
}

void launch_prefill_gather_rows(const float* x, const int* rows, float* out, int n, int d, hipStream_t s) {
  if (n < 1) return;
  hipLaunchKernelGGL(prefill_gather_rows_kernel, dim3(n), dim3(256), 0, s, x, rows, out, d);
}

__global__ __launch_bounds__(256) void prefill_handover_kernel(PrefillHandoverParams p) {
  const int c = blockIdx.x;
  const int b = p.slot[c], L = p.len[c];
  const int tok = p.task_tok ? p.task_tok[c] : p.transcribe;  // (a clip's own task: DESIGN.md "Language and task per clip")
  if (threadIdx.x == 0) {
    p.off[b] = L;
    p.tok[b] = tok;
    p.n_out[b] = 0;
    if (p.no_speech && p.no_speech_clip) p.no_speech[b] = p.no_speech_clip[c];
  }
  const int d = p.d_model;
  for (int i = threadIdx.x; i < d; i += 256) p.x[(long)b * d + i] = (float)p.tok_emb[(long)tok * d + i] + p.pos[(long)L * d + i];
}

void launch_prefill_handover(const PrefillHandoverParams& p, hipStream_t s) {
  if (p.n_clips < 1) return;
  hipLaunchKernelGGL(prefill_handover_kernel, dim3(p.n_clips), dim3(256), 0, s, p);
}

}  // inline namespace AXW_NS
}  // namespace axw
