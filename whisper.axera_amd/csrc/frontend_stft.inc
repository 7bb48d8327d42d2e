// frontend_stft.inc — the body of the STFT + mel kernel, included by frontend.hip once per variant (textually, so that the clip
// kernel compiles to exactly the code it had before the long-form variant existed: calling a shared inline body changed its
// register allocation). The includer defines
//   AXW_STFT_KERNEL   the kernel's name
//   AXW_STFT_LONG     0: clips (stft_mel_kernel)  1: whole files (stft_mel_long_kernel; DESIGN "Long-form") — file b's samples
//                     start at pcm[ls.pcm_off[b]], there is no staging row and no openai mode, and EVERY frame's row goes to the
//                     per-file store (row ls.frame_off[b] + f) instead of the first 3000 into logmel.
// Staging, DFT, mel projection and their accumulation order are shared, so frame f of the store holds the bits the clip kernel
// writes for frame f < 3000.
#if AXW_STFT_LONG
__global__ __launch_bounds__(256) void AXW_STFT_KERNEL(FrontendParams p, const float* __restrict__ basis_t /*[201][n_mels]*/, LongStoreParams ls) {
#else
__global__ __launch_bounds__(256) void AXW_STFT_KERNEL(FrontendParams p, const float* __restrict__ basis_t /*[201][n_mels]*/) {
  const LongStoreParams ls{};  // not read
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xw = reinterpret_cast<float*>(smem);                 // [FR][XS] windowed frames; later power [FR][PW_LD]
  float2* tw = reinterpret_cast<float2*>(smem + FR * XS * 4);  // [400] (cos, sin)
  __shared__ float red[4];

  const int b = blockIdx.y;
  const int n_real = p.n_samples[b];
  // openai mode: the clip is (virtually) zero-padded or trimmed to 480000 samples before the STFT and frame 3000 of
  // its 3001 frames is dropped (upstream pad_or_trim + stft[..., :-1]; call site generate_data.py:162-176)
  const int n = (!AXW_STFT_LONG && p.openai) ? kFramesOut * kHop : n_real;
  const int n_frames = (!AXW_STFT_LONG && p.openai) ? kFramesOut : 1 + n / kHop;  // 1 + (n + 400 - 400) / 160   (librosa.h:87)
  const int f0 = blockIdx.x * FR;
  if (f0 >= n_frames) return;  // uniform per workgroup
  const float* x = AXW_STFT_LONG ? p.pcm + ls.pcm_off[b] : p.pcm + (long)b * p.stride;
  const int tid = threadIdx.x;

  for (int i = tid; i < kNFFT; i += 256) tw[i] = make_float2(p.twiddle[2 * i], p.twiddle[2 * i + 1]);
  // Stage the 32 windowed frames. Interior workgroups (no reflection at either end of the clip, every sample inside the
  // staging row) take the plain path: k walks the frame, f the frames, no division and no per-sample tests, so the loads
  // of an iteration are independent and go out together.
  const int j_first = f0 * kHop - kNFFT / 2, j_last = (f0 + FR - 1) * kHop + kNFFT - 1 - kNFFT / 2;
  if (j_first >= 0 && j_last < (AXW_STFT_LONG ? n_real : min(n_real, p.stride)) && f0 + FR <= n_frames) {  // uniform per workgroup
    const float* xs = x + j_first;
    for (int k = tid; k < kNFFT; k += 256) {
      const float wk = p.window[k];
#pragma unroll 8
      for (int f = 0; f < FR; ++f) xw[f * XS + k] = xs[f * kHop + k] * wk;
    }
  } else {
    for (int i = tid; i < FR * kNFFT; i += 256) {
      int f = i / kNFFT, k = i - f * kNFFT;
      float v = 0.f;
      if (f0 + f < n_frames) {
        int j = (f0 + f) * kHop + k - kNFFT / 2;       // index into the un-padded signal
        if (j < 0) j = -j;                              // librosa.h:51  x[left - i]
        if (j >= n) j = 2 * n - 2 - j;                  // librosa.h:54  x[size - 2 - i + left]
        j = min(max(j, 0), n - 1);                      // clips shorter than the pad: stay in bounds
        float smp = 0.f;                                // librosa.h:92 (openai mode: zeros behind the clip's end)
        if (AXW_STFT_LONG) { if (j < n_real) smp = x[j]; }
        else if (j < n_real) smp = j < p.stride ? x[j] : p.overflow[p.over_off[b] + (j - p.stride)];  // clips beyond the staging row
        v = smp * p.window[k];
      }
      xw[f * XS + k] = v;
    }
  }
  __syncthreads();

  // ---- DFT on the matrix cores. One v_mfma_f32_32x32x2_f32 multiplies A = 32 frames x 2 samples (lane: frame lane % 32,
  // sample 2s + lane / 32) by B = 2 samples x 32 bins (lane: bin lane % 32) into a 32 x 32 fp32 tile whose lanes run along
  // the bins and whose registers run along the frames; the cos and the sin tile of the same 32 bins share lane and
  // register, so re^2 + im^2 is register-local. 201 bins = 7 groups of 32: wave w takes groups w and w + 4.
  // B is read from the twiddle table: bin n at sample k needs entry (k * n) mod 400, and k advances by 2 per step.
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int n_groups = (w + 4 < kBinGroups) ? 2 : 1;  // wave-uniform
  f32x16 acc[2][2];  // [group][cos | sin]
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[g][c][e] = 0.f;
  const int bin0 = w * 32 + r, bin1 = (w + 4) * 32 + r;
  int idx0 = (h * bin0) % kNFFT, idx1 = (h * bin1) % kNFFT;
  const int inc0 = (2 * bin0) % kNFFT, inc1 = (2 * bin1) % kNFFT;
  const float* xa = xw + r * XS + h;
  if (n_groups == 2) {
#pragma unroll 4
    for (int s2 = 0; s2 < kNFFT / 2; ++s2) {
      const float a = xa[2 * s2];
      const float2 t0 = tw[idx0], t1 = tw[idx1];
      idx0 += inc0; idx0 -= idx0 >= kNFFT ? kNFFT : 0;
      idx1 += inc1; idx1 -= idx1 >= kNFFT ? kNFFT : 0;
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, t0.x, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, t0.y, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, t1.x, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, t1.y, acc[1][1], 0, 0, 0);
    }
  } else {
#pragma unroll 4
    for (int s2 = 0; s2 < kNFFT / 2; ++s2) {
      const float a = xa[2 * s2];
      const float2 t0 = tw[idx0];
      idx0 += inc0; idx0 -= idx0 >= kNFFT ? kNFFT : 0;
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, t0.x, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, t0.y, acc[0][1], 0, 0, 0);
    }
  }
  __syncthreads();  // all waves are done reading xw
  float* pw = xw;   // power [FR][PW_LD]
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int bin = g ? bin1 : bin0;
    if (g < n_groups && bin <= kBins) {  // bin 201 (of the last group) is the zero that pads the bins to an even count
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int f = (e & 3) + 8 * (e >> 2) + 4 * h;
        const float pv = acc[g][0][e] * acc[g][0][e] + acc[g][1][e] * acc[g][1][e];  // librosa.h:98-100
        pw[f * PW_LD + bin] = bin < kBins ? pv : 0.f;
      }
    }
  }
  __syncthreads();

  // ---- mel projection (librosa.h:153) + log10 (Whisper.cpp:160) + clip maximum (:162-164), also on the matrix cores:
  // [32 frames x 202 bins] . [202 x 32 mels] per wave (wave w: mels 32w .. 32w + 31), the filterbank operand straight from
  // global memory (64-103 KB shared by every workgroup: L1 / L2 hits), lanes along the mels = the contiguous axis of logmel.
  const int nm = p.n_mels;
  float lmax = -3.402823466e38f;
  if (w * 32 < nm) {
    const int m = w * 32 + r;
    const bool m_ok = m < nm;
    f32x16 macc;
#pragma unroll
    for (int e = 0; e < 16; ++e) macc[e] = 0.f;
    const float* pa = pw + r * PW_LD + h;
    const float* bb = basis_t + (long)h * nm + (m_ok ? m : 0);
#pragma unroll 4
    for (int s2 = 0; s2 < (kBins + 1) / 2; ++s2) {
      const int k = 2 * s2 + h;
      const float a = pa[2 * s2];                                  // bin 201 of every row is zero (written above)
      const float bv = (m_ok && k < kBins) ? bb[(long)2 * s2 * nm] : 0.f;
      macc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, macc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int f = (e & 3) + 8 * (e >> 2) + 4 * h;
      if (!m_ok || f0 + f >= n_frames) continue;
      const float v = log10f(fmaxf(macc[e], 1e-10f));
      lmax = fmaxf(lmax, v);
      if (AXW_STFT_LONG) ls.store[((long)ls.frame_off[b] + f0 + f) * nm + m] = v;
      else if (f0 + f < kFramesOut) p.logmel[((long)b * kFramesOut + f0 + f) * nm + m] = v;
    }
  }
  lmax = wave_max(lmax);
  if (lane == 0) red[w] = lmax;
  __syncthreads();
  if (tid == 0) atomicMax(&p.gmax[b], float_to_ordered(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

