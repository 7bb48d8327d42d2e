// mel_window.inc — the text of the long-form window kernel, compiled twice: frontend.hip builds mel_window_kernel (AXW_MEL_WINDOW_CUT 0,
// a full 30 s window at a seek) and long_cuts.hip builds mel_window_cut_kernel (AXW_MEL_WINDOW_CUT 1, the same window ended at
// win_len[a] frames: zero from there on; DESIGN "Chunked long-form"). The includer defines AXW_MEL_WINDOW_KERNEL, AXW_MEL_WINDOW_CUT,
// the constant WF (frames per workgroup) and ordered_to_float.
//
// The window at `seek` is rows [seek, seek + 3000) of the file's store, clamped to the FILE's maximum - 8 and scaled as
// mel_normalize_kernel does, zero past the file's last frame. Store rows and the time-major h16 rows are both [frame][mel], so a
// window is one flat run on either side: a lane moves 8 values per step (2 x 16 B in, 16 B out), no index arithmetic beyond
// one division per thread. The [n_mels][3000] fp32 layout (stage-level callers only) goes through an LDS tile so that both its
// reads and its writes stay coalesced.
#if AXW_MEL_WINDOW_CUT
__global__ __launch_bounds__(256) void AXW_MEL_WINDOW_KERNEL(MelWindowParams p, const int* __restrict__ win_len) {
#else
__global__ __launch_bounds__(256) void AXW_MEL_WINDOW_KERNEL(MelWindowParams p) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);  // [WF][n_mels + 1], only with mel_ref
  const int a = blockIdx.y, nm = p.n_mels, tid = threadIdx.x;
  const int file = p.win_file[a], seek = p.win_seek[a];
  const int f0 = blockIdx.x * WF;
  const int nf = min(WF, kFramesOut - f0);                            // frames of this workgroup
#if AXW_MEL_WINDOW_CUT
  const int nv = min(max(min(p.n_frames[file] - seek, win_len[a]) - f0, 0), nf);  // of them inside the file and before the cut
#else
  const int nv = min(max(p.n_frames[file] - seek - f0, 0), nf);       // of them inside the file
#endif
  const float floor_v = ordered_to_float(p.gmax[file]) - 8.0f;
  const float* src = p.store + ((long)p.frame_off[file] + seek + f0) * nm;
  h16* dst = p.mel_tm ? p.mel_tm + ((long)a * p.mel_rows + 1 + f0) * nm : nullptr;  // row 0 = conv left pad
  const int cols = nm >> 3;  // 8-value groups per frame (n_mels is a multiple of 8)
  const int n_groups = nf * cols, n_valid = nv * cols, ld = nm + 1;
  int f = tid / cols, c = tid - f * cols;
  const int df = 256 / cols, dc = 256 - df * cols;
  for (int g = tid; g < n_groups; g += 256) {
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (g < n_valid) {
      v0 = *reinterpret_cast<const f32x4*>(src + (long)g * 8);
      v1 = *reinterpret_cast<const f32x4*>(src + (long)g * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v0[e] = (fmaxf(v0[e], floor_v) + 4.0f) * 0.25f;
        v1[e] = (fmaxf(v1[e], floor_v) + 4.0f) * 0.25f;
      }
    }
    if (dst) {
      h16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = (h16)v0[e]; o[4 + e] = (h16)v1[e]; }
      *reinterpret_cast<h16x8*>(dst + (long)g * 8) = o;
    }
    if (p.mel_ref) {
      float* t = tile + f * ld + c * 8;
#pragma unroll
      for (int e = 0; e < 4; ++e) { t[e] = v0[e]; t[4 + e] = v1[e]; }
    }
    f += df; c += dc;
    if (c >= cols) { c -= cols; ++f; }
  }
  if (p.mel_ref) {  // uniform per launch
    __syncthreads();
    const int fr = tid & (WF - 1);
    if (fr < nf)
      for (int m = tid / WF; m < nm; m += 256 / WF) p.mel_ref[((long)a * nm + m) * kFramesOut + f0 + fr] = tile[fr * ld + m];
  }
}
