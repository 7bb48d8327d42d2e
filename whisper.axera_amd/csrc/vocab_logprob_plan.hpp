// vocab_logprob_plan.hpp — the tiling of the fused vocabulary log-probability kernel (vocab_logprob.hip), host only and the same in
// both builds: the launcher, the engine's scratch and AX_WHISPER_VocabLogProbPlan (tests place ids at the ends of a split) ask here.
#pragma once

namespace axw {

constexpr int kVocabLogProbChunk = 256;  // columns a workgroup covers per sweep of its row tile: 4 waves x 4 tiles of 16

// The tiling of `rows` rows of d over eot columns. row_tile: 64 rows up to d = 512, 32 up to 1024, 16 up to 2048 (the tile's LDS
// image stays at 65 KB, two workgroups per CU). The 256-column chunks are dealt to n_splits splits of split_cols columns each so that
// row tiles x splits reaches about 1024 workgroups (four per CU) where the columns allow it. false: a shape the kernel does not take.
inline bool vocab_logprob_plan(int d, int rows, int eot, int* row_tile, int* n_splits, int* split_cols) {
  if (d < 128 || d % 128 != 0 || d > 2048 || rows < 1 || eot < 1) return false;
  const int rt = d <= 512 ? 64 : d <= 1024 ? 32 : 16;
  const int tiles = (rows + rt - 1) / rt, chunks = (eot + kVocabLogProbChunk - 1) / kVocabLogProbChunk;
  const int want = (1024 + tiles - 1) / tiles, s0 = want < chunks ? want : chunks;
  const int per = (chunks + s0 - 1) / s0;
  *row_tile = rt;
  *n_splits = (chunks + per - 1) / per;
  *split_cols = per * kVocabLogProbChunk;
  return true;
}

}  // namespace axw
