// decode_layout_tables.cpp — prints the index maps of whisper.axera_amd/csrc/decode_layout.hpp over small ranges, one table per
// line ("name v0 v1 ..."), for tests/test_decode_kernel_reference.py::test_index_maps to compare element for element with the
// Python references' own statement of the same layouts. Host only: g++ -std=c++17 -I whisper.axera_amd/csrc.
#include <cstdio>

#include "decode_layout.hpp"

using namespace axw::layout;

int main() {
  const int ROWS = 40, K = 96, NBS = 3, KS = K / 32, KEYS = 448, DIM = 64;
  printf("frag");  // activation pair: [clip][k], nbs allocated clip blocks
  for (int r = 0; r < ROWS; ++r) for (int k = 0; k < K; ++k) printf(" %ld", frag_index(r, k, NBS));
  printf("\nwfrag");  // packed weights: [row][k]
  for (int r = 0; r < ROWS; ++r) for (int k = 0; k < K; ++k) printf(" %ld", wfrag_index(r, k, KS));
  printf("\nwfrag_source");  // the packing kernels' direction: (row, k) of every packed element of 48 rows
  for (long i = 0; i < wfrag_elems(ROWS, K); ++i) { const RowK s = wfrag_source(i, KS); printf(" %d %d", s.row, s.k); }
  printf("\nk");  // blocked K: [key][dim]
  for (int t = 0; t < KEYS; ++t) for (int c = 0; c < DIM; ++c) printf(" %d", k_index(t, c));
  printf("\nv");  // row-major V
  for (int t = 0; t < KEYS; ++t) for (int c = 0; c < DIM; ++c) printf(" %d", v_index(t, c));
  printf("\nvt");  // transposed V of the persistent launches' LDS cache
  for (int t = 0; t < KEYS; ++t) for (int c = 0; c < DIM; ++c) printf(" %d", vt_index(t, c));
  printf("\nkv_chunk");  // the readers' 16-byte pieces: [block][chunk][row]
  for (int b = 0; b < KEYS / 64; ++b) for (int i = 0; i < 8; ++i) for (int r = 0; r < 64; ++r) printf(" %d", kv_chunk_offset(b, i, r));
  printf("\nv_row");
  for (int t = 0; t < KEYS; ++t) printf(" %d", v_row_offset(t));
  printf("\nsizes %ld %ld %ld %ld %d %ld %ld", pair_elems(KS, NBS), wfrag_elems(ROWS, K), frag_kstep_stride(NBS), clip_block_offset(32),
         kClipBlockStride, kv_head_elems(KEYS), frag_tile_offset(2, 1, NBS));
  printf("\npart %d %d %d %d %d %ld %ld\n", kPartStride, kPartM, kPartL, kPartO, kAttnSplitMax, part_offset(3, 5, 2, 12, 6), part_elems(4, 12, 6));
  return 0;
}
