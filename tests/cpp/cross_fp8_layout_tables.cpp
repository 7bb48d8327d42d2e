// cross_fp8_layout_tables.cpp — prints the FP8 cross K/V index maps and the scale rule of whisper.axera_amd/csrc/decode_layout.hpp
// over small ranges, one table per line ("name v0 v1 ..."), for tests/test_cross_fp8_reference.py to compare element for element with
// tests/cross_fp8_reference.py's own statement of them. Host only: g++ -std=c++17 -I whisper.axera_amd/csrc.
#include <cstdio>
#include <cstring>

#include "decode_layout.hpp"

using namespace axw::layout;

int main() {
  const int KEYS = 192, DIM = 64, L = 2, SLOTS = 3, H = 3;
  printf("k8");  // blocked K codes: [key][dim]
  for (int t = 0; t < KEYS; ++t) for (int c = 0; c < DIM; ++c) printf(" %d", k8_index(t, c));
  printf("\nv8");  // row-major V codes
  for (int t = 0; t < KEYS; ++t) for (int c = 0; c < DIM; ++c) printf(" %d", v8_index(t, c));
  printf("\nk8_chunk");  // the readers' 16-byte pieces: [block][chunk][row]
  for (int b = 0; b < KEYS / 64; ++b) for (int i = 0; i < 4; ++i) for (int r = 0; r < 64; ++r) printf(" %d", k8_chunk_offset(b, i, r));
  printf("\nscale");  // [layer][slot][head][K, V][dim]
  for (int l = 0; l < L; ++l) for (int s = 0; s < SLOTS; ++s) for (int h = 0; h < H; ++h) for (int kv = 0; kv < 2; ++kv)
    for (int c = 0; c < DIM; ++c) printf(" %ld", kv8_scale_index(l, s, h, kv, c, SLOTS, H));
  printf("\nsizes %ld %ld %d %d %d %d %d", kv8_head_bytes(KEYS), kv8_scale_elems(L, SLOTS, H), kKv8BlockBytes, kKv8ChunkBytes, kKv8ScaleHead,
         kKv8ExpMin, kKv8ExpMax);
  // the scale exponent of a few magnitudes (printed as bit pattern, exponent), and the bit patterns of 2^e
  const float probes[] = {0.f, 1.f, 447.9f, 448.f, 448.5f, 449.f, 512.f, 0.875f, 0.8750001f, 1.75f, 1.7500001f, 3.4e38f, 1e-38f, 1e-45f,
                          6.1e-5f, 65504.f, 0.0131f, 30.f, 2.f, 1.9999999f};
  printf("\nexponent");
  for (float f : probes) { unsigned u; memcpy(&u, &f, 4); printf(" %u %d", u, kv8_scale_exponent(u)); }
  printf("\npow2");
  for (int e = kKv8ExpMin; e <= 127; ++e) printf(" %u", kv8_pow2_bits(e));
  printf("\n");
  return 0;
}
