// cross_v_swizzle_table.cpp — prints, from whisper.axera_amd/csrc/decode_layout.hpp, the persistent launches' LDS image of a cross V
// block for tests/test_cross_v_swizzle_layout.py, once for the swizzled image and once for the plain one:
//   "stage <swz> s0 s1 ..."  the staging map: the source piece (row-major, 8 row + chunk) of each of the 512 LDS pieces
//   "read <swz> a0 a1 ..."   the BYTE address inside the 8 KiB tile that every lane supplies to each of the block's 16 transposed
//                            reads, in the order [dim block nb][k-step ks][half][lane]
// Host only: g++ -std=c++17 -I whisper.axera_amd/csrc.
#include <cstdio>

#include "decode_layout.hpp"

using namespace axw::layout;

int main() {
  for (int swz = 1; swz >= 0; --swz) {
    printf("stage %d", swz);
    for (int slot = 0; slot < 512; ++slot) printf(" %d", cross_v_source_piece(slot, swz != 0));
    printf("\nread %d", swz);
    for (int nb = 0; nb < 4; ++nb)
      for (int ks = 0; ks < 2; ++ks)
        for (int half = 0; half < 2; ++half)
          for (int lane = 0; lane < 64; ++lane) printf(" %d", 2 * cross_v_read_offset(cross_v_read_base(lane, swz != 0), nb, ks, half, swz != 0));
    printf("\n");
  }
  return 0;
}
