// decode_layout.hpp — the decoder's device data layouts, each defined ONCE: the blocked K cache, the row-major V cache, the
// transposed V of the persistent launches' LDS cache, the fragment-major (hi, lo) activation pairs and packed weights, and the
// attention split record. Kernels, the engine and the host-side table printer (tests/cpp/decode_layout_tables.cpp) all index
// through these functions; tests/decode_kernel_reference.py restates the maps independently and the CPU suite compares the two
// element for element. Plain C++: no HIP include, `__host__ __device__` only where the compiler is hipcc.
#pragma once

#ifdef __HIPCC__
#define AXW_LAYOUT_FN __host__ __device__ constexpr inline
#else
#define AXW_LAYOUT_FN constexpr inline
#endif

namespace axw {
namespace layout {

// ------------------------------------------------------------------ K / V of one (clip, head): 64 dims per key, 64-key blocks
constexpr int kKvDim = 64;                          // head dimension (all Whisper sizes)
constexpr int kKvBlockKeys = 64;                    // keys per block
constexpr int kKvBlockElems = kKvBlockKeys * kKvDim;  // 4096 elements: one block of K or of V
constexpr int kKvChunkElems = 8 * kKvBlockKeys;     // 512: one 8-dim chunk of a K block (8 keys of a transposed V block)

// elements of one head's K or V with `keys_pad` allocated keys (a multiple of 64)
AXW_LAYOUT_FN long kv_head_elems(int keys_pad) { return (long)keys_pad * kKvDim; }
// The readers' view of a blocked tile: element offset of (block, 8-wide chunk, row), a 16-byte piece of 8 elements.
//   blocked K      chunk = dim / 8,        row = key % 64   (lane = key: the q.k dot product is lane-local)
//   transposed V   chunk = (key % 64) / 8, row = dim        (lane = dim: o[dim] accumulates over key pairs)
// Row-major V read in this order is piece chunk * 64 + row of the block's 512 sixteen-byte pieces: a whole-block copy (the persistent
// launches' LDS-DMA of cross K and V tiles) walks both layouts with it.
AXW_LAYOUT_FN int kv_chunk_offset(int block, int chunk, int row) { return block * kKvBlockElems + chunk * kKvChunkElems + row * 8; }
// blocked K [key / 64][dim / 8][key % 64][8]: the self cache, the cross cache and the persistent launches' LDS K
AXW_LAYOUT_FN int k_index(int key, int dim) { return kv_chunk_offset(key >> 6, dim >> 3, key & 63) + (dim & 7); }
// row-major V [key][64]: the self and cross caches in global memory
AXW_LAYOUT_FN int v_row_offset(int key) { return key * kKvDim; }
AXW_LAYOUT_FN int v_index(int key, int dim) { return v_row_offset(key) + dim; }
// transposed V of the persistent launches' own self-attention cache: [key / 64][(key % 64) / 8][dim][8 keys]
AXW_LAYOUT_FN int vt_index(int key, int dim) { return kv_chunk_offset(key >> 6, (key >> 3) & 7, dim) + (key & 7); }

// ------------------------------------------------------------------ FP8 cross K/V of one (clip, head) (cross_kv_fp8.hip; opt-in)
// One byte per element, OCP e4m3fn (largest finite value 448, 0x7f / 0xff NaN; never the fnuz variant), with ONE power-of-two scale
// per (layer, slot, head, K or V, head dimension): value = code * 2^e. e is the smallest integer with amax * 2^-e <= 448, amax
// over the clip's valid keys of that dimension, taken from the exponent and mantissa fields of amax itself (448 = 1.75 * 2^8:
// e = E - 8 where the mantissa is at most 1.75, else E - 7), kept in [kKv8ExpMin, kKv8ExpMax] so that 2^e and 2^-e are both
// normal fp32 numbers; an all-zero channel has e = 0. x * 2^-e is exact in fp32, so a code is one round-to-nearest-even of an exact
// value and the host reproduces it bit for bit (tests/cross_fp8_reference.py).
//   K image  blocked [key / 64][dim / 16][key % 64][16] bytes  (lane = key: a wave's 16-byte loads of one chunk are a contiguous 1 KiB)
//   V image  row-major [key][64] bytes
//   scales   fp32 [layer][slot][head][K, V][64]
// Bytes of keys at or beyond the clip's key count are code 0 in both images.
constexpr int kKv8BlockBytes = kKvBlockKeys * kKvDim;   // 4096: one 64-key block of K or of V
constexpr int kKv8ChunkBytes = 16 * kKvBlockKeys;       // 1024: one 16-dim chunk of a K block
constexpr int kKv8ExpMin = -126, kKv8ExpMax = 120;
AXW_LAYOUT_FN long kv8_head_bytes(int keys_pad) { return (long)keys_pad * kKvDim; }
AXW_LAYOUT_FN int k8_chunk_offset(int block, int chunk, int row) { return block * kKv8BlockBytes + chunk * kKv8ChunkBytes + row * 16; }
AXW_LAYOUT_FN int k8_index(int key, int dim) { return k8_chunk_offset(key >> 6, dim >> 4, key & 63) + (dim & 15); }
AXW_LAYOUT_FN int v8_row_offset(int key) { return key * kKvDim; }
AXW_LAYOUT_FN int v8_index(int key, int dim) { return v8_row_offset(key) + dim; }
constexpr int kKv8ScaleK = 0, kKv8ScaleV = 1;
constexpr int kKv8ScaleHead = 2 * kKvDim;               // floats of one (layer, slot, head): K's 64, then V's 64
AXW_LAYOUT_FN long kv8_scale_index(long layer, long slot, int head, int kv, int dim, int n_slots, int n_head) {
  return ((layer * n_slots + slot) * n_head + head) * kKv8ScaleHead + kv * kKvDim + dim;
}
AXW_LAYOUT_FN long kv8_scale_elems(int n_layer, int n_slots, int n_head) { return kv8_scale_index(n_layer, 0, 0, 0, 0, n_slots, n_head); }
// the scale exponent e of a channel whose largest magnitude has the fp32 bit pattern amax_bits (sign bit clear)
AXW_LAYOUT_FN int kv8_scale_exponent(unsigned amax_bits) {
  if (amax_bits == 0u) return 0;
  const int field = (int)(amax_bits >> 23), E = (field ? field : 1) - 127;
  const int e = (amax_bits & 0x7fffffu) <= 0x600000u ? E - 8 : E - 7;
  return e < kKv8ExpMin ? kKv8ExpMin : e > kKv8ExpMax ? kKv8ExpMax : e;
}
AXW_LAYOUT_FN unsigned kv8_pow2_bits(int e) { return (unsigned)(e + 127) << 23; }  // fp32 bit pattern of 2^e, e in [-126, 127]

// ------------------------------------------------------------------ the persistent launches' LDS image of a cross V block
// A row-major [64 keys][64 dims] block whose eight 16-byte chunks are permuted inside every 128-byte row: LDS slot (row R, chunk c)
// holds the block's chunk c ^ x(R), x(R) = 2 (2 (R / 8 % 2) + R / 2 % 2). The matrix-pipe block reads the tile with transposed
// 8-byte reads (ds_read_b64_tr_b16: per 32-lane half, rows q, q + 1, q + 2, q + 3 of two 4-row blocks eight rows apart, four
// 8-byte columns each); on plain 128-byte rows, rows R and R + 2 and the two blocks share eight of the 64 banks, a 4-way conflict.
// x moves rows R + 2 by two chunks (16 banks) and rows R + 8 by four (32 banks): every read of the block is conflict-free
// (tests/test_cross_v_swizzle_layout.py counts it). A permutation inside a row: no LDS, no HBM byte and no memory line more.
AXW_LAYOUT_FN int cross_v_swizzle(int row) { return 2 * (2 * ((row >> 3) & 1) + ((row >> 1) & 1)); }
// element of (key, dim) in the swizzled block (swz) or the plain row-major one
AXW_LAYOUT_FN int cross_v_index(int key, int dim, bool swz) {
  return swz ? v_row_offset(key) + (((dim >> 3) ^ cross_v_swizzle(key)) << 3) + (dim & 7) : v_index(key, dim);
}
// staging: which of the block's 512 sixteen-byte pieces (row-major order, piece = 8 row + chunk) LDS piece `slot` receives
AXW_LAYOUT_FN int cross_v_source_piece(int slot, bool swz) { return swz ? slot ^ cross_v_swizzle(slot >> 3) : slot; }
// The address (element offset in the block) lane `lane` supplies to transposed read `half` (keys + 0..3 / + 4..7) of B piece (dim
// block nb, k-step ks) of the output product: key 32 ks + 8 (lane / 16) + lane / 4 % 4 + 4 half, dims 16 nb + 4 (lane % 4) .. + 3.
// x does not depend on ks, half or nb, so a lane keeps ONE base and a piece is base ^ 16 nb (+ 16 nb in the plain image) plus a
// constant row offset.
AXW_LAYOUT_FN int cross_v_read_base(int lane, bool swz) { return cross_v_index(8 * (lane >> 4) + ((lane >> 2) & 3), 4 * (lane & 3), swz); }
AXW_LAYOUT_FN int cross_v_read_offset(int base, int nb, int ks, int half, bool swz) {
  return (swz ? base ^ (16 * nb) : base + 16 * nb) + v_row_offset(32 * ks + 4 * half);
}

// ------------------------------------------------------------------ fragment-major MFMA operands (v_mfma_f32_16x16x32)
// A tile is 16 rows x 32 k = 512 elements in the order the instruction consumes them, so an operand load of a wave is ONE
// contiguous 1 KiB access (lane * 16 bytes): element (lane, j) of a tile = [row & 15 = lane & 15][k & 31 = (lane >> 4) * 8 + j].
//   activations (hi and lo each)  tile (ks, cb) at (ks * nbs + cb): clip = cb * 16 + (lane & 15), nbs = allocated clip blocks
//   packed weights                tile (rb, ks) at (rb * KS + ks):  row  = rb * 16 + (lane & 15), KS = K / 32
constexpr int kFragTileElems = 512;
constexpr int kClipBlockStride = kFragTileElems;    // elements between the clip blocks of one k-step
AXW_LAYOUT_FN int frag_lane_offset(int lane) { return lane * 8; }
AXW_LAYOUT_FN int frag_in_tile(int row, int k) { return frag_lane_offset(((k >> 3) & 3) * 16 + (row & 15)) + (k & 7); }
AXW_LAYOUT_FN long frag_tile_offset(long ks, int cb, int nbs) { return (ks * nbs + cb) * kFragTileElems; }
AXW_LAYOUT_FN long wfrag_tile_offset(long rb, int ks, int KS) { return (rb * KS + ks) * kFragTileElems; }
AXW_LAYOUT_FN long frag_index(int clip, int k, int nbs) { return frag_tile_offset(k >> 5, clip >> 4, nbs) + frag_in_tile(clip, k); }
AXW_LAYOUT_FN long wfrag_index(int row, int k, int KS) { return wfrag_tile_offset(row >> 4, k >> 5, KS) + frag_in_tile(row, k); }
AXW_LAYOUT_FN long frag_kstep_stride(int nbs) { return (long)nbs * kFragTileElems; }   // elements between consecutive k-steps of a pair buffer
AXW_LAYOUT_FN long pair_elems(int k_steps, int nbs) { return k_steps * frag_kstep_stride(nbs); }  // one buffer (hi or lo) of a pair
AXW_LAYOUT_FN long clip_block_offset(int clip0) { return (long)(clip0 / 16) * kClipBlockStride; }  // clip0: a multiple of 16
AXW_LAYOUT_FN long wfrag_elems(int N, int K) { return wfrag_tile_offset((N + 15) / 16, 0, K / 32); }   // rows padded to 16
// the packing kernels' direction: which W[row][k] sits at element i of the packed array
struct RowK { int row, k; };
AXW_LAYOUT_FN RowK wfrag_source(long i, int KS) {
  const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
  const long tile = i / kFragTileElems;
  return RowK{(int)(tile / KS) * 16 + (lane & 15), (int)(tile % KS) * 32 + (lane >> 4) * 8 + j};
}

// ------------------------------------------------------------------ attention split record: m, l, o[64]
constexpr int kPartM = 0, kPartL = 1, kPartO = 2;
constexpr int kPartStride = kPartO + kKvDim;        // 66 floats
constexpr int kAttnSplitMax = 6;                    // most workgroups per (clip, head) whose records one launch folds itself
// record of (clip, head, split) in a [clips][n_head][n_split] array, and the floats `clips` clips take
AXW_LAYOUT_FN long part_offset(long clip, int head, int split, int n_head, int n_split) { return ((clip * n_head + head) * n_split + split) * kPartStride; }
AXW_LAYOUT_FN long part_elems(long clips, int n_head, int n_split) { return part_offset(clips, 0, 0, n_head, n_split); }

}  // namespace layout
}  // namespace axw
