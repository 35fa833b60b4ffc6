// riptrm_spack.h — the exact 58-bit packed copy of S that the super-tile S-pass streams (symmetric-tile layout).
//
// S = Z + Z^T is dense noise: its 52 mantissa bits do not compress, its 11 exponent bits do.  Within
// one 128 x 128 tile nearly every entry lies within 31 binades of the largest, so sign + a 5-bit
// exponent code + 52 mantissa bits = 58 bits give every double back bit for bit.
//
// Element (one double, hi:lo dwords):
//   lo   = the low dword, stored as is
//   hi26 = sign (bit 25) | code (bits 24..20) | the top 20 mantissa bits (bits 19..0)
//   code 0      biased exponent field 0 (+-0 and denormals; no base involved)
//   code 1..31  biased exponent ebase + code
// An exponent field outside ebase + 1 .. ebase + 31 (Inf and NaN included) cannot be encoded: the
// tile then stays plain.
//
// Block = one (tile, wave): the wave's 16 rows x 128 columns, 32 elements per lane in the order the
// S-pass holds them: element e = 16 rb + 2 k + c is row 16 w + 8 rb + k, column 2 lane + c
// (sv2[rb][k].x / .y).  Storage (every wave access contiguous across lanes):
//   bytes     0 ..  8191   8 dwordx4 slabs: slab s, lane l holds lo of elements 4 s .. 4 s + 3
//   bytes  8192 .. 14335   6 dwordx4 slabs: slab s, lane l holds dwords 4 s .. 4 s + 3 of the lane's
//   bytes 14336 .. 14847   1 dwordx2 slab:  dwords 24, 25         26-dword stream of 32 x 26 bits
// (element e at bits 26 e .. 26 e + 25 of the stream, so the 8-row batch rb owns dwords 13 rb ..
// 13 rb + 12 and every field extraction is a constant shift).  8 blocks = one tile of 118,784 B
// against 131,072 B plain.
//
// Tile word: one int32 per full tile per instance: 0 = read the tile from plain S, else its ebase
// = (largest biased exponent field in the tile) - 31.  A tile whose ebase would be 0, or that holds
// an element that cannot be encoded, is plain; so are the edge tiles (narrower than 128), which have
// no slot at all.  Full tiles (I, J), I <= J < ntf, are numbered row by row; tile t of instance b
// lives at b * ntiles_full * SPK_TILE_BYTES + t * SPK_TILE_BYTES.
#pragma once
#include <stdint.h>
#include "riptrm_device.h"

namespace riptrm {

constexpr int SPK_ELEMS = 32;                    // elements per lane per block
constexpr int SPK_HI_DWORDS = 26;                // 32 x 26 bits per lane
constexpr int SPK_ROWS = TS / SP_WAVES;          // rows per block
constexpr int SPK_LO_BYTES = SPK_ELEMS * 4 * 64;              // 8192
constexpr int SPK_HI4_BYTES = 24 * 4 * 64;                    // the six dwordx4 slabs of the bit stream
constexpr int SPK_BLOCK_BYTES = SPK_LO_BYTES + SPK_HI_DWORDS * 4 * 64;   // 14848
constexpr int SPK_TILE_BYTES = SP_WAVES * SPK_BLOCK_BYTES;    // 118784
static_assert(SPK_ROWS == 16 && SPK_ELEMS == SPK_ROWS * 2, "a lane holds two columns of the block's 16 rows");
static_assert(SPK_BLOCK_BYTES == 14848 && SPK_TILE_BYTES == 118784, "packed sizes");

// full tiles per dimension (the last tile row / column is an edge unless n fills it) and per instance
inline int32_t spk_ntf_of(int32_t n) { return edge_w_of(n) == TS ? nt_of(n) : nt_of(n) - 1; }
inline int64_t spk_nfull_of(int32_t n) { const int64_t t = spk_ntf_of(n); return t * (t + 1) / 2; }
__host__ __device__ inline int spk_tile_index(int I, int J, int ntf) { return I * ntf - I * (I - 1) / 2 + (J - I); }
// bytes one S-pass reads per instance with every full tile packed
inline int64_t spk_pass_bytes(int32_t n) {
  return s_elems_of(n, RIPTRM_LAYOUT_SYMTILE) * 8 - spk_nfull_of(n) * ((int64_t)TS * TS * 8 - SPK_TILE_BYTES);
}

// byte offset inside a block of lane `lane`'s lo dword j (0..31) / bit-stream dword j (0..25)
__host__ __device__ inline int spk_lo_off(int j, int lane) { return (j >> 2) * 1024 + lane * 16 + (j & 3) * 4; }
__host__ __device__ inline int spk_hi_off(int j, int lane) {
  return j < 24 ? SPK_LO_BYTES + (j >> 2) * 1024 + lane * 16 + (j & 3) * 4 : SPK_LO_BYTES + SPK_HI4_BYTES + lane * 8 + (j - 24) * 4;
}
// tile row / column of element e of lane `lane` in wave w's block
__host__ __device__ inline int spk_row(int w, int e) { return SPK_ROWS * w + 8 * (e >> 4) + ((e >> 1) & 7); }
__host__ __device__ inline int spk_col(int lane, int e) { return 2 * lane + (e & 1); }

// hi dword -> 26-bit field; false when the exponent cannot be encoded with this base
__host__ __device__ inline bool spk_enc_hi(uint32_t hi, int ebase, uint32_t& f) {
  const int E = (int)((hi >> 20) & 0x7FFu);
  const int code = E == 0 ? 0 : E - ebase;
  f = ((hi >> 31) << 25) | ((uint32_t)code << 20) | (hi & 0xFFFFFu);
  return E == 0 || (E != 0x7FF && code >= 1 && code <= 31);
}
// 26-bit field -> hi dword (ebase may be negative: the sum is taken modulo 2^32 and lands in range)
__host__ __device__ inline uint32_t spk_dec_hi(uint32_t f, int ebase) {
  const uint32_t t = f & 0x1FFFFFFu;
  return ((t >> 20) ? t + ((uint32_t)ebase << 20) : t) | ((f >> 25) << 31);
}
// field e of a lane's 26-dword stream (constant shifts once e is a constant)
__host__ __device__ inline uint32_t spk_get(const uint32_t* h, int e) {
  const int bit = 26 * e, i = bit >> 5, s = bit & 31;
  if (s + 26 <= 32) return (h[i] >> s) & 0x3FFFFFFu;
  return ((h[i] >> s) | (h[i + 1] << (32 - s))) & 0x3FFFFFFu;   // a funnel shift (v_alignbit_b32); s >= 7 here
}
__host__ __device__ inline void spk_put(uint32_t* h, int e, uint32_t f) {   // h zeroed beforehand
  const int bit = 26 * e, i = bit >> 5, s = bit & 31;
  h[i] |= f << s;
  if (s + 26 > 32) h[i + 1] |= f >> (32 - s);
}

// Tile classifier.  Fold elements with spk_range_add (emin starts at 0x7FF, emax at 0, bad at 0); the
// zero / denormal field 0 takes no part in the range.
__host__ __device__ inline void spk_range_add(uint32_t hi, int& emin, int& emax, int& bad) {
  const int E = (int)((hi >> 20) & 0x7FFu);
  if (E == 0x7FF) bad = 1;
  else if (E != 0) {
    emin = E < emin ? E : emin;
    emax = E > emax ? E : emax;
  }
}
// the tile word of a folded range: 0 = plain.  A tile of zeros and denormals alone packs with base 1.
__host__ __device__ inline int32_t spk_tile_word(int emin, int emax, int bad) {
  if (bad) return 0;
  if (emax == 0) return 1;
  const int ebase = emax - 31;
  return (ebase != 0 && emin >= ebase + 1) ? ebase : 0;
}

}  // namespace riptrm
