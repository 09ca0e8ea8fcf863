// tsim_bitrows.hip.h - the one reader of bit-packed rows, shared by every kernel behind count(): k_tally (tsim_tally.hip.h),
// k_planes (tsim_pairs.hip.h), k_claim / k_verify / k_decode (tsim_rowtab.hip.h), k_uf (tsim_uf.hip.h), k_ufw (tsim_ufw.hip.h).
//
// The row contract:
//   rows   n rows in device memory, row r at rows + r * row_bytes (the stride; any stride >= used, any base alignment).
//          Column c of a row is bit c & 7 of its byte c >> 3 (little-endian); used = ceil(n_cols / 8) bytes hold the columns.
//   xor    optional row of `used` bytes (NULL: zeros); everything is computed on row ^ xor.
//   test   optional row of `used` bytes (NULL: zeros); a row is KEPT iff (row ^ xor) & test == 0.
//   The pad bits of byte used - 1 (columns n_cols .. 8 used - 1) and the bytes used .. row_bytes - 1 of a row are not columns:
//   they may hold anything and are never counted, keyed or decoded.  Of the masks' pad bits: cut_pad() and below() take the
//   test mask's away before the comparison (pairs, rowtab, uf, ufw); k_tally compares the mask's whole bytes, so its caller
//   passes them as zero (include/tsim_hip.h, tsim_tally_rows_device).
//   Every address is formed in 64 bits (n x row_bytes may exceed 2^31).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bitrows {

constexpr int kChunk = 128;          // bytes of a row staged at a time in chunk mode (1024 columns)
constexpr int kStage = kChunk + 4;   // LDS bytes per staged row in chunk mode (33 dwords: lanes fall on distinct banks)

// keeps the compiler from moving LDS accesses of this wave across the point (the wave's LDS operations execute in order)
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes b0 .. b0 + nb - 1 of `rows` rows -> LDS.  contig: the rows' whole span (b0 = 0, LDS stride = rb); else one LDS
// row of kStage bytes per row.  w4: the row pointer and rb are multiples of 4 (b0 is a multiple of 8)
__device__ __forceinline__ void stage_rows(uint8_t *stage, const uint8_t *src, int rows, int b0, int nb, long long rb, int contig,
                                           int w4, int lane) {
  if (contig) {
    const int n = rows * (int)rb;
    int done = 0;
    if (w4) {
      const int nd = n >> 2;
      for (int i = lane; i < nd; i += 64) reinterpret_cast<uint32_t *>(stage)[i] = reinterpret_cast<const uint32_t *>(src)[i];
      done = nd << 2;
    }
    for (int i = done + lane; i < n; i += 64) stage[i] = src[i];
  } else if (w4) {  // (a dword that starts before nb ends inside the row: rb is a multiple of 4)
    constexpr int kDw = kChunk / 4;
    for (int i = lane; i < rows * kDw; i += 64) {
      const int r = i / kDw, k = (i % kDw) * 4;
      if (k < nb) *reinterpret_cast<uint32_t *>(stage + r * kStage + k) = *reinterpret_cast<const uint32_t *>(src + r * rb + b0 + k);
    }
  } else {
    for (int r = 0; r < rows; ++r)
      for (int k = lane; k < nb; k += 64) stage[r * kStage + k] = src[r * rb + b0 + k];
  }
}

// 8 bytes of a staged row (p 4-aligned when a4)
__device__ __forceinline__ uint64_t lds_word(const uint8_t *p, bool a4) {
  if (a4) return (uint64_t)reinterpret_cast<const uint32_t *>(p)[0] | ((uint64_t)reinterpret_cast<const uint32_t *>(p)[1] << 32);
  uint64_t w = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) w |= (uint64_t)p[q] << (8 * q);
  return w;
}

// bytes b .. b + 7 of a mask row of `used` bytes (0 past its end, 0 for no mask); b is wave-uniform
__device__ __forceinline__ uint64_t mask_word(const uint8_t *m, int b, int used) {
  if (!m) return 0;
  uint64_t w = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (b + q < used) w |= (uint64_t)m[b + q] << (8 * q);
  return w;
}

// the mask word tw of bytes b .. b + 7 without the pad bits of the last byte, which are not columns
__device__ __forceinline__ uint64_t cut_pad(uint64_t tw, int b, int n_cols) {
  const int past = (b + 8) * 8 - n_cols;
  if (past > 0) tw &= past >= 64 ? 0ull : (~0ull >> past);
  return tw;
}

// the bits of columns 8 b .. 8 b + 63 that are below column `end`
__device__ __forceinline__ uint64_t below(int b, int end) {
  const long long left = (long long)end - 8ll * b;
  return left <= 0 ? 0ull : left >= 64 ? ~0ull : ~0ull >> (64 - left);
}

// bytes b .. b + 7 of a row in global memory (0 past its `used` bytes); `R` has used and w8: the row pointer and the stride are
// multiples of 8
template <class R>
__device__ __forceinline__ uint64_t row_word(const R &a, const uint8_t *row, int b) {
  if (a.w8) return *reinterpret_cast<const uint64_t *>(row + b);  // (rb is a multiple of 8: inside the row)
  uint64_t w = 0;
  for (int q = 0; q < 8 && b + q < a.used; ++q) w |= (uint64_t)row[b + q] << (8 * q);
  return w;
}

// the observable columns obs_lo .. obs_hi - 1 of a row in global memory, bit i = column obs_lo + i; `R` has xr, obs_lo, obs_hi
template <class R>
__device__ __forceinline__ uint64_t row_obs(const R &a, const uint8_t *row) {
  uint64_t obs = 0;
  for (int c = a.obs_lo; c < a.obs_hi; ++c) {
    uint32_t byte = row[c >> 3];
    if (a.xr) byte ^= a.xr[c >> 3];
    obs |= (uint64_t)((byte >> (c & 7)) & 1u) << (c - a.obs_lo);
  }
  return obs;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l) << 32);
}

}  // namespace bitrows
