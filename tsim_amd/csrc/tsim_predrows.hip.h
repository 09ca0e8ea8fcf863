// tsim_predrows.hip.h - a decoder's predictions into the bit-packed rows they belong to (tsim_pred_rows_device).  Rows are
// those of the row contract of tsim_bitrows.hip.h; pred[r] is row r's prediction, bit k = column col0 + k, n_obs <= 64 columns.
//
// k_pred_rows: a lane per row, a persistent grid.  The range col0 .. col0 + n_obs - 1 lies in at most 9 bytes of the row and,
// when the row pointer and the stride are multiples of 8 (w8), in at most two of its 8-byte words: the prediction is shifted to
// its place as a 128-bit value and each word is read, changed and stored once; otherwise byte by byte.
//   XOR    row ^= prediction: a word (byte) whose share of the prediction is 0 is not stored, so a row that predicts no flip
//          is not written and nothing outside the range ever changes, pad bits and padding bytes included;
//   WRITE  the range is SET to the prediction and the other bits of the bytes col0 / 8 .. (col0 + n_obs - 1) / 8 are cleared
//          (whole bytes are stored; on the word path the bytes of the word outside those are kept).
// A row is owned by one lane and rows do not share a byte (nor, under w8, a word): plain loads and vector stores, no atomics.
// Every address is formed in 64 bits.
#pragma once
#include "tsim_bitrows.hip.h"

namespace predk {

constexpr int kWaves = 4;
enum { kXor = 0, kWrite = 1 };

struct Args {
  const unsigned long long *pred;  // [n]
  uint8_t *rows;
  long long n, rb;       // rows, row stride in bytes
  int col0, n_obs, mode;
  int w8;                // the row pointer and rb are multiples of 8
};

// the bits lo .. hi - 1 of a 64-bit word (0 <= lo, hi <= 64; empty for hi <= lo)
__device__ __forceinline__ uint64_t bit_span(int lo, int hi) {
  if (hi <= lo) return 0;
  return (hi >= 64 ? ~0ull : ((1ull << hi) - 1)) & ~((1ull << lo) - 1);  // (lo < hi <= 64: lo <= 63)
}

__global__ void __launch_bounds__(64 * kWaves) k_pred_rows(Args a) {
  const uint64_t keep = a.n_obs >= 64 ? ~0ull : ((1ull << a.n_obs) - 1);  // bits at and above n_obs are ignored
  const int b0 = a.col0 >> 3, b1 = (a.col0 + a.n_obs - 1) >> 3;          // the first and the last byte of the range
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (long long)gridDim.x * blockDim.x) {
    const uint64_t p = a.pred[r] & keep;
    if (a.mode == kXor && p == 0) continue;
    uint8_t *row = a.rows + r * a.rb;
    if (a.w8) {
      const int w0 = b0 >> 3, o = a.col0 & 63;  // the range starts at bit o of word w0
      uint64_t *w = reinterpret_cast<uint64_t *>(row) + w0;
      const uint64_t lo = p << o, hi = o ? p >> (64 - o) : 0ull;
      const bool two = o + a.n_obs > 64;  // (then word w0 + 1 holds columns of the range: it lies inside the row)
      if (a.mode == kXor) {
        if (lo) w[0] ^= lo;
        if (two && hi) w[1] ^= hi;
      } else {
        const int s = 8 * (b0 & 7), e = 8 * (b1 - 8 * w0 + 1);  // the bytes b0 .. b1 as bits of the words w0, w0 + 1
        w[0] = (w[0] & ~bit_span(s, min(e, 64))) | lo;
        if (two) w[1] = (w[1] & ~bit_span(0, e - 64)) | hi;
      }
    } else {
      const int sh = a.col0 & 7;
      for (int k = 0; k <= b1 - b0; ++k) {  // (at most 9 bytes; k >= 1: a shift of 8 k - sh in 1 .. 63)
        const uint32_t c = (uint32_t)(k == 0 ? p << sh : p >> (8 * k - sh)) & 255u;
        if (a.mode == kWrite) row[b0 + k] = (uint8_t)c;
        else if (c) row[b0 + k] ^= (uint8_t)c;
      }
    }
  }
}

}  // namespace predk
