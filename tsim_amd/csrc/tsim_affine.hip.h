// tsim_affine.hip.h - affine measurement sampler (k_affine): out_j = flip_j XOR (XOR of x_c over c in S_j), per shot, where
// column c < num_f is bit c of the shot's packed f row and column num_f + s is random symbol s of the shot.
//
// k_m2d's bit-sliced scheme (tsim_m2d.hip.h) with a second source of column masks.  One wave owns a tile of 64 shots:
//   1. the f columns of the window are staged in LDS and balloted into 64-bit shot masks exactly as k_m2d does for
//      bit-packed input; the random columns of the window are not loaded at all: the mask of symbol s over the 64 shots
//      of tile T is ONE Threefry block, w = x0 | x1 << 32 of threefry2x32(key, (s, T)) with T = first_shot / 64 + tile -
//      lane l computes the block of symbol 64 g + l, 64 symbols per pass;
//   2. m2dk::outputs: lane l XORs the masks of output l's CSR list, 64 ballots transpose back, coalesced stores.
// A shot's bit of symbol s is bit (global shot index % 64) of block (s, global shot index / 64): results depend on the
// key and the global shot index only, however a request is cut into launches (first_shot is a multiple of 64).
// Columns beyond one wave's LDS go through in windows like k_m2d's; a window may hold f columns, random columns or both.
#pragma once
#include "tsim_kernels.hip.h"
#include "tsim_m2d.hip.h"

namespace affk {

struct Args {
  m2dk::Args m;      // in = the f rows, M = num_f + n_random, in_used = bytes of an f row that hold the num_f bits
  int num_f;
  uint32_t k0, k1;   // key (hi, lo)
  long long tile0;   // first_shot / 64
};

template <bool OUT_PACKED>
__global__ void __launch_bounds__(256) k_affine(Args A) {
  extern __shared__ uint64_t lds[];
  const m2dk::Args &a = A.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint64_t *mask = lds + (size_t)wave * (a.win + m2dk::kStageBytes / 8);
  uint8_t *stage = reinterpret_cast<uint8_t *>(mask + a.win);
  const long long tiles = (a.B + 63) >> 6;
  for (long long t = (long long)blockIdx.x * nw + wave; t < tiles; t += (long long)gridDim.x * nw) {
    const long long r0 = t << 6;
    const int rows = (int)min(64LL, a.B - r0);
    const uint8_t *src = a.in + r0 * a.in_rb;
    uint8_t *dst = a.out + r0 * a.out_rb;
    const uint32_t tile = (uint32_t)(A.tile0 + t);  // < 2^32: first_shot + B <= 2^38
    for (int w = 0; w < a.n_win; ++w) {
      // columns c_lo .. c_lo + mw - 1 of this window: f columns below f_hi, random symbols from there on
      const int c_lo = w * a.win, mw = min(a.win, a.M - c_lo);
      const int f_hi = min(c_lo + mw, A.num_f), mf = f_hi - c_lo;
      const int32_t *rp = a.row_ptr + (long long)w * (a.n_out + 1);
      // ---- phase 1a: masks of the f columns (the last group of 64 may run into the random columns: 1b follows)
      m2dk::wsync();
      if (mf > 0) {
        if (a.in_contig) {  // (only with one window)
          m2dk::load_span(stage, src, rows * (int)a.in_rb, a.in_w4, lane);
          m2dk::wsync();
          m2dk::slice<true>(mask, stage + lane * (int)a.in_rb, 0, (mf + 63) >> 6, lane);
        } else {
          const int lo = c_lo / 8, hi = min(a.in_used, (f_hi + 7) / 8);
          for (int b0 = lo; b0 < hi; b0 += 64) {
            const int nb = min(64, hi - b0);
            m2dk::wsync();
            m2dk::load_rows(stage, src + b0, rows, nb, a.in_rb, a.in_w4, lane);  // (a dword past nb is still inside the row)
            m2dk::wsync();
            const int cb = b0 * 8 - c_lo;
            m2dk::slice<true>(mask, stage + lane * m2dk::kStageRow, cb, min(8, (mf - cb + 63) >> 6), lane);
          }
        }
      }
      m2dk::wsync();
      // ---- phase 1b: masks of the random columns, one Threefry block each
      for (int c = max(c_lo, A.num_f) + lane; c < c_lo + mw; c += 64) {
        uint32_t x0 = (uint32_t)(c - A.num_f), x1 = tile;
        tsimk::threefry2x32(A.k0, A.k1, x0, x1);
        mask[c - c_lo] = (uint64_t)x0 | ((uint64_t)x1 << 32);
      }
      m2dk::wsync();
      // ---- phase 2
      m2dk::outputs<OUT_PACKED>(a, rp, w > 0, mask, stage, dst, rows, lane);
    }
  }
}

}  // namespace affk
