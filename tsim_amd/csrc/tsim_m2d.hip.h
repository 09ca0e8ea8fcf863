// tsim_m2d.hip.h - measurements -> detection events (k_m2d): out_j = ref_j XOR (XOR of m_k over k in S_j), per shot.
//
// One wave owns a tile of 64 shots (row r of the tile = lane r) and runs it in two phases:
//   1. bit-slice: the tile's input rows are staged in LDS with coalesced loads, then one ballot per measurement column
//      turns "lane r's bit of column c" into a 64-bit shot mask; the masks of all M columns stay in the wave's LDS;
//   2. outputs, 64 at a time: lane l forms the shot mask of output l as the XOR of the masks of its CSR column list,
//      inverted when ref_l = 1; 64 more ballots transpose the block back (ballot j = shot j's 64 output bits), the bits
//      are assembled into the output rows in LDS and written out with coalesced stores.
// Staging: a tile whose rows are at most kStageRow bytes apart is ONE contiguous span of rows x stride bytes (rows are
// dense in the buffer), loaded as dwords when the pointer allows; wider rows go through in 64-byte column chunks, one
// LDS row of kStageRow bytes each.  Unpacked input is decoded in the same pass (ballot of byte != 0).
// Records beyond what one wave's LDS holds go through in windows of `win` columns: phase 1 builds the window's masks,
// phase 2 XORs the window's part of every output (a CSR per window, window-local column indices) into the rows the
// earlier windows wrote - chunks and 64-output groups without a record in the window are skipped.
// Every address is formed in 64 bits (B x row bytes may exceed 2^31).  Phase 2 is a function of its own (outputs): the affine
// measurement sampler (tsim_affine.hip.h) builds its masks differently and shares it.
#pragma once
#include "tsim_bitrows.hip.h"

namespace m2dk {

constexpr int kStageRow = 68;                        // LDS bytes per staged row in chunk mode (64 + a dword of padding)
constexpr int kStageBytes = 64 * kStageRow + 64;     // + slack for the 8-byte column groups that run past the last row
constexpr int kMaxWaves = 4;

struct Args {
  const uint8_t *in;
  long long B, in_rb;     // rows, input row stride in bytes
  int M, in_used;         // measurement columns, bytes of a row that hold them
  int in_contig, in_w4;   // stage the tile as one span; dword loads allowed
  const int32_t *row_ptr, *cols;
  const uint8_t *ref;
  int col0, n_cols;       // outputs col0 .. col0 + n_cols - 1
  uint8_t *out;
  long long out_rb;       // output row stride in bytes
  int out_used;           // bytes of a row that are written
  int out_contig, out_w4;
  int n_out;              // outputs of the handle (stride of the per-window row_ptr arrays)
  int win, n_win;         // columns per window (masks per wave, a multiple of 512 when n_win > 1), windows
};

using bitrows::wsync;  // (csrc/tsim_bitrows.hip.h; the samplers that share this file call it as m2dk::wsync)

// n contiguous bytes global -> LDS (dwords when w4: src and dst 4-aligned)
__device__ __forceinline__ void load_span(uint8_t *stage, const uint8_t *src, int n, int w4, int lane) {
  int done = 0;
  if (w4) {
    const int nd = n >> 2;
    for (int i = lane; i < nd; i += 64) reinterpret_cast<uint32_t *>(stage)[i] = reinterpret_cast<const uint32_t *>(src)[i];
    done = nd << 2;
  }
  for (int i = done + lane; i < n; i += 64) stage[i] = src[i];
}

// LDS -> n contiguous bytes global
__device__ __forceinline__ void store_span(uint8_t *dst, const uint8_t *stage, int n, int w4, int lane) {
  int done = 0;
  if (w4) {
    const int nd = n >> 2;
    for (int i = lane; i < nd; i += 64) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(stage)[i];
    done = nd << 2;
  }
  for (int i = done + lane; i < n; i += 64) dst[i] = stage[i];
}

// `rows` rows of nb <= 64 bytes (source stride rb) -> LDS rows of kStageRow bytes.  w4: rb and src are multiples of 4
__device__ __forceinline__ void load_rows(uint8_t *stage, const uint8_t *src, int rows, int nb, long long rb, int w4, int lane) {
  if (w4) {
    for (int i = lane; i < rows * 16; i += 64) {
      const int r = i >> 4, k = (i & 15) << 2;
      if (k < nb) *reinterpret_cast<uint32_t *>(stage + r * kStageRow + k) = *reinterpret_cast<const uint32_t *>(src + r * rb + k);
    }
  } else {
    for (int r = 0; r < rows; ++r)
      if (lane < nb) stage[r * kStageRow + lane] = src[r * rb + lane];
  }
}

__device__ __forceinline__ void store_rows(uint8_t *dst, const uint8_t *stage, int rows, int nb, long long rb, int w4, int lane) {
  if (w4) {
    for (int i = lane; i < rows * 16; i += 64) {
      const int r = i >> 4, k = (i & 15) << 2;
      if (k < nb) *reinterpret_cast<uint32_t *>(dst + r * rb + k) = *reinterpret_cast<const uint32_t *>(stage + r * kStageRow + k);
    }
  } else {
    for (int r = 0; r < rows; ++r)
      if (lane < nb) dst[r * rb + lane] = stage[r * kStageRow + lane];
  }
}

// lane j of `v` := the wave-uniform m.  Callers pass j = 8 i + jj with i a loop variable kept rolled: the 64 compares
// lane == j would otherwise be hoisted out of every loop and held in SGPRs all at once.
__device__ __forceinline__ void put_lane(uint64_t &v, uint64_t m, int lane, int j) { v = lane == j ? m : v; }

// Phase 1 on one staged chunk: `ng` groups of 64 columns starting at column cb; lane's row starts at `row` in LDS.
template <bool IN_PACKED>
__device__ __forceinline__ void slice(uint64_t *mask, const uint8_t *row, int cb, int ng, int lane) {
  for (int g = 0; g < ng; ++g) {
    uint64_t mine = 0;
    if (IN_PACKED) {
      uint64_t bits = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) bits |= (uint64_t)row[g * 8 + q] << (8 * q);
#pragma unroll 1
      for (int i = 0; i < 8; ++i) {
        const uint32_t byte = (uint32_t)(bits >> (8 * i)) & 0xFFu;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) put_lane(mine, __builtin_amdgcn_ballot_w64(((byte >> jj) & 1u) != 0u), lane, 8 * i + jj);
      }
    } else {
#pragma unroll 1
      for (int i = 0; i < 8; ++i) {
        const uint8_t *p = row + g * 64 + 8 * i;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) put_lane(mine, __builtin_amdgcn_ballot_w64(p[jj] != 0), lane, 8 * i + jj);
      }
    }
    mask[cb + g * 64 + lane] = mine;
  }
}

// Phase 2 on one tile: outputs a.col0 .. a.col0 + a.n_cols - 1 from the column masks in `mask` and the CSR of one window
// (`rp`: its row_ptr, window-local indices in a.cols); xr: XOR into the rows already at dst (a later window).
template <bool OUT_PACKED>
__device__ __forceinline__ void outputs(const Args &a, const int32_t *rp, bool xr, const uint64_t *mask, uint8_t *stage, uint8_t *dst,
                                        int rows, int lane) {
  constexpr int kPerChunk = OUT_PACKED ? 512 : 64;
  for (int o0 = 0; o0 < a.n_cols; o0 += kPerChunk) {
    const int o1 = min(o0 + kPerChunk, a.n_cols);
    if (xr && rp[a.col0 + o0] == rp[a.col0 + o1]) continue;  // no record of this window in the chunk
    const int ss = a.out_contig ? (int)a.out_rb : kStageRow;
    const int b0 = OUT_PACKED ? o0 / 8 : o0;
    const int nb = min(64, a.out_used - b0);
    if (xr) {  // the rows as the earlier windows left them
      if (a.out_contig) load_span(stage, dst, rows * (int)a.out_rb, a.out_w4, lane);
      else load_rows(stage, dst + b0, rows, nb, a.out_rb, a.out_w4 && !(nb & 3), lane);
      wsync();
    }
    uint8_t *mine = stage + lane * ss;
    for (int g = 0; g < kPerChunk / 64; ++g) {
      const int ob = o0 + g * 64;
      if (ob >= a.n_cols) break;
      if (xr && rp[a.col0 + ob] == rp[a.col0 + min(ob + 64, a.n_cols)]) continue;
      // lane l forms the shot mask of output ob + l (its own CSR list), then 64 ballots transpose the 64 x 64 bit block:
      // ballot j collects bit j (shot j) of every lane's output mask, i.e. shot j's 64 output bits
      uint64_t acc = 0;
      const int o = ob + lane;
      if (o < a.n_cols) {
        const int q = a.col0 + o;
        acc = (!xr && a.ref[q]) ? ~0ull : 0ull;
        const int k1 = rp[q + 1];
        for (int k = rp[q]; k < k1; ++k) acc ^= mask[a.cols[k]];
      }
      uint64_t word = 0;
#pragma unroll 1
      for (int i = 0; i < 8; ++i) {
        const uint32_t byte = (uint32_t)(acc >> (8 * i)) & 0xFFu;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) put_lane(word, __builtin_amdgcn_ballot_w64(((byte >> jj) & 1u) != 0u), lane, 8 * i + jj);
      }
      const uint32_t wlo = (uint32_t)word, whi = (uint32_t)(word >> 32);
      if (OUT_PACKED) {
        if (a.out_contig) {
#pragma unroll
          for (int q = 0; q < 8; ++q)  // the row is out_rb bytes: the next lane's row starts there
            if (g * 8 + q < ss) {
              const uint8_t v = (uint8_t)((q < 4 ? wlo : whi) >> (8 * (q & 3)));
              mine[g * 8 + q] = xr ? (uint8_t)(mine[g * 8 + q] ^ v) : v;
            }
        } else {
          uint32_t *p = reinterpret_cast<uint32_t *>(mine + g * 8);
          p[0] = xr ? p[0] ^ wlo : wlo;
          p[1] = xr ? p[1] ^ whi : whi;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const uint32_t wq = q < 8 ? wlo >> (4 * q) : whi >> (4 * (q - 8));
          const uint32_t v = (wq & 1u) | ((wq & 2u) << 7) | ((wq & 4u) << 14) | ((wq & 8u) << 21);
          if (a.out_contig) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (4 * q + k < ss) {
                const uint8_t vb = (uint8_t)(v >> (8 * k));
                mine[4 * q + k] = xr ? (uint8_t)(mine[4 * q + k] ^ vb) : vb;
              }
          } else {
            uint32_t *p = reinterpret_cast<uint32_t *>(mine + 4 * q);
            *p = xr ? *p ^ v : v;
          }
        }
      }
    }
    wsync();
    if (a.out_contig) store_span(dst, stage, rows * (int)a.out_rb, a.out_w4, lane);
    else store_rows(dst + b0, stage, rows, nb, a.out_rb, a.out_w4 && !(nb & 3), lane);
    wsync();
  }
}

template <bool IN_PACKED, bool OUT_PACKED>
__global__ void __launch_bounds__(256) k_m2d(Args a) {
  extern __shared__ uint64_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint64_t *mask = lds + (size_t)wave * (a.win + kStageBytes / 8);
  uint8_t *stage = reinterpret_cast<uint8_t *>(mask + a.win);
  const long long tiles = (a.B + 63) >> 6;
  for (long long t = (long long)blockIdx.x * nw + wave; t < tiles; t += (long long)gridDim.x * nw) {
    const long long r0 = t << 6;
    const int rows = (int)min(64LL, a.B - r0);
    const uint8_t *src = a.in + r0 * a.in_rb;
    uint8_t *dst = a.out + r0 * a.out_rb;
    for (int w = 0; w < a.n_win; ++w) {
      // columns c_lo .. c_lo + mw - 1 of this window; its CSR holds window-local column indices
      const int c_lo = w * a.win, mw = min(a.win, a.M - c_lo);
      const int32_t *rp = a.row_ptr + (long long)w * (a.n_out + 1);
      const bool xr = w > 0;  // later windows XOR their part into the rows the earlier ones wrote
      // ---- phase 1: column masks
      wsync();
      if (mw > 0) {
        if (a.in_contig) {  // (only with one window: rows of at most kStageRow bytes hold at most 544 columns)
          load_span(stage, src, rows * (int)a.in_rb, a.in_w4, lane);
          wsync();
          slice<IN_PACKED>(mask, stage + lane * (int)a.in_rb, 0, (mw + 63) >> 6, lane);
        } else {
          const int lo = IN_PACKED ? c_lo / 8 : c_lo, hi = IN_PACKED ? min(a.in_used, (c_lo + mw + 7) / 8) : c_lo + mw;
          for (int b0 = lo; b0 < hi; b0 += 64) {
            const int nb = min(64, hi - b0);
            wsync();
            load_rows(stage, src + b0, rows, nb, a.in_rb, a.in_w4, lane);  // (a dword past nb is still inside the row)
            wsync();
            const int cb = (IN_PACKED ? b0 * 8 : b0) - c_lo;
            const int ng = IN_PACKED ? min(8, (mw - cb + 63) >> 6) : 1;
            slice<IN_PACKED>(mask, stage + lane * kStageRow, cb, ng, lane);
          }
        }
      }
      wsync();
      // ---- phase 2: outputs, one chunk of 64 bytes per row at a time
      outputs<OUT_PACKED>(a, rp, xr, mask, stage, dst, rows, lane);
    }
  }
}

}  // namespace m2dk
