// tsim_faults.hip.h - fault-driven detector sampler: k_faults.
//
// One lane = one shot.  A wave owns tiles of 64 consecutive shots (grid-stride) and keeps the tile's output rows in LDS, one
// row of S 32-bit words per lane (S odd: lanes that touch the same word of their rows hit different banks), bit r of a row =
// output col0 + w0 + r of the request.  A lane initialises its row from the outputs' constants, walks every class of the form
// (tsim_amd/faults.py) and XORs the column list of each error bit that fired into its OWN row: no atomic, in LDS or in HBM.
// The walk of class c for shot g (exact integer arithmetic, the tables faults.fault_rows_host reads): pos = -1; draw j:
// (x0, x1) = threefry2x32(class key, (g mod 2^32, (g >> 32) | (j << 6))); skip = #{k in 1..kGapK: x0 < gap[k - 1]} (gap
// decreases: one compare for skip == kGapK, else a binary search); skip == kGapK: pos += kGapK, draw again; else
// pos += skip + 1, done when pos >= n_c, else site pos fires with the first outcome whose threshold exceeds x1 (the last one
// when none does).  The walk stops as soon as pos >= n_c - 1 (the next draw could only end it).  Lanes diverge in their draw
// counts; the wave leaves a class when its last lane has.
// TAB_LDS: the gap rows and outcome tables are copied into the block's LDS once (a few KiB per distinct fire probability);
// forms whose tables exceed kTabLdsBytes read them from global memory.
// The tile is already shot-major: it is stored with consecutive lanes on consecutive dwords (bytes where the buffer's
// alignment or a row's tail asks for it), bit-packed as it lies or a byte per bit; bytes of a row past out_used are not
// written, pad bits of the last byte are zero.  Outputs beyond what one wave's LDS holds go through in windows of `win`
// columns: the same draws again (they are a pure function of key, class, g and j), keeping the columns inside the window.
// Every global address is formed in 64 bits.
#pragma once
#include "tsim_kernels.hip.h"
#include "tsim_m2d.hip.h"

namespace fltk {

constexpr int kGapK = 1024;               // entries of a gap row: a constant of the stream (faults.K_GAP)
constexpr uint32_t kClassFold = 0x9E3779B9u;
constexpr int kMaxWaves = 8;
constexpr int kTabLdsBytes = 32 * 1024;   // tables up to this size live in LDS

struct Form {
  const int32_t *class_ptr, *site_e0, *table_ptr, *table_gap;
  const uint32_t *out_vals, *out_thr, *gap_thr;
  const int32_t *col_ptr, *cols;
  const uint32_t *const_words;  // the outputs' constants, 32 to a word, two zero words after the last
  int n_classes, n_gaps, n_outcomes;
};

struct Args {
  Form f;
  long long B, g0;        // shots of this launch, global index of the first
  uint32_t n0, n1;        // the request's noise key
  uint8_t *out;
  long long out_rb;       // output row stride in bytes
  int out_w4;             // dword stores allowed (row stride and buffer 4-aligned)
  int col0, n_cols;       // outputs col0 .. col0 + n_cols - 1
  int S;                  // words per LDS row (odd)
  int win, n_win;         // columns per window (a multiple of 32), windows of this request
};

// ---- the pieces of a tile's work that k_faults and k_faults_weight (tsim_faults_weight.hip.h) share

// the row starts as the constants of the outputs cb .. cb + wc - 1, pad bits zero
__device__ __forceinline__ void row_init(uint32_t *mine, const Form &f, int cb, int wc) {
  const uint32_t *cw = f.const_words + (cb >> 5);
  const int sh = cb & 31, n_words = (wc + 31) >> 5;
  for (int i = 0; i < n_words; ++i) {
    uint32_t v = sh ? (cw[i] >> sh) | (cw[i + 1] << (32 - sh)) : cw[i];
    const int left = wc - 32 * i;
    if (left < 32) v &= (1u << left) - 1u;
    mine[i] = v;
  }
}

// a site with first error bit e0 fires under x1: the first outcome of its table (o0 .. o0 + no - 1; l_thr / l_val: the
// tables in LDS) whose threshold exceeds x1, the last one when none does; the column lists of its error bits go into the row
template <bool TAB_LDS>
__device__ __forceinline__ void fire_site(uint32_t *mine, const Form &f, const uint32_t *l_thr, const uint32_t *l_val, int o0, int no,
                                          uint32_t x1, int e0, int cb, int wc) {
  int o = 0;
  while (o < no - 1 && (TAB_LDS ? l_thr[o0 + o] : f.out_thr[o0 + o]) <= x1) ++o;
  uint32_t v = TAB_LDS ? l_val[o0 + o] : f.out_vals[o0 + o];
  while (v) {
    const int e = e0 + __ffs((int)v) - 1;
    v &= v - 1u;
    const int t1 = f.col_ptr[e + 1];
    for (int k = f.col_ptr[e]; k < t1; ++k) {
      const uint32_t r = (uint32_t)(f.cols[k] - cb);
      if (r < (uint32_t)wc) mine[r >> 5] ^= 1u << (r & 31);
    }
  }
}

// the store of `rows` rows of a tile (S words each), columns w0 .. w0 + wc - 1 of the request: lanes run over (row, dword)
// pairs, the dword fastest
template <bool OUT_PACKED>
__device__ __forceinline__ void store_tile(const uint32_t *tile, int S, uint8_t *out, long long out_rb, int out_w4, long long r0, int rows,
                                           int w0, int wc, int lane) {
  if (OUT_PACKED) {
    uint8_t *dst = out + r0 * out_rb + (w0 >> 3);
    const int nb = (wc + 7) >> 3, nd = out_w4 ? nb >> 2 : 0, rem = nb - 4 * nd;
    for (int i = lane; i < rows * nd; i += 64) {
      const int r = i / nd, k = i - r * nd;
      *reinterpret_cast<uint32_t *>(dst + (long long)r * out_rb + 4 * k) = tile[r * S + k];
    }
    for (int i = lane; i < rows * rem; i += 64) {
      const int r = i / rem, k = 4 * nd + i - r * rem;
      dst[(long long)r * out_rb + k] = (uint8_t)(tile[r * S + (k >> 2)] >> (8 * (k & 3)));
    }
  } else {
    uint8_t *dst = out + r0 * out_rb + w0;
    const int nq = out_w4 ? wc >> 2 : 0, rem = wc - 4 * nq;
    for (int i = lane; i < rows * nq; i += 64) {
      const int r = i / nq, q = i - r * nq;
      const uint32_t b = tile[r * S + (q >> 3)] >> (4 * (q & 7));
      *reinterpret_cast<uint32_t *>(dst + (long long)r * out_rb + 4 * q) =
          (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
    }
    for (int i = lane; i < rows * rem; i += 64) {
      const int r = i / rem, k = 4 * nq + i - r * rem;
      dst[(long long)r * out_rb + k] = (uint8_t)((tile[r * S + (k >> 5)] >> (k & 31)) & 1u);
    }
  }
}

template <bool OUT_PACKED, bool TAB_LDS>
__global__ void __launch_bounds__(64 * kMaxWaves) k_faults(Args A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const Form &f = A.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int n_gap_words = f.n_gaps * kGapK, no_all = f.n_outcomes;
  int tab_words = 0;
  if (TAB_LDS) {
    for (int i = threadIdx.x; i < n_gap_words; i += blockDim.x) lds[i] = f.gap_thr[i];
    for (int i = threadIdx.x; i < no_all; i += blockDim.x) {
      lds[n_gap_words + i] = f.out_thr[i];
      lds[n_gap_words + no_all + i] = f.out_vals[i];
    }
    tab_words = (n_gap_words + 2 * no_all + 3) & ~3;
    __syncthreads();
  }
  const uint32_t *l_gap = lds, *l_thr = lds + n_gap_words, *l_val = lds + n_gap_words + no_all;
  uint32_t *tile = lds + tab_words + (size_t)wave * 64 * A.S;
  uint32_t *mine = tile + lane * A.S;
  const long long tiles = (A.B + 63) >> 6;
  for (long long t = (long long)blockIdx.x * nw + wave; t < tiles; t += (long long)gridDim.x * nw) {
    const long long r0 = t << 6;
    const int rows = (int)min(64LL, A.B - r0);
    const unsigned long long g = (unsigned long long)(A.g0 + r0 + lane);  // < 2^38
    const uint32_t g_lo = (uint32_t)g, g_hi = (uint32_t)(g >> 32);
    for (int w = 0; w < A.n_win; ++w) {
      const int w0 = w * A.win, wc = min(A.win, A.n_cols - w0), cb = A.col0 + w0;
      m2dk::wsync();  // (the store of the previous tile or window has read the rows)
      if (lane < rows) {
        row_init(mine, f, cb, wc);
        // ---- the walk
        for (int c = 0; c < f.n_classes; ++c) {
          const int s0 = f.class_ptr[c], n_c = f.class_ptr[c + 1] - s0;
          const int o0 = f.table_ptr[c], no = f.table_ptr[c + 1] - o0;
          const int gb = f.table_gap[c] * kGapK;
          const uint32_t k0 = A.n0 ^ ((uint32_t)c * kClassFold), k1 = A.n1;
          const uint32_t gap_last = TAB_LDS ? l_gap[gb + kGapK - 1] : f.gap_thr[gb + kGapK - 1];
          int pos = -1;
          for (uint32_t j = 0; pos < n_c - 1; ++j) {
            uint32_t x0 = g_lo, x1 = g_hi | (j << 6);
            tsimk::threefry2x32(k0, k1, x0, x1);
            if (x0 < gap_last) {  // every entry is above x0: nothing fires in the next kGapK sites
              pos += kGapK;
              continue;
            }
            int lo = 0, hi = kGapK - 1;  // the first index whose entry is <= x0 = the number of entries above x0
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (x0 < (TAB_LDS ? l_gap[gb + mid] : f.gap_thr[gb + mid])) lo = mid + 1;
              else hi = mid;
            }
            pos += lo + 1;
            if (pos >= n_c) break;
            fire_site<TAB_LDS>(mine, f, l_thr, l_val, o0, no, x1, f.site_e0[s0 + pos], cb, wc);
          }
        }
      }
      m2dk::wsync();
      store_tile<OUT_PACKED>(tile, A.S, A.out, A.out_rb, A.out_w4, r0, rows, w0, wc, lane);
    }
  }
}

}  // namespace fltk
