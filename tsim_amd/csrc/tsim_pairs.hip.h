// tsim_pairs.hip.h - pair counts over bit-packed rows: N[a][b] = kept rows with selected columns a and b both set, a
// binary X^T X.  Rows, xor, test and the keep rule are the row contract of tsim_bitrows.hip.h and the counts are taken over
// row ^ xor, as in k_tally (csrc/tsim_tally.hip.h): the diagonal is the tally's column counts.  Two kernels per slab of rows:
//   k_planes  one wave owns a tile of 64 rows (row r = lane r).  The rows go through LDS in chunks of kChunk bytes
//             (coalesced loads, dwords where the pointer and the stride allow).  Pass 1, only with a test mask: lane r
//             ORs (row ^ xor) & test over the chunks the mask touches.  Pass 2: per selected column one ballot turns
//             "lane r's bit" into the 64-bit shot mask of the tile (eight columns' LDS reads in flight: one at a time
//             the loop waits out the LDS latency per column); lane j keeps the mask of the j-th column of a run
//             of 64, XORs the reference bit, clears the rows that are not kept and stores the word.  The columns come
//             sorted (with the chunks that hold any listed), each with the slot it has in the caller's order.
//             Layout: plane[group][slot][kGroup] uint64, group = 16 tiles = 1024 rows: the words of one column and
//             group are one 128-byte line, and the k-chunk of a block of columns is one contiguous span.
//   k_gemm    popcount GEMM over the upper-triangle 64 x 64 tiles of the slot x slot matrix (blockIdx.x), the groups
//             of the slab dealt over blockIdx.y.  Per group the 64 + 64 planes (32 dwords each) are staged in LDS (row
//             stride 36 dwords: the 16 lanes of a 128-bit read fall on distinct banks) while the next group's are
//             already in flight to registers; a thread holds 4 x 4 uint32 accumulators (columns ty + 16 i, tx + 16 j)
//             and does v_and + v_bcnt per dword.  Each block ends with one 64-bit atomic add per non-zero accumulator:
//             integer adds commute, the counts do not depend on the schedule.  A launch covers at most 2^20 rows, so a
//             uint32 accumulator cannot overflow.  Tiles (ti, tj) with ti < tj are written at [a][b] only; the host
//             mirrors them on read.
// k_planes keeps a stager of its own (stage_chunk): bitrows::stage_rows in its place compiles to another kernel.
#pragma once
#include "tsim_bitrows.hip.h"

namespace pairsk {

using namespace bitrows;            // kChunk, kStage, wsync, mask_word, cut_pad (the stager is this file's own: stage_chunk)
constexpr int kWaves = 4;           // waves per k_planes block
constexpr int kGroup = 16;          // tiles per group: 1024 rows, 32 dwords per plane
constexpr int kWords = 2 * kGroup;  // dwords of a plane per group
constexpr int kPad = kWords + 4;    // LDS dwords per staged plane
constexpr int kTile = 64;           // columns per side of a k_gemm tile

struct PlaneArgs {
  const uint8_t *rows;
  long long n, rb;             // rows of the slab, row stride in bytes
  int n_cols, used;            // columns; bytes of a row that hold them
  const uint8_t *xr, *test;    // optional rows of `used` bytes (NULL: none)
  int k, kpad;                 // selected columns; slots of the workspace (k rounded up to kTile)
  const int32_t *scol, *sslot; // [k] the columns in ascending order, and the slot of each
  const int32_t *ach, *aoff;   // [n_ach] chunks with a selected column, [n_ach + 1] their ranges of scol
  int n_ach;
  int w4;                      // the row pointer and rb are multiples of 4
  unsigned long long *plane;   // [groups][kpad][kGroup]
};

struct GemmArgs {
  const uint32_t *plane;  // [groups][kpad][kWords]
  int kpad, k, groups;
  unsigned long long *counts;  // [k][k]
};

// bytes b0 .. b0 + nb - 1 of `rows` rows -> one LDS row of kStage bytes each
__device__ __forceinline__ void stage_chunk(uint8_t *stage, const uint8_t *src, int rows, int b0, int nb, long long rb, int w4, int lane) {
  if (w4) {  // (b0 is a multiple of 4; a dword that starts before nb ends inside the row: rb is a multiple of 4)
    const int ndw = (nb + 3) >> 2;
    for (int i = lane; i < rows * ndw; i += 64) {
      const int r = i / ndw, q = (i - r * ndw) * 4;
      *reinterpret_cast<uint32_t *>(stage + r * kStage + q) = *reinterpret_cast<const uint32_t *>(src + r * rb + b0 + q);
    }
  } else {
    for (int r = 0; r < rows; ++r)
      for (int q = lane; q < nb; q += 64) stage[r * kStage + q] = src[r * rb + b0 + q];
  }
}

__global__ void __launch_bounds__(64 * kWaves) k_planes(PlaneArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves][64 * kStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *stage = lds[wave];
  const long long t = (long long)blockIdx.x * kWaves + wave;  // (the grid covers whole groups: every word is written)
  const long long r0 = t << 6;
  const int rows = (int)max(0LL, min(64LL, a.n - r0));
  const uint8_t *src = a.rows + r0 * a.rb;
  const uint8_t *mine = stage + lane * kStage;
  bool kept = lane < rows;
  int staged = -1;
  // ---- pass 1: the keep mask
  if (a.test && rows > 0) {
    uint64_t fail = 0;
    const int n_ch = (a.used + kChunk - 1) / kChunk;
    for (int ch = 0; ch < n_ch; ++ch) {
      const int b0 = ch * kChunk, nb = min(kChunk, a.used - b0);
      const bool any = (lane < nb && a.test[b0 + lane]) || (lane + 64 < nb && a.test[b0 + lane + 64]);
      if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
      wsync();
      stage_chunk(stage, src, rows, b0, nb, a.rb, a.w4, lane);
      wsync();
      staged = ch;
      for (int g = 0; g * 8 < nb; ++g) {
        const int b = b0 + g * 8;
        uint64_t tw = mask_word(a.test, b, a.used);
        if (tw == 0) continue;
        tw = cut_pad(tw, b, a.n_cols);
        const uint64_t v = ((uint64_t)reinterpret_cast<const uint32_t *>(mine + g * 8)[0] |
                            ((uint64_t)reinterpret_cast<const uint32_t *>(mine + g * 8)[1] << 32)) ^ mask_word(a.xr, b, a.used);
        fail |= v & tw;
      }
    }
    kept = kept && fail == 0;
  }
  const uint64_t keep = __builtin_amdgcn_ballot_w64(kept);
  unsigned long long *out = a.plane + ((t / kGroup) * a.kpad) * kGroup + (t % kGroup);
  // ---- pass 2: one shot mask per selected column
  for (int m = 0; m < a.n_ach; ++m) {
    const int ch = a.ach[m], i_end = a.aoff[m + 1];
    const int b0 = ch * kChunk, nb = min(kChunk, a.used - b0);
    if (keep && staged != ch) {
      wsync();
      stage_chunk(stage, src, rows, b0, nb, a.rb, a.w4, lane);
      wsync();
      staged = ch;
    }
    for (int i0 = a.aoff[m]; i0 < i_end; i0 += 64) {
      const int cnt = min(64, i_end - i0);
      const int c = lane < cnt ? a.scol[i0 + lane] : b0 * 8;  // (a lane past the run reads the chunk's first byte)
      uint64_t word = 0;
      if (keep) {  // (no kept row: the words are zero, nothing staged is read)
        for (int j0 = 0; j0 < cnt; j0 += 8) {  // eight LDS reads in flight; the lanes past cnt keep words nobody stores
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int cj = __builtin_amdgcn_readlane(c, j0 + u);
            const uint32_t bit = ((uint32_t)mine[(cj >> 3) - b0] >> (cj & 7)) & 1u;
            const uint64_t shots = __builtin_amdgcn_ballot_w64(bit != 0u);
            word = lane == j0 + u ? shots : word;
          }
        }
        if (a.xr && lane < cnt && ((a.xr[c >> 3] >> (c & 7)) & 1)) word = ~word;
        word &= keep;
      }
      if (lane < cnt) out[(long long)a.sslot[i0 + lane] * kGroup] = word;
    }
  }
}

__global__ void __launch_bounds__(256) k_gemm(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t sA[kTile * kPad], sB[kTile * kPad];
  // tile pair (ti <= tj) of blockIdx.x, row by row of the upper triangle
  const int nt = a.kpad / kTile;
  int ti = 0, rest = blockIdx.x;
  while (rest >= nt - ti) {
    rest -= nt - ti;
    ++ti;
  }
  const int tj = ti + rest;
  const bool diag = ti == tj;
  const uint32_t *sBb = diag ? sA : sB;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  uint32_t acc[4][4] = {};
  // staging: the tile's planes of a group are 64 * 128 contiguous bytes = 512 uint4, two per thread and side
  const int q0 = tid, q1 = tid + 256;  // uint4 q: column q / 8, dwords 4 (q % 8) ..
  const int l0 = (q0 >> 3) * kPad + (q0 & 7) * 4, l1 = (q1 >> 3) * kPad + (q1 & 7) * 4;
  const long long gstride = (long long)a.kpad * kWords;
  const uint32_t *pa = a.plane + (long long)ti * kTile * kWords, *pb = a.plane + (long long)tj * kTile * kWords;
  uint4 ra0, ra1, rb0 = {}, rb1 = {};
  int g = blockIdx.y;
  if (g < a.groups) {
    ra0 = reinterpret_cast<const uint4 *>(pa + g * gstride)[q0];
    ra1 = reinterpret_cast<const uint4 *>(pa + g * gstride)[q1];
    if (!diag) {
      rb0 = reinterpret_cast<const uint4 *>(pb + g * gstride)[q0];
      rb1 = reinterpret_cast<const uint4 *>(pb + g * gstride)[q1];
    }
  }
  for (; g < a.groups; g += gridDim.y) {
    __syncthreads();  // (the previous group's reads are done)
    *reinterpret_cast<uint4 *>(sA + l0) = ra0;
    *reinterpret_cast<uint4 *>(sA + l1) = ra1;
    if (!diag) {
      *reinterpret_cast<uint4 *>(sB + l0) = rb0;
      *reinterpret_cast<uint4 *>(sB + l1) = rb1;
    }
    __syncthreads();
    const int gn = g + gridDim.y;
    if (gn < a.groups) {
      ra0 = reinterpret_cast<const uint4 *>(pa + gn * gstride)[q0];
      ra1 = reinterpret_cast<const uint4 *>(pa + gn * gstride)[q1];
      if (!diag) {
        rb0 = reinterpret_cast<const uint4 *>(pb + gn * gstride)[q0];
        rb1 = reinterpret_cast<const uint4 *>(pb + gn * gstride)[q1];
      }
    }
#pragma unroll 1
    for (int w = 0; w < kWords; w += 4) {
      uint4 x[4], y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const uint4 *>(sA + (ty + 16 * i) * kPad + w);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = *reinterpret_cast<const uint4 *>(sBb + (tx + 16 * j) * kPad + w);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] += __popc(x[i].x & y[j].x);
          acc[i][j] += __popc(x[i].y & y[j].y);
          acc[i][j] += __popc(x[i].z & y[j].z);
          acc[i][j] += __popc(x[i].w & y[j].w);
        }
    }
  }
  // ---- flush: one 64-bit global atomic per non-zero accumulator (16 lanes = 128 contiguous bytes of a row)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ca = ti * kTile + ty + 16 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cb = tj * kTile + tx + 16 * j;
      if (acc[i][j] && ca < a.k && cb < a.k) atomicAdd(&a.counts[(long long)ca * a.k + cb], (unsigned long long)acc[i][j]);
    }
  }
}

}  // namespace pairsk
