// tsim_tally.hip.h - counts over bit-packed rows (k_tally): kept rows, kept rows with an observable set, one count per
// column over the kept rows, and a histogram over up to 16 columns of the kept rows.  Rows, xor, test and the keep rule are
// the row contract of tsim_bitrows.hip.h, whose reader this kernel uses; every count is taken over row ^ xor.  The test mask is
// compared in whole bytes: its pad bits must be zero (the one consumer that does not cut them).
//
// One wave owns a tile of 64 rows (row r of the tile = lane r) and runs it in two passes over LDS-staged bytes:
//   1. keep (only with a test mask, or for the observables): lane r ORs (row ^ xor) & test and (row ^ xor) & obs over
//      the byte range the test mask and the observable columns cover; its own row, read from LDS;
//   2. columns: per 64-bit word of the rows, one ballot per column turns "lane r's bit" into a 64-bit shot mask (rows
//      that are not kept are zero), its popcount is the tile's count of that column, and lane j keeps column j's
//      count; a word that is zero in every kept row costs one ballot.
// Staging: a tile of rows of at most kChunk bytes (and one window) is ONE contiguous span of rows x stride bytes; wider
// rows go through in kChunk-byte column chunks, one LDS row of kStage bytes each.  Dword loads where the pointer and
// the stride allow, byte loads otherwise.
// Per-block partials: uint32 in LDS (a launch covers fewer than 2^32 rows), added to with LDS atomics; at the end each
// block adds every non-zero partial to its uint64 counter with one global atomic.  Integer adds commute: the counts do
// not depend on the schedule.  Columns beyond `win` per block go through in windows (blockIdx.y): every window's blocks
// compute the keep mask; window 0's also count kept rows, observables and the histogram.
#pragma once
#include "tsim_bitrows.hip.h"

namespace tallyk {

using namespace bitrows;  // kChunk, kStage, wsync, stage_rows, lds_word, mask_word
constexpr int kMaxHist = 16;
constexpr int kMaxWaves = 4;

struct Args {
  const uint8_t *rows;
  long long n, rb;          // rows, row stride in bytes
  int n_cols, used;         // columns; bytes of a row that hold them
  const uint8_t *xr, *test; // optional rows of `used` bytes (NULL: none)
  int obs_lo, obs_hi;       // observable columns obs_lo .. obs_hi - 1 (empty: none)
  int n_hist;
  int hc[kMaxHist];         // histogram columns, bin bit i = column hc[i]
  unsigned long long *counts;  // [0] kept, [1] kept with an observable, [2 ..] columns, then 2^n_hist bins
  int win;                  // columns per window (a multiple of 64)
  int hist_lds;             // bins kept in LDS (else wave-aggregated global atomics)
  int contig, w4;           // stage a tile as one span; dword loads allowed
  int stage_bytes;          // LDS bytes of one wave's staging area
};

// bits lo .. hi - 1 of the 64 columns starting at cb
__device__ __forceinline__ uint64_t range_bits(int cb, int lo, int hi) {
  const int a = max(lo - cb, 0), b = min(hi - cb, 64);
  if (b <= a) return 0;
  const uint64_t upto = b >= 64 ? ~0ull : ((1ull << b) - 1);
  return upto & ~((1ull << a) - 1);
}

__global__ void __launch_bounds__(256) k_tally(Args a) {
  extern __shared__ uint64_t lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int n_bins = 1 << a.n_hist;
  uint32_t *part = reinterpret_cast<uint32_t *>(lds_raw);         // [win] column partials
  uint32_t *bins = part + a.win;                                     // [n_bins] when hist_lds
  uint32_t *slot = bins + (a.hist_lds ? (n_bins + 1) & ~1 : 0);      // kept, kept with observable, test lo / hi byte
  uint8_t *stage = reinterpret_cast<uint8_t *>(slot + 4) + (size_t)wave * a.stage_bytes;
  const int w = blockIdx.y;
  const bool first = w == 0;
  const int c0 = w * a.win, c1 = min(a.n_cols, c0 + a.win);
  for (int i = threadIdx.x; i < a.win; i += blockDim.x) part[i] = 0;
  if (a.hist_lds)
    for (int i = threadIdx.x; i < n_bins; i += blockDim.x) bins[i] = 0;
  if (threadIdx.x == 0) {
    slot[0] = slot[1] = 0;
    slot[2] = 0x7FFFFFFF;
    slot[3] = 0;
  }
  __syncthreads();
  if (a.test)  // the bytes the test mask covers
    for (int b = threadIdx.x; b < a.used; b += blockDim.x)
      if (a.test[b]) {
        atomicMin(&slot[2], (uint32_t)b);
        atomicMax(&slot[3], (uint32_t)b + 1);
      }
  __syncthreads();
  // the pass-1 byte range: the test mask's, and window 0 also reads the observables
  int plo = (int)min(slot[2], 0x7FFFFFFFu), phi = (int)slot[3];
  if (first && a.obs_hi > a.obs_lo) {
    plo = min(plo, a.obs_lo >> 3);
    phi = max(phi, (a.obs_hi + 7) >> 3);
  }
  plo &= ~7;
  const bool pass1 = phi > plo;
  unsigned long long kept_acc = 0, obs_acc = 0;  // wave-uniform
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * nw + wave; t < tiles; t += (long long)gridDim.x * nw) {
    const long long r0 = t << 6;
    const int rows = (int)min(64LL, a.n - r0);
    const uint8_t *src = a.rows + r0 * a.rb;
    const int ss = a.contig ? (int)a.rb : kStage;
    const uint8_t *mine = stage + lane * ss;
    const bool a4 = (ss & 3) == 0;
    bool kept = lane < rows;
    bool obs = false;
    if (a.contig) {
      wsync();
      stage_rows(stage, src, rows, 0, a.used, a.rb, 1, a.w4, lane);
      wsync();
    }
    // ---- pass 1: keep mask and observables
    if (pass1) {
      uint64_t fail = 0, seen = 0;
      for (int b0 = plo; b0 < phi; b0 += kChunk) {
        const int nb = min(kChunk, phi - b0);
        if (!a.contig) {
          wsync();
          stage_rows(stage, src, rows, b0, nb, a.rb, 0, a.w4, lane);
          wsync();
        }
        const uint8_t *p = a.contig ? mine + b0 : mine;
        for (int g = 0; g * 8 < nb; ++g) {
          const int b = b0 + g * 8;
          const uint64_t v = lds_word(p + g * 8, a4) ^ mask_word(a.xr, b, a.used);
          fail |= v & mask_word(a.test, b, a.used);
          if (first) seen |= v & range_bits(b * 8, a.obs_lo, a.obs_hi);
        }
      }
      kept = kept && fail == 0;
      obs = seen != 0;
    }
    const uint64_t keep = __builtin_amdgcn_ballot_w64(kept);
    if (first) {
      kept_acc += (unsigned long long)__popcll(keep);
      obs_acc += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(kept && obs));
      if (keep) {  // ---- histogram: lane's bin from its own row, lanes that share a bin add once
        uint32_t idx = 0;
        if (kept)
#pragma unroll
          for (int i = 0; i < kMaxHist; ++i) {  // (constant indices: the columns stay in the kernel arguments)
            if (i >= a.n_hist) break;
            const int c = a.hc[i];
            const uint32_t byte = src[(long long)lane * a.rb + (c >> 3)] ^ (a.xr ? a.xr[c >> 3] : 0u);
            idx |= ((byte >> (c & 7)) & 1u) << i;
          }
        uint64_t pending = keep;
        while (pending) {
          const int leader = __builtin_ctzll(pending);
          const uint32_t bin = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
          const uint64_t same = __builtin_amdgcn_ballot_w64(kept && idx == bin) & pending;
          if (lane == leader) {
            if (a.hist_lds) atomicAdd(&bins[bin], (uint32_t)__popcll(same));
            else atomicAdd(&a.counts[2 + a.n_cols + bin], (unsigned long long)__popcll(same));
          }
          pending &= ~same;
        }
      }
    }
    if (!keep) continue;
    // ---- pass 2: column counts of this window
    const int blo = c0 >> 3, bhi = (c1 + 7) >> 3;
    for (int b0 = blo; b0 < bhi; b0 += kChunk) {
      const int nb = min(kChunk, bhi - b0);
      if (!a.contig) {
        wsync();
        stage_rows(stage, src, rows, b0, nb, a.rb, 0, a.w4, lane);
        wsync();
      }
      const uint8_t *p = a.contig ? mine + b0 : mine;
      for (int g = 0; g * 8 < nb; ++g) {
        const int b = b0 + g * 8, cb = b * 8;
        uint64_t v = (lds_word(p + g * 8, a4) ^ mask_word(a.xr, b, a.used)) & range_bits(cb, c0, c1);
        if (!kept) v = 0;
        if (__builtin_amdgcn_ballot_w64(v != 0) == 0) continue;
        uint32_t cnt = 0;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
          const uint32_t byte = (uint32_t)(v >> (8 * i)) & 0xFFu;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(((byte >> jj) & 1u) != 0u));
            cnt = lane == 8 * i + jj ? c : cnt;
          }
        }
        if (cnt) atomicAdd(&part[cb - c0 + lane], cnt);  // (cnt != 0: column cb + lane is inside the window)
      }
    }
  }
  if (first && lane == 0) {
    if (kept_acc) atomicAdd(&slot[0], (uint32_t)kept_acc);
    if (obs_acc) atomicAdd(&slot[1], (uint32_t)obs_acc);
  }
  __syncthreads();
  // ---- flush: one 64-bit global atomic per non-zero partial
  for (int i = threadIdx.x; i < c1 - c0; i += blockDim.x)
    if (part[i]) atomicAdd(&a.counts[2 + c0 + i], (unsigned long long)part[i]);
  if (first) {
    if (a.hist_lds)
      for (int i = threadIdx.x; i < n_bins; i += blockDim.x)
        if (bins[i]) atomicAdd(&a.counts[2 + a.n_cols + i], (unsigned long long)bins[i]);
    if (threadIdx.x == 0) {
      if (slot[0]) atomicAdd(&a.counts[0], (unsigned long long)slot[0]);
      if (slot[1]) atomicAdd(&a.counts[1], (unsigned long long)slot[1]);
    }
  }
}

}  // namespace tallyk
