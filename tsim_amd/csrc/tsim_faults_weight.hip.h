// tsim_faults_weight.hip.h - fault-driven detector sampler, conditioned on exactly k fired sites: k_faults_weight.
//
// The geometry is k_faults' (tsim_faults.hip.h): one lane = one shot, a wave owns tiles of 64 shots whose rows live in LDS
// (S odd words per lane, private XOR, no atomic), the row initialisation, the firing of a site, the shot-major store, the
// col0 / n_cols contract and the column windows are its device functions; a window redraws the same pure-function stream.
// What differs is which sites fire (tsim_amd/fixed_weight.py states it in numpy).  With r = k sites to place, the classes in
// order: draw 0 of the class, x0, picks k_c from row (c, r) of the split table - the smallest m < min(r, n_c) with
// x0 < thr[m], min(r, n_c) when there is none; the last class takes k_c = r without a draw; r -= k_c.  Draws j = 1, 2, ...
// then give (x0, x1): t = x0 n_c (64 bits), pos = t >> 32; the draw is rejected when (t mod 2^32) < 2^32 mod n_c (Lemire:
// every position keeps floor(2^32 / n_c) values of x0) or when pos already fired in this shot and class; otherwise site pos
// fires under x1, until k_c sites have.  The rejection loop is a dependent Threefry chain as the gap walk is; lanes diverge
// in their draw counts and the wave leaves a class with its slowest lane.
// The split rows are indexed by the lane's own r: vector reads, from LDS when TAB_LDS (the outcome tables and the split table
// are copied in once per block; the gap rows are not needed), else from global memory.
// The positions that fired in the current class, at most kMaxWeight per lane, are a list in LDS: entry i of lane l at word
// i * 64 + l of the wave's list - a wave's access to entry i touches 64 consecutive words, every lane its own bank - so that
// no register array is indexed dynamically.  That is kMaxWeight * 256 bytes = 8 KiB per wave, next to its tile.
// Termination: k_c <= n_c always (m < min(r, n_c) by the loop bound; tsim_faults_set_split checks that no row can leave the
// later classes more than they hold, and k_c is clamped to n_c all the same), so a free position always exists: a draw is
// rejected by Lemire's rule with probability below n_c / 2^32 <= 2^-7 and otherwise hits a free position with probability
// (n_c - fired) / n_c >= 1 / 32 when the class is taken whole (n_c <= 32 then), far more in every other case.
#pragma once
#include "tsim_faults.hip.h"

namespace fltk {

constexpr int kMaxWeight = 32;                       // fixed_weight.MAX_FAULT_WEIGHT
constexpr int kListWords = kMaxWeight * 64;          // the fired-position list of one wave

struct WeightArgs {
  Args a;                  // n0, n1: the noise key of the fixed-weight stream; S, win, n_win: of this kernel's LDS rule
  const uint32_t *split;   // [n_classes][kmax + 1][kmax + 1]
  int k, kmax;
};

template <bool OUT_PACKED, bool TAB_LDS>
__global__ void __launch_bounds__(64 * kMaxWaves) k_faults_weight(WeightArgs W) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const Args &A = W.a;
  const Form &f = A.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int no_all = f.n_outcomes, kw = W.kmax + 1, n_split = f.n_classes * kw * kw;
  int tab_words = 0;
  if (TAB_LDS) {
    for (int i = threadIdx.x; i < no_all; i += blockDim.x) {
      lds[i] = f.out_thr[i];
      lds[no_all + i] = f.out_vals[i];
    }
    for (int i = threadIdx.x; i < n_split; i += blockDim.x) lds[2 * no_all + i] = W.split[i];
    tab_words = (2 * no_all + n_split + 3) & ~3;
    __syncthreads();
  }
  const uint32_t *l_thr = lds, *l_val = lds + no_all, *l_split = lds + 2 * no_all;
  uint32_t *tile = lds + tab_words + (size_t)wave * (64 * A.S + kListWords);
  uint32_t *mine = tile + lane * A.S;
  uint32_t *list = tile + 64 * A.S + lane;  // entry i: list[i * 64]
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
        int r = W.k;  // sites still to place
        for (int c = 0; c < f.n_classes && r > 0; ++c) {
          const int s0 = f.class_ptr[c], n_c = f.class_ptr[c + 1] - s0;
          const int o0 = f.table_ptr[c], no = f.table_ptr[c + 1] - o0;
          const uint32_t k0 = A.n0 ^ ((uint32_t)c * kClassFold), k1 = A.n1;
          // ---- the split: how many of the r sites this class takes
          int k_c = min(r, n_c);
          if (c < f.n_classes - 1) {
            uint32_t x0 = g_lo, x1 = g_hi;
            tsimk::threefry2x32(k0, k1, x0, x1);
            const int row = (c * kw + r) * kw;
            int m = 0;
            while (m < k_c && (TAB_LDS ? l_split[row + m] : W.split[row + m]) <= x0) ++m;
            k_c = m;
          }
          r -= k_c;
          // ---- k_c distinct positions of the class, each with its outcome
          const uint32_t reject = (0u - (uint32_t)n_c) % (uint32_t)n_c;  // 2^32 mod n_c
          int fired = 0;
          for (uint32_t j = 1; fired < k_c; ++j) {
            uint32_t x0 = g_lo, x1 = g_hi | (j << 6);
            tsimk::threefry2x32(k0, k1, x0, x1);
            const unsigned long long tt = (unsigned long long)x0 * (uint32_t)n_c;
            const uint32_t pos = (uint32_t)(tt >> 32);  // < n_c
            if ((uint32_t)tt < reject) continue;
            bool again = false;
            for (int i = 0; i < fired; ++i) again |= list[i * 64] == pos;
            if (again) continue;
            list[fired * 64] = pos;
            ++fired;
            fire_site<TAB_LDS>(mine, f, l_thr, l_val, o0, no, x1, f.site_e0[s0 + (int)pos], cb, wc);
          }
        }
      }
      m2dk::wsync();
      store_tile<OUT_PACKED>(tile, A.S, A.out, A.out_rb, A.out_w4, r0, rows, w0, wc, lane);
    }
  }
}

}  // namespace fltk
