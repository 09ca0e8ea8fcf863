// tsim_frame.hip.h - Pauli-frame sampler: k_frame (propagation) and k_frame_out (output stage).
//
// k_frame.  A block owns a tile of T 64-shot words and carries the frames x[q][T], z[q][T] (uint64, one bit per shot) in LDS
// through the operation list of the form (tsim_amd/frame.py): H swaps x and z, S z ^= x, CX x_t ^= x_c and z_c ^= z_t, RESET
// clears, MEASURE stores x_q as the record's flip word, FEEDBACK XORs a record's flip word into x_q and / or z_q, NOISE draws
// a site for one word and XORs the outcome's bits into their targets.  The list is cut into batches of one kind whose items
// touch pairwise disjoint qubits and records: the block reads the batch list uniformly, spreads (item, word) pairs over its
// threads (256 .. 1024, by the items of the largest batch) and separates batches with a barrier - a thread owns its word of
// its item's qubits and records, so there is no atomic, in LDS or in HBM.  Record flip words live in the record-major scratch F[record][word] in HBM (row stride: the
// words of a launch); a batch that reads a record (FEEDBACK, a NOISE site with a record target) runs after the barrier that
// follows the batch that wrote it.  Words of the tile past the launch's last word are skipped.
// The draw of a site for the word tau (exact integer arithmetic, the same tables as frame.draw_site): pos = -1; draw j:
// (x0, x1) = threefry2x32(site key, (tau, j)); skip = #{k in 1..64: x0 < gap[k - 1]} (gap decreases: a binary search);
// pos += skip + 1; done when pos > 63; else shot pos fires with the first outcome whose threshold exceeds x1 (the last one when
// none does).  At most 64 draws.
//
// k_frame_out.  k_affine (tsim_affine.hip.h) with another source of column masks: columns are [records | random symbols], the
// mask of a record column over a wave's 64 shots is ONE word of F, the mask of a symbol column one Threefry block.  Phase 2
// is m2dk::outputs, unchanged, windows beyond one wave's LDS included.
#pragma once
#include "tsim_kernels.hip.h"
#include "tsim_m2d.hip.h"

namespace frmk {

enum : int { kH = 0, kS = 1, kCX = 2, kReset = 3, kMeasure = 4, kFeedback = 5, kNoise = 6 };
constexpr int kMaxThreads = 1024;  // a block: 4 .. 16 waves, by the items of the largest batch (tsim_frame.hip)
constexpr uint32_t kSiteFold = 0x9E3779B9u;

struct Form {
  const uint8_t *op_kind;
  const int32_t *op_a, *op_b, *op_c, *batch_ptr;
  const int32_t *site_chan, *site_table, *site_bit, *bit_ptr, *targets, *table_ptr, *table_gap;
  const uint32_t *out_vals, *out_thr, *gap_thr;
  int n_batches, nq;
};

struct Args {
  Form f;
  uint64_t *F;          // [records + hidden records][stride]
  long long stride;     // words per row of F
  long long words;      // words of this launch (<= stride)
  long long tile0;      // global index of the launch's first word
  int log2T;
  uint32_t n0, n1;      // the request's noise key
};

__device__ __forceinline__ void draw_site(const Form &f, int s, uint32_t n0, uint32_t n1, uint32_t tau, uint64_t *xw, uint64_t *zw, int T,
                                          uint64_t *Fw, long long stride) {
  const int tab = f.site_table[s];
  const uint32_t *gap = f.gap_thr + 64 * f.table_gap[tab];
  const int o0 = f.table_ptr[tab], no = f.table_ptr[tab + 1] - o0;
  const int b0 = f.site_bit[s];
  const uint32_t k0 = n0 ^ ((uint32_t)f.site_chan[s] * kSiteFold), k1 = n1;
  int pos = -1;
  for (uint32_t j = 0; j < 64u; ++j) {
    uint32_t x0 = tau, x1 = j;
    tsimk::threefry2x32(k0, k1, x0, x1);
    if (x0 < gap[63]) break;  // every entry is above x0: skip = 64 (nearly every draw of a rare channel ends here)
    int lo = 0, hi = 63;  // the first index whose entry is <= x0 = the number of entries above x0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (x0 < gap[mid]) lo = mid + 1;
      else hi = mid;
    }
    pos += lo + 1;
    if (pos > 63) break;
    int o = 0;
    while (o < no - 1 && f.out_thr[o0 + o] <= x1) ++o;
    uint32_t v = f.out_vals[o0 + o];
    const uint64_t bit = 1ull << pos;
    while (v) {
      const int i = __ffs((int)v) - 1;
      v &= v - 1u;
      for (int t = f.bit_ptr[b0 + i]; t < f.bit_ptr[b0 + i + 1]; ++t) {
        const int tg = f.targets[t], idx = tg >> 2, kind = tg & 3;
        if (kind == 0) xw[(size_t)idx * T] ^= bit;
        else if (kind == 1) zw[(size_t)idx * T] ^= bit;
        else Fw[(long long)idx * stride] ^= bit;
      }
    }
  }
}

__global__ void __launch_bounds__(kMaxThreads) k_frame(Args A) {
  extern __shared__ uint64_t frames[];
  const Form &f = A.f;
  const int T = 1 << A.log2T, nq = f.nq, nt = blockDim.x;
  uint64_t *x = frames, *z = frames + (size_t)nq * T;
  const long long w0 = (long long)blockIdx.x << A.log2T;
  const int tw = (int)min((long long)T, A.words - w0);  // words of this tile inside the launch
  for (int i = threadIdx.x; i < 2 * nq * T; i += nt) frames[i] = 0;
  __syncthreads();
  for (int b = 0; b < f.n_batches; ++b) {
    const int lo = f.batch_ptr[b], n = (f.batch_ptr[b + 1] - lo) << A.log2T;
    const int kind = f.op_kind[lo];
    for (int p = threadIdx.x; p < n; p += nt) {
      const int item = lo + (p >> A.log2T), w = p & (T - 1);
      if (w >= tw) continue;
      const int a = f.op_a[item];
      uint64_t *Fw = A.F + (w0 + w);
      switch (kind) {
        case kH: {
          const uint64_t t = x[a * T + w];
          x[a * T + w] = z[a * T + w];
          z[a * T + w] = t;
        } break;
        case kS: z[a * T + w] ^= x[a * T + w]; break;
        case kCX: {
          const int t = f.op_b[item];
          x[t * T + w] ^= x[a * T + w];
          z[a * T + w] ^= z[t * T + w];
        } break;
        case kReset:
          x[a * T + w] = 0;
          z[a * T + w] = 0;
          break;
        case kMeasure: Fw[(long long)f.op_b[item] * A.stride] = a >= 0 ? x[a * T + w] : 0ull; break;
        case kFeedback: {
          const int q = f.op_b[item], c = f.op_c[item];
          const uint64_t v = Fw[(long long)a * A.stride];
          if (c & 1) x[q * T + w] ^= v;
          if (c & 2) z[q * T + w] ^= v;
        } break;
        default: draw_site(f, a, A.n0, A.n1, (uint32_t)(A.tile0 + w0 + w), x + w, z + w, T, Fw, A.stride); break;
      }
    }
    __syncthreads();  // (also orders the block's stores to F before its later loads)
  }
}

struct OutArgs {
  m2dk::Args m;        // in unused; M = n_records + n_random
  const uint64_t *F;
  long long stride;
  int n_rec;
  uint32_t k0, k1;     // the request key
  long long tile0;
};

template <bool OUT_PACKED>
__global__ void __launch_bounds__(256) k_frame_out(OutArgs A) {
  extern __shared__ uint64_t lds[];
  const m2dk::Args &a = A.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint64_t *mask = lds + (size_t)wave * (a.win + m2dk::kStageBytes / 8);
  uint8_t *stage = reinterpret_cast<uint8_t *>(mask + a.win);
  const long long tiles = (a.B + 63) >> 6;
  for (long long t = (long long)blockIdx.x * nw + wave; t < tiles; t += (long long)gridDim.x * nw) {
    const long long r0 = t << 6;
    const int rows = (int)min(64LL, a.B - r0);
    uint8_t *dst = a.out + r0 * a.out_rb;
    const uint32_t tile = (uint32_t)(A.tile0 + t);  // < 2^32: first_shot + B <= 2^38
    for (int w = 0; w < a.n_win; ++w) {
      const int c_lo = w * a.win, mw = min(a.win, a.M - c_lo);
      const int32_t *rp = a.row_ptr + (long long)w * (a.n_out + 1);
      m2dk::wsync();
      // ---- phase 1: a record's mask is its flip word of this tile, a symbol's mask one Threefry block
      for (int c = c_lo + lane; c < c_lo + mw; c += 64) {
        uint64_t m;
        if (c < A.n_rec) {
          m = A.F[(long long)c * A.stride + t];
        } else {
          uint32_t x0 = (uint32_t)(c - A.n_rec), x1 = tile;
          tsimk::threefry2x32(A.k0, A.k1, x0, x1);
          m = (uint64_t)x0 | ((uint64_t)x1 << 32);
        }
        mask[c - c_lo] = m;
      }
      m2dk::wsync();
      // ---- phase 2
      m2dk::outputs<OUT_PACKED>(a, rp, w > 0, mask, stage, dst, rows, lane);
    }
  }
}

}  // namespace frmk
