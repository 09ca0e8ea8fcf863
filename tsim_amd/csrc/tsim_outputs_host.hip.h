// tsim_outputs_host.hip.h - the host side that the column-list handles share (tsim_m2d.hip, tsim_affine.hip, tsim_frame.hip and,
// for the request check, tsim_faults.hip): outputs that are XORs over column lists, written as byte or bit-packed rows for a
// sub-range of the outputs.  The window plan of the lists, their per-window CSR, the output half of m2dk::Args, the geometry of a
// launch, and the checks of a request, on the prelude of tsim_host.hip.h.  Host code only; every check comes before the first
// device call of its caller.
#pragma once

#include "tsim_host.hip.h"
#include "tsim_m2d.hip.h"

#include <algorithm>
#include <new>
#include <vector>

namespace outh {
constexpr int kLdsBudget = 64 * 1024;              // dynamic LDS per block of the output stage
constexpr int kWindow = 2048;                      // columns per window when one wave's LDS cannot hold every column's mask
constexpr int64_t kMaxWindowedRowPtr = 1ll << 28;  // n_win x (n_out + 1) entries of the per-window CSR
constexpr int64_t kMaxShot = 1ll << 38;            // first_shot + B: the tile index is a 32-bit Threefry counter

// one wave's LDS: a 64-shot mask per column of a window, then the stage of a tile's rows
inline int64_t lds_per_wave(int64_t win) { return win * 8 + m2dk::kStageBytes; }

// the lists of a handle as its create call has them on the host: the caller's arrays, or the per-window CSR in wrp / wcols
struct Lists {
  const int32_t *row_ptr = nullptr, *cols = nullptr;
  std::vector<int32_t> wrp, wcols;
};

// The output stage of a handle: n_out outputs over M columns, in n_win windows of win columns (row_ptr holds n_win CSRs of
// n_out + 1 entries, cols is window-local), and the outputs' constant bits.
struct Outputs {
  int32_t M = 0, n_out = 0;
  int32_t win = 0, n_win = 1;  // masks per wave; windows of the columns
  const int32_t *row_ptr = nullptr, *cols = nullptr;  // device
  const uint8_t *ref = nullptr;                       // device

  // The window plan: all columns' masks in one wave's LDS when they fit the budget (in whole 64-column words, at least
  // min_win), else windows of kWindow columns, each with its own CSR.  The entries of the row pointers, which the caller
  // refuses in its own words when they pass kMaxWindowedRowPtr.
  int64_t plan(int32_t columns, int32_t outputs, int32_t min_win = 0) {
    M = columns;
    n_out = outputs;
    n_win = 1;
    if (lds_per_wave(((int64_t)M + 63) / 64 * 64) <= kLdsBudget) {
      win = std::max(min_win, (M + 63) / 64 * 64);
    } else {
      win = kWindow;
      n_win = (int32_t)(((int64_t)M + kWindow - 1) / kWindow);
    }
    return (int64_t)n_win * ((int64_t)n_out + 1);
  }

  // The lists the device gets (row_ptr: n_out + 1 entries from 0, cols inside 0 .. M - 1, both checked by the caller): as they
  // are with one window, else every output's columns bucketed by window, the columns window-local.  0, or an error code after
  // tsim_fail.
  int build(const int32_t *row_ptr_in, const int32_t *cols_in, Lists *l) const {
    l->row_ptr = row_ptr_in;
    l->cols = cols_in;
    if (n_win == 1) return TSIM_OK;
    try {
      const size_t stride = (size_t)n_out + 1;
      l->wrp.assign((size_t)n_win * stride, 0);
      l->wcols.resize((size_t)row_ptr_in[n_out]);
      for (int32_t j = 0; j < n_out; ++j)
        for (int32_t k = row_ptr_in[j]; k < row_ptr_in[j + 1]; ++k) ++l->wrp[(size_t)(cols_in[k] / win) * stride + j + 1];
      int32_t run = 0;
      for (int32_t w = 0; w < n_win; ++w) {
        int32_t *r = l->wrp.data() + (size_t)w * stride;
        r[0] = run;
        for (int32_t j = 0; j < n_out; ++j) r[j + 1] = (run += r[j + 1]);
      }
      std::vector<int32_t> fill(l->wrp);
      for (int32_t j = 0; j < n_out; ++j)
        for (int32_t k = row_ptr_in[j]; k < row_ptr_in[j + 1]; ++k) {
          const int32_t w = cols_in[k] / win;
          l->wcols[(size_t)fill[(size_t)w * stride + j]++] = cols_in[k] - w * win;
        }
    } catch (const std::bad_alloc &) {
      return tsim_fail(TSIM_ENOMEM, "out of host memory for the per-window CSR");
    }
    l->row_ptr = l->wrp.data();
    l->cols = l->wcols.data();
    return TSIM_OK;
  }

  // the lists of build() and the n_out constant bits, into buffers of `up`
  void upload(tsimh::Uploads &up, const Lists &l, int32_t nnz, const uint8_t *ref_in) {
    row_ptr = up.put(l.row_ptr, (size_t)n_win * ((size_t)n_out + 1));
    cols = up.put(l.cols, (size_t)nnz);
    ref = up.put(ref_in, (size_t)n_out);
  }

  // The kernels' arguments for B rows of the outputs col0 .. col0 + n_cols - 1 (a request that check_request passed): the
  // output half, B and M.  The input half is zero: no input rows (fill_in sets it for the handles that read some).
  m2dk::Args args(int64_t B, uint8_t *d_out, int64_t out_rb, int32_t out_packed, int32_t col0, int32_t n_cols) const {
    m2dk::Args a{};
    a.B = B;
    a.M = M;
    a.row_ptr = row_ptr;
    a.cols = cols;
    a.ref = ref;
    a.col0 = col0;
    a.n_cols = n_cols;
    a.out = d_out;
    a.out_rb = out_rb;
    a.out_used = out_packed ? (n_cols + 7) / 8 : n_cols;
    a.out_contig = out_rb == a.out_used && out_rb <= 64;
    a.out_w4 = (out_rb % 4 == 0 || a.out_contig) && reinterpret_cast<uintptr_t>(d_out) % 4 == 0;
    a.n_out = n_out;
    a.win = win;
    a.n_win = n_win;
    return a;
  }

  // The input half: bit or byte rows in_rb apart of which in_used bytes hold the columns; `one_span`: the handle's own
  // condition for staging a tile as one span, besides a stride of at most kStageRow bytes and one window.
  void fill_in(m2dk::Args &a, const uint8_t *d_in, int64_t in_rb, int in_used, bool one_span) const {
    a.in = d_in;
    a.in_rb = in_rb;
    a.in_used = in_used;
    a.in_contig = one_span && in_rb <= m2dk::kStageRow && n_win == 1;
    a.in_w4 = (in_rb % 4 == 0 || a.in_contig) && reinterpret_cast<uintptr_t>(d_in) % 4 == 0;
  }

  // a launch over `tiles` 64-row tiles: a wave per tile, as many waves in a block as the budget holds
  struct Launch {
    int nw;           // waves per block
    unsigned blocks;
    size_t lds;       // dynamic LDS bytes of a block
  };
  Launch geometry(int64_t tiles) const {
    const int per_wave = (int)lds_per_wave(win);
    const int nw = std::max(1, std::min(m2dk::kMaxWaves, kLdsBudget / per_wave));
    return {nw, (unsigned)std::min<int64_t>((tiles + nw - 1) / nw, 256 * 8 * 4 / nw), (size_t)nw * per_wave};
  }
};

// the input rows of a request: what the refusal calls their stride, the stride, the bytes of a row that hold the columns
struct InRows {
  const char *name;
  int64_t row_bytes, used;
};

// The checks of a request for B rows of the outputs col0 .. col0 + n_cols - 1 of n_out, before any device call and in this
// order: B; the shot counter (first_shot NULL: the call has none); the output range; the input rows' stride (in NULL: the call
// reads none); the output rows' stride; then the empty request (*run = false: success, nothing to do) and the buffers
// (bufs_ok: no pointer the kernel follows is NULL).  0, or an error code after tsim_fail.
inline int check_request(int32_t n_out, int64_t B, const int64_t *first_shot, int32_t col0, int32_t n_cols, const InRows *in,
                         int64_t out_row_bytes, int32_t out_packed, bool bufs_ok, bool *run) {
  *run = false;
  if (B < 0) return tsim_fail(TSIM_EINVAL, "negative B");
  if (first_shot) {
    const int64_t s = *first_shot;
    if (s < 0 || s % 64 != 0) return tsim_fail(TSIM_EINVAL, "first_shot = %lld is not a non-negative multiple of 64", (long long)s);
    if (s > kMaxShot || B > kMaxShot - s)
      return tsim_fail(TSIM_EINVAL, "first_shot + B = %lld + %lld exceeds 2^38", (long long)s, (long long)B);
  }
  if (col0 < 0 || n_cols < 0 || (int64_t)col0 + n_cols > n_out)
    return tsim_fail(TSIM_EINVAL, "outputs %d .. %d + %d of %d", col0, col0, n_cols, n_out);
  if (in && (in->row_bytes < in->used || in->row_bytes > 0x7FFFFFFF))
    return tsim_fail(TSIM_EINVAL, "%s = %lld for %lld bytes per row", in->name, (long long)in->row_bytes, (long long)in->used);
  const int64_t out_used = out_packed ? (n_cols + 7) / 8 : n_cols;
  if (out_row_bytes < out_used || out_row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "out_row_bytes = %lld for %lld bytes per row", (long long)out_row_bytes, (long long)out_used);
  if (B == 0 || n_cols == 0) return TSIM_OK;
  if (!bufs_ok) return tsim_fail(TSIM_EINVAL, "NULL buffer");
  *run = true;
  return TSIM_OK;
}
}  // namespace outh
