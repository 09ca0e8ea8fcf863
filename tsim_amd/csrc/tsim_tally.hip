// tsim_tally.hip - counts over bit-packed device rows (tsim_tally_rows_device): kept rows, kept rows with an observable
// set, per-column counts and a histogram, accumulated into caller-owned uint64 counters; the kernel is csrc/tsim_tally.hip.h.
#include "tsim_host.hip.h"
#include "tsim_tally.hip.h"

#include <algorithm>

namespace {
constexpr int kWindow = 4096;              // columns per block's partials (16 KiB of LDS)
constexpr int kLdsHistBits = 11;           // histograms of up to 2^11 bins are kept in LDS per block
constexpr int64_t kRowsPerLaunch = 1ll << 31;  // a block's uint32 partials cannot overflow
constexpr int kBlocksPerWindow = 1024;
}  // namespace

extern "C" int tsim_tally_rows_device(int32_t device, const uint8_t *d_rows, int64_t n, int64_t row_bytes, int32_t n_cols,
                                      const uint8_t *d_xor, const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi,
                                      const int32_t *hist_cols, int32_t n_hist, uint64_t *d_counts, void *stream) {
  if (n < 0) return tsim_fail(TSIM_EINVAL, "negative n");
  if (n_cols < 1 || n_cols > (1 << 30)) return tsim_fail(TSIM_EINVAL, "n_cols = %d (1 .. 2^30)", n_cols);
  const int64_t used = tsimh::row_used(n_cols, row_bytes);
  if (used < 0) return (int)used;
  if (obs_lo < 0 || obs_hi < obs_lo || obs_hi > n_cols)
    return tsim_fail(TSIM_EINVAL, "observable columns %d .. %d of %d", obs_lo, obs_hi, n_cols);
  if (n_hist < 0 || n_hist > tallyk::kMaxHist) return tsim_fail(TSIM_EINVAL, "n_hist = %d (0 .. %d)", n_hist, tallyk::kMaxHist);
  if (n_hist > 0 && !hist_cols) return tsim_fail(TSIM_EINVAL, "hist_cols is NULL");
  for (int i = 0; i < n_hist; ++i) {
    if (hist_cols[i] < 0 || hist_cols[i] >= n_cols)
      return tsim_fail(TSIM_EINVAL, "hist_cols[%d] = %d is not a column (0 .. %d)", i, hist_cols[i], n_cols - 1);
    for (int j = 0; j < i; ++j)
      if (hist_cols[j] == hist_cols[i]) return tsim_fail(TSIM_EINVAL, "hist_cols[%d] = hist_cols[%d] = %d", j, i, hist_cols[i]);
  }
  if (!d_counts || reinterpret_cast<uintptr_t>(d_counts) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_counts is NULL or not 8-byte aligned");
  if (n > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(device));

  tallyk::Args a{};
  a.rb = row_bytes;
  a.n_cols = n_cols;
  a.used = (int)used;
  a.xr = d_xor;
  a.test = d_test;
  a.obs_lo = obs_lo;
  a.obs_hi = obs_hi;
  a.n_hist = n_hist;
  for (int i = 0; i < n_hist; ++i) a.hc[i] = hist_cols[i];
  a.counts = reinterpret_cast<unsigned long long *>(d_counts);
  const int n_win = (int)(((int64_t)n_cols + kWindow - 1) / kWindow);
  a.win = n_win > 1 ? kWindow : (n_cols + 63) / 64 * 64;
  a.hist_lds = n_hist <= kLdsHistBits;
  tsimh::choose_staging(a, d_rows, row_bytes, n_win == 1);
  const int nw = tallyk::kMaxWaves;
  const size_t lds = (size_t)a.win * 4 + (a.hist_lds ? (size_t)(((1 << n_hist) + 1) & ~1) * 4 : 0) + 16 + (size_t)nw * a.stage_bytes;
  hipStream_t s = (hipStream_t)stream;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * row_bytes;
    const int64_t tiles = (a.n + 63) / 64;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((tiles + nw - 1) / nw, kBlocksPerWindow));
    hipLaunchKernelGGL(tallyk::k_tally, dim3((unsigned)blocks, (unsigned)n_win), dim3(64 * nw), lds, s, a);
    HIP_TRY(hipGetLastError());
  }
  return TSIM_OK;
}
