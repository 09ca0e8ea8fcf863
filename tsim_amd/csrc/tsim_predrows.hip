// tsim_predrows.hip - a decoder's predictions XORed into, or written as, columns of bit-packed device rows
// (tsim_pred_rows_device): no handle, caller-owned rows and predictions; the kernel is csrc/tsim_predrows.hip.h.
#include "tsim_host.hip.h"
#include "tsim_predrows.hip.h"

#include <algorithm>

namespace {
constexpr int64_t kRowsPerLaunch = 1ll << 30;  // the cut of the decode calls whose d_pred this reads (ufh::launch_rows)
constexpr int kGrid = 2048;                    // blocks of a full grid: the rest of a launch's rows by grid stride
}  // namespace

extern "C" int tsim_pred_rows_device(int32_t device, const uint64_t *d_pred, int64_t n, int32_t n_obs, uint8_t *d_rows, int64_t row_bytes,
                                     int32_t col0, int32_t mode, void *stream) {
  if (n < 0) return tsim_fail(TSIM_EINVAL, "negative n");
  if (n_obs < 1 || n_obs > 64) return tsim_fail(TSIM_EINVAL, "n_obs = %d (1 .. 64)", n_obs);
  if (col0 < 0) return tsim_fail(TSIM_EINVAL, "col0 = %d is negative", col0);
  if (row_bytes < 1 || row_bytes > 0x7FFFFFFF) return tsim_fail(TSIM_EINVAL, "row_bytes = %lld (1 .. 2^31 - 1)", (long long)row_bytes);
  if ((int64_t)col0 + n_obs > 8 * row_bytes)
    return tsim_fail(TSIM_EINVAL, "columns %d .. %lld of rows of %lld bytes", col0, (long long)col0 + n_obs - 1, (long long)row_bytes);
  if (mode != predk::kXor && mode != predk::kWrite) return tsim_fail(TSIM_EINVAL, "mode = %d (0: xor, 1: write)", mode);
  if (n > 0 && (!d_pred || !d_rows)) return tsim_fail(TSIM_EINVAL, "d_pred or d_rows is NULL");
  if (reinterpret_cast<uintptr_t>(d_pred) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_pred is not 8-byte aligned");
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(device));

  predk::Args a{};
  a.rb = row_bytes;
  a.col0 = col0;
  a.n_obs = n_obs;
  a.mode = mode;
  a.w8 = reinterpret_cast<uintptr_t>(d_rows) % 8 == 0 && row_bytes % 8 == 0;
  const int block = 64 * predk::kWaves;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * row_bytes;
    a.pred = reinterpret_cast<const unsigned long long *>(d_pred) + r0;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((a.n + block - 1) / block, kGrid));
    hipLaunchKernelGGL(predk::k_pred_rows, dim3((unsigned)blocks), dim3(block), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
  }
  return TSIM_OK;
}
