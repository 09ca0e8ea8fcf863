// tsim_host.hip.h - the host prelude of every translation unit that calls HIP: the error convention, opening a device, and the
// host half of the row contract of csrc/tsim_bitrows.hip.h.  Host code only.
#pragma once
#include "../../include/tsim_hip.h"
#include "tsim_bitrows.hip.h"

#include <hip/hip_runtime.h>

// every entry point returns 0 or a negative TSIM_E* code; the message is thread-local (tsim_program.hip)
int tsim_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return tsim_fail(TSIM_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace tsimh {

// makes `device` current; its compute units (cus may be NULL)
inline int open_device(int device, int *cus) {
  int count = 0;
  HIP_TRY(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) return tsim_fail(TSIM_EINVAL, "device %d of %d", device, count);
  HIP_TRY(hipSetDevice(device));
  if (cus) HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
  return TSIM_OK;
}

// the bytes of a row that hold n_cols columns, or an error code after tsim_fail when the stride row_bytes cannot hold them
inline int64_t row_used(int32_t n_cols, int64_t row_bytes) {
  const int64_t used = ((int64_t)n_cols + 7) / 8;
  if (row_bytes < used || row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "row_bytes = %lld for %lld bytes per row", (long long)row_bytes, (long long)used);
  return used;
}

// how bitrows::stage_rows stages a tile, into a.contig, a.w4 and a.stage_bytes: as one span when the stride is at most kChunk
// bytes (and `one_span` allows it), dword loads where the pointer and the stride allow
template <class Args>
void choose_staging(Args &a, const uint8_t *d_rows, int64_t row_bytes, bool one_span = true) {
  a.contig = one_span && row_bytes <= bitrows::kChunk;
  const bool p4 = reinterpret_cast<uintptr_t>(d_rows) % 4 == 0;
  a.w4 = p4 && (a.contig || row_bytes % 4 == 0);
  a.stage_bytes = a.contig ? (int)(64 * row_bytes + 8 + 7) / 8 * 8 : 64 * bitrows::kStage;
}

}  // namespace tsimh
