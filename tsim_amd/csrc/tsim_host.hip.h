// tsim_host.hip.h - the host prelude of every translation unit that calls HIP: the error convention, opening a device, the
// host half of the row contract of csrc/tsim_bitrows.hip.h, the device buffers a handle owns and the dynamic-LDS attribute of
// its kernels.  Host code only.
#pragma once
#include "../../include/tsim_hip.h"
#include "tsim_bitrows.hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

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

// The device buffers a handle owns: the first error is kept and ends the work, the bytes are added up.  The convention, one
// for every handle: a table of n elements gets a buffer of max(1, n) elements (an empty table still has an address; the
// union-find handles never pass one), a copy of no byte is not made, and `bytes` counts the n elements only.
struct Uploads {
  std::vector<void *> ptrs;
  int64_t bytes = 0;
  hipError_t err = hipSuccess;

  // `size` bytes of device memory, not written
  void *room(size_t size) {
    void *d = nullptr;
    if (err == hipSuccess) err = hipMalloc(&d, size);
    if (err != hipSuccess) return nullptr;
    ptrs.push_back(d);
    return d;
  }
  // n elements of src in a buffer of their own; `slack`: bytes after them that src holds too, uploaded but not counted
  template <class T>
  T *put(const T *src, size_t n, size_t slack = 0) {
    void *d = room(std::max<size_t>(1, n) * sizeof(T) + slack);
    if (!d) return nullptr;
    if (n * sizeof(T) + slack) err = hipMemcpy(d, src, n * sizeof(T) + slack, hipMemcpyHostToDevice);
    bytes += (int64_t)(n * sizeof(T));
    return static_cast<T *>(d);
  }
  template <class T>
  T *put(const std::vector<T> &v) { return put(v.data(), v.size()); }

  // frees the buffers on `device`; the handle's own stream, if it has one, is waited for first and destroyed after
  void release(int device, hipStream_t stream = nullptr) {
    if (device >= 0) (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void *p : ptrs) (void)hipFree(p);
    ptrs.clear();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// lets a block of each kernel take `bytes` of dynamic LDS; once per handle (*done)
template <class K, size_t N>
int allow_lds(K *const (&kernels)[N], int64_t bytes, bool *done) {
  if (*done) return TSIM_OK;
  for (K *k : kernels) HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  *done = true;
  return TSIM_OK;
}

}  // namespace tsimh
