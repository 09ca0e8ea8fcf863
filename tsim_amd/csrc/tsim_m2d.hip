// tsim_m2d.hip - the measurements -> detection events converter (tsim_m2d_*): a handle of its own, bound to one device,
// holding the CSR of the outputs' record lists and their reference bits; the kernel is csrc/tsim_m2d.hip.h.
#include "tsim_outputs_host.hip.h"

#include <cstring>

namespace {
constexpr int64_t kChunkBytes = 64ll << 20;       // host convert: input + output bytes per staged chunk
}  // namespace

struct tsim_m2d {
  int device = -1;
  int32_t nnz = 0;
  outh::Outputs o;     // over the M record columns (csrc/tsim_outputs_host.hip.h)
  tsimh::Uploads up;   // its lists and reference bits
  hipStream_t stream = nullptr;
  // host convert staging (grow-only)
  uint8_t *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
  int64_t in_cap = 0, out_cap = 0;
};

extern "C" int tsim_m2d_create(int32_t device, int32_t num_measurements, int32_t n_out, const int32_t *row_ptr,
                               const int32_t *cols, const uint8_t *ref, tsim_m2d **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (num_measurements < 0 || n_out < 0) return tsim_fail(TSIM_EINVAL, "bad sizes: num_measurements=%d n_out=%d", num_measurements, n_out);
  if (!row_ptr || (n_out > 0 && !ref)) return tsim_fail(TSIM_EINVAL, "NULL CSR array");
  if (row_ptr[0] != 0) return tsim_fail(TSIM_EINVAL, "row_ptr[0] = %d, not 0", row_ptr[0]);
  for (int32_t j = 0; j < n_out; ++j)
    if (row_ptr[j + 1] < row_ptr[j]) return tsim_fail(TSIM_EINVAL, "row_ptr decreases at output %d", j);
  const int32_t nnz = row_ptr[n_out];
  if (nnz > 0 && !cols) return tsim_fail(TSIM_EINVAL, "NULL CSR array");
  for (int32_t k = 0; k < nnz; ++k)
    if (cols[k] < 0 || cols[k] >= num_measurements)
      return tsim_fail(TSIM_EINVAL, "cols[%d] = %d is not a measurement record (0 .. %d)", k, cols[k], num_measurements - 1);
  outh::Outputs o;
  if (const int64_t entries = o.plan(num_measurements, n_out); entries > outh::kMaxWindowedRowPtr)
    return tsim_fail(TSIM_ENOTSUP, "%d records x %d outputs: %d windows of %d records, a CSR of %lld entries per window set "
                     "(at most %lld)", num_measurements, n_out, o.n_win, outh::kWindow, (long long)entries,
                     (long long)outh::kMaxWindowedRowPtr);
  outh::Lists lists;
  if (const int rc = o.build(row_ptr, cols, &lists)) return rc;
  if (const int rc = tsimh::open_device(device, nullptr)) return rc;
  tsim_m2d *h = new (std::nothrow) tsim_m2d();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->nnz = nnz;
  h->up.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  o.upload(h->up, lists, nnz, ref);
  h->o = o;
  if (const hipError_t e = h->up.err; e != hipSuccess) {
    tsim_m2d_destroy(h);
    return tsim_fail(TSIM_EHIP, "converter upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_m2d_destroy(tsim_m2d *h) {
  if (!h) return;
  h->up.release(h->device, h->stream);
  if (h->d_in) (void)hipFree(h->d_in);
  if (h->d_out) (void)hipFree(h->d_out);
  if (h->h_in) (void)hipHostFree(h->h_in);
  if (h->h_out) (void)hipHostFree(h->h_out);
  delete h;
}

// The checks of a conversion, before any device call (buffers: the input and output pointers); *run = false: nothing to do.
static int m2d_check(const tsim_m2d *h, int64_t B, int64_t in_row_bytes, int32_t in_packed, int64_t out_row_bytes,
                     int32_t out_packed, int32_t col0, int32_t n_cols, const void *in, const void *out, bool *run) {
  if (!h) return tsim_fail(TSIM_EINVAL, "converter is NULL");
  const outh::InRows rows{"in_row_bytes", in_row_bytes, in_packed ? (h->o.M + 7) / 8 : h->o.M};
  return outh::check_request(h->o.n_out, B, nullptr, col0, n_cols, &rows, out_row_bytes, out_packed, out && (h->o.M == 0 || in), run);
}

// enqueue the kernel (arguments already checked; B > 0, n_cols > 0)
static int m2d_launch(tsim_m2d *h, const uint8_t *d_meas, int64_t B, int64_t in_rb, int32_t in_packed, uint8_t *d_out,
                      int64_t out_rb, int32_t out_packed, int32_t col0, int32_t n_cols, hipStream_t s) {
  m2dk::Args a = h->o.args(B, d_out, out_rb, out_packed, col0, n_cols);
  h->o.fill_in(a, d_meas, in_rb, in_packed ? (h->o.M + 7) / 8 : h->o.M, true);
  const outh::Outputs::Launch g = h->o.geometry((B + 63) / 64);
  void (*k)(m2dk::Args) = in_packed ? (out_packed ? m2dk::k_m2d<true, true> : m2dk::k_m2d<true, false>)
                                    : (out_packed ? m2dk::k_m2d<false, true> : m2dk::k_m2d<false, false>);
  hipLaunchKernelGGL(k, dim3(g.blocks), dim3(64 * g.nw), g.lds, s, a);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_m2d_convert_device(tsim_m2d *h, const uint8_t *d_meas, int64_t B, int64_t in_row_bytes, int32_t in_packed,
                                       uint8_t *d_out, int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols,
                                       void *stream) {
  bool run = false;
  const int rc = m2d_check(h, B, in_row_bytes, in_packed, out_row_bytes, out_packed, col0, n_cols, d_meas, d_out, &run);
  if (rc != TSIM_OK || !run) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return m2d_launch(h, d_meas, B, in_row_bytes, in_packed, d_out, out_row_bytes, out_packed, col0, n_cols,
                    stream ? (hipStream_t)stream : h->stream);
}

static int m2d_grow(tsim_m2d *h, int64_t in_bytes, int64_t out_bytes) {
  if (in_bytes > h->in_cap) {
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->h_in) (void)hipHostFree(h->h_in);
    h->d_in = h->h_in = nullptr;
    h->in_cap = 0;
    HIP_TRY(hipMalloc(&h->d_in, (size_t)in_bytes));
    HIP_TRY(hipHostMalloc(&h->h_in, (size_t)in_bytes, hipHostMallocDefault));
    h->in_cap = in_bytes;
  }
  if (out_bytes > h->out_cap) {
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->h_out) (void)hipHostFree(h->h_out);
    h->d_out = h->h_out = nullptr;
    h->out_cap = 0;
    HIP_TRY(hipMalloc(&h->d_out, (size_t)out_bytes));
    HIP_TRY(hipHostMalloc(&h->h_out, (size_t)out_bytes, hipHostMallocDefault));
    h->out_cap = out_bytes;
  }
  return TSIM_OK;
}

extern "C" int tsim_m2d_convert(tsim_m2d *h, const uint8_t *meas, int64_t B, int64_t in_row_bytes, int32_t in_packed, uint8_t *out,
                                int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols) {
  bool run = false;
  const int rc = m2d_check(h, B, in_row_bytes, in_packed, out_row_bytes, out_packed, col0, n_cols, meas, out, &run);
  if (rc != TSIM_OK || !run) return rc;
  HIP_TRY(hipSetDevice(h->device));
  // chunks of whole 64-row tiles, about kChunkBytes of input + output each: device memory stays bounded for any B
  int64_t rows = kChunkBytes / std::max<int64_t>(1, in_row_bytes + out_row_bytes);
  rows = std::max<int64_t>(64, rows / 64 * 64);
  rows = std::min(rows, B);
  if (int r = m2d_grow(h, std::max<int64_t>(1, rows * in_row_bytes), rows * out_row_bytes)) return r;
  for (int64_t r0 = 0; r0 < B; r0 += rows) {
    const int64_t n = std::min(rows, B - r0);
    const size_t ib = (size_t)(n * in_row_bytes), ob = (size_t)(n * out_row_bytes);
    if (ib) {
      std::memcpy(h->h_in, meas + r0 * in_row_bytes, ib);
      HIP_TRY(hipMemcpyAsync(h->d_in, h->h_in, ib, hipMemcpyHostToDevice, h->stream));
    }
    if (int r = m2d_launch(h, h->d_in, n, in_row_bytes, in_packed, h->d_out, out_row_bytes, out_packed, col0, n_cols, h->stream))
      return r;
    HIP_TRY(hipMemcpyAsync(h->h_out, h->d_out, ob, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::memcpy(out + r0 * out_row_bytes, h->h_out, ob);
  }
  return TSIM_OK;
}

extern "C" int tsim_m2d_info(const tsim_m2d *h, int64_t out[4]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  out[0] = h->o.M;
  out[1] = h->o.n_out;
  out[2] = h->nnz;
  out[3] = h->device;
  return TSIM_OK;
}
