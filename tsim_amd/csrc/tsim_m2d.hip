// tsim_m2d.hip - the measurements -> detection events converter (tsim_m2d_*): a handle of its own, bound to one device,
// holding the CSR of the outputs' record lists and their reference bits; the kernel is csrc/tsim_m2d.hip.h.
#include "tsim_host.hip.h"
#include "tsim_m2d.hip.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace {
constexpr int kLdsBudget = 64 * 1024;             // dynamic LDS per block
constexpr int kWindow = 2048;                     // columns per window when one wave's LDS cannot hold every record's mask
constexpr int64_t kMaxWindowedRowPtr = 1ll << 28; // n_win x (n_out + 1) entries of the per-window CSR
constexpr int64_t kChunkBytes = 64ll << 20;       // host convert: input + output bytes per staged chunk
}  // namespace

struct tsim_m2d {
  int device = -1;
  int32_t M = 0, n_out = 0, nnz = 0;
  int32_t win = 0, n_win = 1;  // masks per wave; windows of the record columns (row_ptr holds n_win CSRs)
  int32_t *d_row_ptr = nullptr, *d_cols = nullptr;
  uint8_t *d_ref = nullptr;
  hipStream_t stream = nullptr;
  // host convert staging (grow-only)
  uint8_t *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
  int64_t in_cap = 0, out_cap = 0;
};

static void m2d_release(tsim_m2d *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->d_row_ptr) (void)hipFree(h->d_row_ptr);
  if (h->d_cols) (void)hipFree(h->d_cols);
  if (h->d_ref) (void)hipFree(h->d_ref);
  if (h->d_in) (void)hipFree(h->d_in);
  if (h->d_out) (void)hipFree(h->d_out);
  if (h->h_in) (void)hipHostFree(h->h_in);
  if (h->h_out) (void)hipHostFree(h->h_out);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

static int64_t m2d_lds_per_wave(int64_t win) { return win * 8 + m2dk::kStageBytes; }

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
  // all records' masks in one wave's LDS when they fit, else windows of kWindow columns, each with its own CSR
  int32_t win = 0, n_win = 1;
  if (m2d_lds_per_wave(((int64_t)num_measurements + 63) / 64 * 64) <= kLdsBudget) {
    win = (num_measurements + 63) / 64 * 64;
  } else {
    win = kWindow;
    n_win = (int32_t)(((int64_t)num_measurements + kWindow - 1) / kWindow);
  }
  if ((int64_t)n_win * ((int64_t)n_out + 1) > kMaxWindowedRowPtr)
    return tsim_fail(TSIM_ENOTSUP, "%d records x %d outputs: %d windows of %d records, a CSR of %lld entries per window set "
                     "(at most %lld)", num_measurements, n_out, n_win, kWindow, (long long)n_win * ((long long)n_out + 1),
                     (long long)kMaxWindowedRowPtr);
  std::vector<int32_t> wrp, wcols;
  if (n_win > 1) try {  // bucket every output's records by window; columns become window-local
    wrp.assign((size_t)n_win * (n_out + 1), 0);
    wcols.resize((size_t)nnz);
    for (int32_t j = 0; j < n_out; ++j)
      for (int32_t k = row_ptr[j]; k < row_ptr[j + 1]; ++k) ++wrp[(size_t)(cols[k] / win) * (n_out + 1) + j + 1];
    int32_t run = 0;
    for (int32_t w = 0; w < n_win; ++w) {
      int32_t *r = wrp.data() + (size_t)w * (n_out + 1);
      r[0] = run;
      for (int32_t j = 0; j < n_out; ++j) r[j + 1] = (run += r[j + 1]);
    }
    std::vector<int32_t> fill(wrp);
    for (int32_t j = 0; j < n_out; ++j)
      for (int32_t k = row_ptr[j]; k < row_ptr[j + 1]; ++k) {
        const int32_t w = cols[k] / win;
        wcols[(size_t)fill[(size_t)w * (n_out + 1) + j]++] = cols[k] - w * win;
      }
    row_ptr = wrp.data();
    cols = wcols.data();
  } catch (const std::bad_alloc &) {
    return tsim_fail(TSIM_ENOMEM, "out of host memory for the per-window CSR");
  }
  if (const int rc = tsimh::open_device(device, nullptr)) return rc;
  tsim_m2d *h = new (std::nothrow) tsim_m2d();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->M = num_measurements;
  h->n_out = n_out;
  h->nnz = nnz;
  h->win = win;
  h->n_win = n_win;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&h->d_row_ptr, sizeof(int32_t) * (size_t)n_win * (n_out + 1));
  if (e == hipSuccess) e = hipMalloc(&h->d_cols, sizeof(int32_t) * (size_t)std::max(1, nnz));
  if (e == hipSuccess) e = hipMalloc(&h->d_ref, (size_t)std::max(1, n_out));
  if (e == hipSuccess) e = hipMemcpy(h->d_row_ptr, row_ptr, sizeof(int32_t) * (size_t)n_win * (n_out + 1), hipMemcpyHostToDevice);
  if (e == hipSuccess && nnz > 0) e = hipMemcpy(h->d_cols, cols, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice);
  if (e == hipSuccess && n_out > 0) e = hipMemcpy(h->d_ref, ref, (size_t)n_out, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    m2d_release(h);
    delete h;
    return tsim_fail(TSIM_EHIP, "converter upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_m2d_destroy(tsim_m2d *h) {
  if (!h) return;
  m2d_release(h);
  delete h;
}

static int m2d_check(const tsim_m2d *h, int64_t B, int64_t in_row_bytes, int32_t in_packed, int64_t out_row_bytes,
                     int32_t out_packed, int32_t col0, int32_t n_cols) {
  if (!h) return tsim_fail(TSIM_EINVAL, "converter is NULL");
  if (B < 0) return tsim_fail(TSIM_EINVAL, "negative B");
  if (col0 < 0 || n_cols < 0 || (int64_t)col0 + n_cols > h->n_out)
    return tsim_fail(TSIM_EINVAL, "outputs %d .. %d + %d of %d", col0, col0, n_cols, h->n_out);
  const int64_t in_used = in_packed ? (h->M + 7) / 8 : h->M;
  const int64_t out_used = out_packed ? (n_cols + 7) / 8 : n_cols;
  if (in_row_bytes < in_used || in_row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "in_row_bytes = %lld for %lld bytes per row", (long long)in_row_bytes, (long long)in_used);
  if (out_row_bytes < out_used || out_row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "out_row_bytes = %lld for %lld bytes per row", (long long)out_row_bytes, (long long)out_used);
  return TSIM_OK;
}

// enqueue the kernel (arguments already checked; B > 0, n_cols > 0)
static int m2d_launch(tsim_m2d *h, const uint8_t *d_meas, int64_t B, int64_t in_rb, int32_t in_packed, uint8_t *d_out,
                      int64_t out_rb, int32_t out_packed, int32_t col0, int32_t n_cols, hipStream_t s) {
  m2dk::Args a;
  a.in = d_meas;
  a.B = B;
  a.in_rb = in_rb;
  a.M = h->M;
  a.in_used = in_packed ? (h->M + 7) / 8 : h->M;
  a.in_contig = in_rb <= m2dk::kStageRow && h->n_win == 1;
  a.in_w4 = (in_rb % 4 == 0 && reinterpret_cast<uintptr_t>(d_meas) % 4 == 0) || (a.in_contig && reinterpret_cast<uintptr_t>(d_meas) % 4 == 0);
  a.row_ptr = h->d_row_ptr;
  a.cols = h->d_cols;
  a.ref = h->d_ref;
  a.col0 = col0;
  a.n_cols = n_cols;
  a.out = d_out;
  a.out_rb = out_rb;
  a.out_used = out_packed ? (n_cols + 7) / 8 : n_cols;
  a.out_contig = out_rb == a.out_used && out_rb <= 64;
  a.out_w4 = (out_rb % 4 == 0 || a.out_contig) && reinterpret_cast<uintptr_t>(d_out) % 4 == 0;
  a.n_out = h->n_out;
  a.win = h->win;
  a.n_win = h->n_win;
  const int per_wave = (int)m2d_lds_per_wave(h->win);
  const int nw = std::max(1, std::min(m2dk::kMaxWaves, kLdsBudget / per_wave));
  const int64_t tiles = (B + 63) / 64;
  const int64_t blocks = std::min<int64_t>((tiles + nw - 1) / nw, 256 * 8 * 4 / nw);
  const size_t lds = (size_t)nw * per_wave;
  void (*k)(m2dk::Args) = in_packed ? (out_packed ? m2dk::k_m2d<true, true> : m2dk::k_m2d<true, false>)
                                    : (out_packed ? m2dk::k_m2d<false, true> : m2dk::k_m2d<false, false>);
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * nw), lds, s, a);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_m2d_convert_device(tsim_m2d *h, const uint8_t *d_meas, int64_t B, int64_t in_row_bytes, int32_t in_packed,
                                       uint8_t *d_out, int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols,
                                       void *stream) {
  if (int r = m2d_check(h, B, in_row_bytes, in_packed, out_row_bytes, out_packed, col0, n_cols)) return r;
  if (B == 0 || n_cols == 0) return TSIM_OK;
  if (!d_out || (h->M > 0 && !d_meas)) return tsim_fail(TSIM_EINVAL, "NULL buffer");
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
  if (int r = m2d_check(h, B, in_row_bytes, in_packed, out_row_bytes, out_packed, col0, n_cols)) return r;
  if (B == 0 || n_cols == 0) return TSIM_OK;
  if (!out || (h->M > 0 && !meas)) return tsim_fail(TSIM_EINVAL, "NULL buffer");
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
  out[0] = h->M;
  out[1] = h->n_out;
  out[2] = h->nnz;
  out[3] = h->device;
  return TSIM_OK;
}
