// tsim_affine.hip - the affine measurement sampler (tsim_affine_*): a handle of its own, bound to one device, holding the
// CSR of the outputs' column lists over [f | random symbols] and their constant bits; the kernel is csrc/tsim_affine.hip.h.
#include "tsim_host.hip.h"
#include "tsim_affine.hip.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {
constexpr int kLdsBudget = 64 * 1024;             // dynamic LDS per block
constexpr int kWindow = 2048;                     // columns per window when one wave's LDS cannot hold every column's mask
constexpr int64_t kMaxWindowedRowPtr = 1ll << 28; // n_win x (n_out + 1) entries of the per-window CSR
constexpr int64_t kMaxShot = 1ll << 38;           // first_shot + B: the tile index is a 32-bit Threefry counter
}  // namespace

struct tsim_affine {
  int device = -1;
  int32_t num_f = 0, n_random = 0, n_out = 0, nnz = 0;
  int32_t win = 0, n_win = 1;  // masks per wave; windows of the columns (row_ptr holds n_win CSRs)
  int32_t *d_row_ptr = nullptr, *d_cols = nullptr;
  uint8_t *d_flip = nullptr;
  hipStream_t stream = nullptr;
};

static void affine_release(tsim_affine *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->d_row_ptr) (void)hipFree(h->d_row_ptr);
  if (h->d_cols) (void)hipFree(h->d_cols);
  if (h->d_flip) (void)hipFree(h->d_flip);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

static int64_t affine_lds_per_wave(int64_t win) { return win * 8 + m2dk::kStageBytes; }

extern "C" int tsim_affine_create(int32_t device, int32_t num_f, int32_t n_random, int32_t n_out, const int32_t *row_ptr,
                                  const int32_t *cols, const uint8_t *flip, tsim_affine **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (num_f < 0 || n_random < 0 || n_out < 0 || (int64_t)num_f + n_random > 0x7FFFFFC0ll)
    return tsim_fail(TSIM_EINVAL, "bad sizes: num_f=%d n_random=%d n_out=%d", num_f, n_random, n_out);
  if (!row_ptr || (n_out > 0 && !flip)) return tsim_fail(TSIM_EINVAL, "NULL CSR array");
  if (row_ptr[0] != 0) return tsim_fail(TSIM_EINVAL, "row_ptr[0] = %d, not 0", row_ptr[0]);
  for (int32_t j = 0; j < n_out; ++j)
    if (row_ptr[j + 1] < row_ptr[j]) return tsim_fail(TSIM_EINVAL, "row_ptr decreases at output %d", j);
  const int32_t M = num_f + n_random, nnz = row_ptr[n_out];
  if (nnz > 0 && !cols) return tsim_fail(TSIM_EINVAL, "NULL CSR array");
  for (int32_t k = 0; k < nnz; ++k)
    if (cols[k] < 0 || cols[k] >= M)
      return tsim_fail(TSIM_EINVAL, "cols[%d] = %d is not a column (0 .. %d: %d f bits, then %d random symbols)", k, cols[k], M - 1,
                       num_f, n_random);
  // all columns' masks in one wave's LDS when they fit, else windows of kWindow columns, each with its own CSR
  int32_t win = 0, n_win = 1;
  if (affine_lds_per_wave(((int64_t)M + 63) / 64 * 64) <= kLdsBudget) {
    win = (M + 63) / 64 * 64;
  } else {
    win = kWindow;
    n_win = (int32_t)(((int64_t)M + kWindow - 1) / kWindow);
  }
  if ((int64_t)n_win * ((int64_t)n_out + 1) > kMaxWindowedRowPtr)
    return tsim_fail(TSIM_ENOTSUP, "%d columns x %d outputs: %d windows of %d columns, a CSR of %lld entries per window set "
                     "(at most %lld)", M, n_out, n_win, kWindow, (long long)n_win * ((long long)n_out + 1),
                     (long long)kMaxWindowedRowPtr);
  std::vector<int32_t> wrp, wcols;
  if (n_win > 1) try {  // bucket every output's columns by window; columns become window-local
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
  tsim_affine *h = new (std::nothrow) tsim_affine();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->num_f = num_f;
  h->n_random = n_random;
  h->n_out = n_out;
  h->nnz = nnz;
  h->win = win;
  h->n_win = n_win;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&h->d_row_ptr, sizeof(int32_t) * (size_t)n_win * (n_out + 1));
  if (e == hipSuccess) e = hipMalloc(&h->d_cols, sizeof(int32_t) * (size_t)std::max(1, nnz));
  if (e == hipSuccess) e = hipMalloc(&h->d_flip, (size_t)std::max(1, n_out));
  if (e == hipSuccess) e = hipMemcpy(h->d_row_ptr, row_ptr, sizeof(int32_t) * (size_t)n_win * (n_out + 1), hipMemcpyHostToDevice);
  if (e == hipSuccess && nnz > 0) e = hipMemcpy(h->d_cols, cols, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice);
  if (e == hipSuccess && n_out > 0) e = hipMemcpy(h->d_flip, flip, (size_t)n_out, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    affine_release(h);
    delete h;
    return tsim_fail(TSIM_EHIP, "affine sampler upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_affine_destroy(tsim_affine *h) {
  if (!h) return;
  affine_release(h);
  delete h;
}

extern "C" int tsim_affine_sample_device(tsim_affine *h, const uint64_t *d_f, int64_t f_row_bytes, int64_t B, int64_t first_shot,
                                         uint32_t key_hi, uint32_t key_lo, uint8_t *d_out, int64_t out_row_bytes,
                                         int32_t out_packed, int32_t col0, int32_t n_cols, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  if (B < 0) return tsim_fail(TSIM_EINVAL, "negative B");
  if (first_shot < 0 || first_shot % 64 != 0)
    return tsim_fail(TSIM_EINVAL, "first_shot = %lld is not a non-negative multiple of 64", (long long)first_shot);
  if (first_shot > kMaxShot || B > kMaxShot - first_shot)
    return tsim_fail(TSIM_EINVAL, "first_shot + B = %lld + %lld exceeds 2^38", (long long)first_shot, (long long)B);
  if (col0 < 0 || n_cols < 0 || (int64_t)col0 + n_cols > h->n_out)
    return tsim_fail(TSIM_EINVAL, "outputs %d .. %d + %d of %d", col0, col0, n_cols, h->n_out);
  const int64_t f_used = (h->num_f + 7) / 8;
  const int64_t out_used = out_packed ? (n_cols + 7) / 8 : n_cols;
  if (f_row_bytes < f_used || f_row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "f_row_bytes = %lld for %lld bytes per row", (long long)f_row_bytes, (long long)f_used);
  if (out_row_bytes < out_used || out_row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "out_row_bytes = %lld for %lld bytes per row", (long long)out_row_bytes, (long long)out_used);
  if (B == 0 || n_cols == 0) return TSIM_OK;
  if (!d_out || (h->num_f > 0 && !d_f)) return tsim_fail(TSIM_EINVAL, "NULL buffer");
  HIP_TRY(hipSetDevice(h->device));
  const uint8_t *f = reinterpret_cast<const uint8_t *>(d_f);
  affk::Args A;
  m2dk::Args &a = A.m;
  a.in = f;
  a.B = B;
  a.in_rb = f_row_bytes;
  a.M = h->num_f + h->n_random;
  a.in_used = (int)f_used;
  a.in_contig = h->num_f > 0 && f_row_bytes <= m2dk::kStageRow && h->n_win == 1;
  a.in_w4 = (f_row_bytes % 4 == 0 || a.in_contig) && reinterpret_cast<uintptr_t>(f) % 4 == 0;
  a.row_ptr = h->d_row_ptr;
  a.cols = h->d_cols;
  a.ref = h->d_flip;
  a.col0 = col0;
  a.n_cols = n_cols;
  a.out = d_out;
  a.out_rb = out_row_bytes;
  a.out_used = (int)out_used;
  a.out_contig = out_row_bytes == out_used && out_row_bytes <= 64;
  a.out_w4 = (out_row_bytes % 4 == 0 || a.out_contig) && reinterpret_cast<uintptr_t>(d_out) % 4 == 0;
  a.n_out = h->n_out;
  a.win = h->win;
  a.n_win = h->n_win;
  A.num_f = h->num_f;
  A.k0 = key_hi;
  A.k1 = key_lo;
  A.tile0 = first_shot / 64;
  const int per_wave = (int)affine_lds_per_wave(h->win);
  const int nw = std::max(1, std::min(m2dk::kMaxWaves, kLdsBudget / per_wave));
  const int64_t tiles = (B + 63) / 64;
  const int64_t blocks = std::min<int64_t>((tiles + nw - 1) / nw, 256 * 8 * 4 / nw);
  const size_t lds = (size_t)nw * per_wave;
  void (*k)(affk::Args) = out_packed ? affk::k_affine<true> : affk::k_affine<false>;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * nw), lds, stream ? (hipStream_t)stream : h->stream, A);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_affine_info(const tsim_affine *h, int64_t out[8]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  out[0] = h->num_f;
  out[1] = h->n_random;
  out[2] = h->n_out;
  out[3] = h->nnz;
  out[4] = h->device;
  out[5] = h->win;
  out[6] = h->n_win;
  out[7] = affine_lds_per_wave(h->win);
  return TSIM_OK;
}
