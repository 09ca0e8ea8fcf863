// tsim_affine.hip - the affine measurement sampler (tsim_affine_*): a handle of its own, bound to one device, holding the
// CSR of the outputs' column lists over [f | random symbols] and their constant bits; the kernel is csrc/tsim_affine.hip.h.
#include "tsim_outputs_host.hip.h"
#include "tsim_affine.hip.h"

struct tsim_affine {
  int device = -1;
  int32_t num_f = 0, n_random = 0, nnz = 0;
  outh::Outputs o;     // over the num_f + n_random columns (csrc/tsim_outputs_host.hip.h)
  tsimh::Uploads up;   // its lists and constant bits
  hipStream_t stream = nullptr;
};

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
  outh::Outputs o;
  if (const int64_t entries = o.plan(M, n_out); entries > outh::kMaxWindowedRowPtr)
    return tsim_fail(TSIM_ENOTSUP, "%d columns x %d outputs: %d windows of %d columns, a CSR of %lld entries per window set "
                     "(at most %lld)", M, n_out, o.n_win, outh::kWindow, (long long)entries, (long long)outh::kMaxWindowedRowPtr);
  outh::Lists lists;
  if (const int rc = o.build(row_ptr, cols, &lists)) return rc;
  if (const int rc = tsimh::open_device(device, nullptr)) return rc;
  tsim_affine *h = new (std::nothrow) tsim_affine();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->num_f = num_f;
  h->n_random = n_random;
  h->nnz = nnz;
  h->up.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  o.upload(h->up, lists, nnz, flip);
  h->o = o;
  if (const hipError_t e = h->up.err; e != hipSuccess) {
    tsim_affine_destroy(h);
    return tsim_fail(TSIM_EHIP, "affine sampler upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_affine_destroy(tsim_affine *h) {
  if (!h) return;
  h->up.release(h->device, h->stream);
  delete h;
}

extern "C" int tsim_affine_sample_device(tsim_affine *h, const uint64_t *d_f, int64_t f_row_bytes, int64_t B, int64_t first_shot,
                                         uint32_t key_hi, uint32_t key_lo, uint8_t *d_out, int64_t out_row_bytes,
                                         int32_t out_packed, int32_t col0, int32_t n_cols, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  const outh::InRows f_rows{"f_row_bytes", f_row_bytes, (h->num_f + 7) / 8};
  bool run = false;
  const int rc = outh::check_request(h->o.n_out, B, &first_shot, col0, n_cols, &f_rows, out_row_bytes, out_packed,
                                     d_out && (h->num_f == 0 || d_f), &run);
  if (rc != TSIM_OK || !run) return rc;
  HIP_TRY(hipSetDevice(h->device));
  affk::Args A;
  A.m = h->o.args(B, d_out, out_row_bytes, out_packed, col0, n_cols);
  h->o.fill_in(A.m, reinterpret_cast<const uint8_t *>(d_f), f_row_bytes, (int)f_rows.used, h->num_f > 0);
  A.num_f = h->num_f;
  A.k0 = key_hi;
  A.k1 = key_lo;
  A.tile0 = first_shot / 64;
  const outh::Outputs::Launch g = h->o.geometry((B + 63) / 64);
  void (*k)(affk::Args) = out_packed ? affk::k_affine<true> : affk::k_affine<false>;
  hipLaunchKernelGGL(k, dim3(g.blocks), dim3(64 * g.nw), g.lds, stream ? (hipStream_t)stream : h->stream, A);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_affine_info(const tsim_affine *h, int64_t out[8]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  out[0] = h->num_f;
  out[1] = h->n_random;
  out[2] = h->o.n_out;
  out[3] = h->nnz;
  out[4] = h->device;
  out[5] = h->o.win;
  out[6] = h->o.n_win;
  out[7] = outh::lds_per_wave(h->o.win);
  return TSIM_OK;
}
