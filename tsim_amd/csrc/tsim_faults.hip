// tsim_faults.hip - the fault-driven detector sampler (tsim_faults_*): a handle of its own, bound to one device, holding the
// compiled form of tsim_amd/faults.py (classes of noise sites, their tables, the error bit -> outputs CSR); the kernel is
// csrc/tsim_faults.hip.h.
#include "../../include/tsim_hip.h"
#include "tsim_faults.hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

int tsim_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define FLT_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return tsim_fail(TSIM_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr int64_t kLds = 160 * 1024;          // all the LDS a workgroup may take
constexpr int32_t kMaxClassSites = 1 << 25;   // the draw index has 26 bits: a class needs at most n_c + n_c / kGapK + 2 draws
constexpr int64_t kMaxShot = 1ll << 38;
}  // namespace

struct tsim_faults {
  int device = -1;
  int32_t n_out = 0, num_e = 0, n_sites = 0, n_classes = 0, n_gaps = 0, n_cols = 0, max_class = 0;
  int32_t tab_lds = 0, S = 1, win = 32, waves = 1;
  int64_t tab_bytes = 0;
  std::vector<void *> bufs;
  fltk::Form form{};
  hipStream_t stream = nullptr;
  bool attr_set = false;
};

static void faults_release(tsim_faults *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : h->bufs) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

template <typename T>
static hipError_t upload(tsim_faults *h, const T *src, size_t n, const T **dst) {
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T));
  if (e != hipSuccess) return e;
  h->bufs.push_back(p);
  *dst = static_cast<const T *>(p);
  return n ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
}

extern "C" int tsim_faults_create(int32_t device, const tsim_faults_desc *d, tsim_faults **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!d) return tsim_fail(TSIM_EINVAL, "desc is NULL");
  const int32_t n_out = d->n_out, num_e = d->num_e, n_sites = d->n_sites, n_cls = d->n_classes;
  if (n_out < 0 || num_e < 0 || n_sites < 0 || n_cls < 0 || d->n_outcomes < 0 || d->n_gaps < 0 || d->n_cols < 0 || n_out > 0x7FFFFF00 ||
      num_e > 0x7FFFFF00 || d->n_gaps > 0x7FFFFFFF / fltk::kGapK)
    return tsim_fail(TSIM_EINVAL, "bad sizes");
  if (d->gap_k != fltk::kGapK) return tsim_fail(TSIM_EINVAL, "gap_k = %d: gap rows have %d entries", d->gap_k, fltk::kGapK);
  if (!d->class_ptr || !d->table_ptr || !d->col_ptr || (n_out && !d->out_const) || (d->n_cols && !d->cols) || (n_sites && !d->site_e0) ||
      (n_cls && (!d->table_bits || !d->table_gap || !d->out_vals || !d->out_thr || !d->gap_thr)))
    return tsim_fail(TSIM_EINVAL, "NULL array");
  // ---- every index the kernel follows is checked here
  if (d->class_ptr[0] != 0 || d->class_ptr[n_cls] != n_sites || d->table_ptr[0] != 0 || d->table_ptr[n_cls] != d->n_outcomes ||
      d->col_ptr[0] != 0 || d->col_ptr[num_e] != d->n_cols)
    return tsim_fail(TSIM_EINVAL, "class_ptr / table_ptr / col_ptr must run from 0 to their array's length");
  int32_t max_class = 0;
  for (int32_t c = 0; c < n_cls; ++c) {
    const int32_t s0 = d->class_ptr[c], n_c = d->class_ptr[c + 1] - s0, k = d->table_bits[c];
    if (n_c < 1) return tsim_fail(TSIM_EINVAL, "class %d has no site", c);
    if (n_c > kMaxClassSites)
      return tsim_fail(TSIM_ENOTSUP, "class %d has %d sites: the draw index has 26 bits, at most %d sites", c, n_c, kMaxClassSites);
    max_class = std::max(max_class, n_c);
    if (k < 1 || k > 32) return tsim_fail(TSIM_EINVAL, "class %d: %d error bits per site (1 .. 32)", c, k);
    if (d->table_ptr[c + 1] <= d->table_ptr[c]) return tsim_fail(TSIM_EINVAL, "table %d has no outcome", c);
    if (d->table_gap[c] < 0 || d->table_gap[c] >= d->n_gaps)
      return tsim_fail(TSIM_EINVAL, "table %d: gap row %d of %d", c, d->table_gap[c], d->n_gaps);
    for (int32_t o = d->table_ptr[c]; o < d->table_ptr[c + 1]; ++o) {
      if (o + 1 < d->table_ptr[c + 1] && d->out_thr[o + 1] < d->out_thr[o]) return tsim_fail(TSIM_EINVAL, "table %d: thresholds decrease", c);
      if (k < 32 && (d->out_vals[o] >> k)) return tsim_fail(TSIM_EINVAL, "table %d: outcome %u has a bit beyond its %d", c, d->out_vals[o], k);
    }
    for (int32_t s = s0; s < s0 + n_c; ++s)
      if (d->site_e0[s] < 0 || d->site_e0[s] > num_e - k)
        return tsim_fail(TSIM_EINVAL, "site %d of class %d: error bits %d .. + %d of %d", s - s0, c, d->site_e0[s], k, num_e);
  }
  for (int32_t g = 0; g < d->n_gaps; ++g)
    for (int k = 0; k + 1 < fltk::kGapK; ++k)
      if (d->gap_thr[(size_t)fltk::kGapK * g + k + 1] > d->gap_thr[(size_t)fltk::kGapK * g + k]) return tsim_fail(TSIM_EINVAL, "gap row %d increases", g);
  for (int32_t e = 0; e < num_e; ++e)
    if (d->col_ptr[e + 1] < d->col_ptr[e]) return tsim_fail(TSIM_EINVAL, "col_ptr decreases at error bit %d", e);
  for (int32_t k = 0; k < d->n_cols; ++k)
    if (d->cols[k] < 0 || d->cols[k] >= n_out) return tsim_fail(TSIM_EINVAL, "cols[%d] = %d is not an output (0 .. %d)", k, d->cols[k], n_out - 1);
  // ---- LDS: the tables when they are small, then one row of S words per lane and wave
  int64_t tab_bytes = ((int64_t)d->n_gaps * fltk::kGapK + 2ll * d->n_outcomes) * 4;
  const int32_t tab_lds = tab_bytes <= fltk::kTabLdsBytes;
  tab_bytes = tab_lds ? (tab_bytes + 15) / 16 * 16 : 0;
  const int64_t avail = kLds - tab_bytes;
  const int64_t words_all = std::max<int64_t>(1, ((int64_t)n_out + 31) / 32);
  int64_t S = words_all | 1;  // odd
  int32_t waves = 1;
  if (256 * S <= avail) {
    waves = (int32_t)std::min<int64_t>(fltk::kMaxWaves, avail / (256 * S));
  } else {  // windows: the widest odd row one wave can keep
    S = avail / 256;
    if (!(S & 1)) --S;
  }
  const int32_t win = (int32_t)std::min<int64_t>(32 * S, 32 * words_all);
  std::vector<uint32_t> cwords;
  try {
    cwords.assign((size_t)words_all + 2, 0u);
  } catch (const std::bad_alloc &) {
    return tsim_fail(TSIM_ENOMEM, "out of host memory");
  }
  for (int32_t j = 0; j < n_out; ++j)
    if (d->out_const[j] & 1) cwords[j >> 5] |= 1u << (j & 31);
  int count = 0;
  FLT_TRY(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) return tsim_fail(TSIM_EINVAL, "device %d of %d", device, count);
  FLT_TRY(hipSetDevice(device));
  tsim_faults *h = new (std::nothrow) tsim_faults();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->n_out = n_out;
  h->num_e = num_e;
  h->n_sites = n_sites;
  h->n_classes = n_cls;
  h->n_gaps = d->n_gaps;
  h->n_cols = d->n_cols;
  h->max_class = max_class;
  h->tab_lds = tab_lds;
  h->tab_bytes = tab_bytes;
  h->S = (int32_t)S;
  h->win = win;
  h->waves = waves;
  fltk::Form &f = h->form;
  f.n_classes = n_cls;
  f.n_gaps = d->n_gaps;
  f.n_outcomes = d->n_outcomes;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
#define UP(field, n) if (e == hipSuccess) e = upload(h, d->field, (size_t)(n), &f.field)
  UP(class_ptr, n_cls + 1); UP(site_e0, n_sites); UP(table_ptr, n_cls + 1); UP(table_gap, n_cls);
  UP(out_vals, d->n_outcomes); UP(out_thr, d->n_outcomes); UP(gap_thr, (size_t)fltk::kGapK * d->n_gaps);
  UP(col_ptr, num_e + 1); UP(cols, d->n_cols);
#undef UP
  if (e == hipSuccess) e = upload(h, cwords.data(), cwords.size(), &f.const_words);
  if (e != hipSuccess) {
    faults_release(h);
    delete h;
    return tsim_fail(TSIM_EHIP, "fault sampler upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_faults_destroy(tsim_faults *h) {
  if (!h) return;
  faults_release(h);
  delete h;
}

extern "C" int tsim_faults_sample_device(tsim_faults *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
                                         int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  if (B < 0) return tsim_fail(TSIM_EINVAL, "negative B");
  if (first_shot < 0 || first_shot % 64 != 0)
    return tsim_fail(TSIM_EINVAL, "first_shot = %lld is not a non-negative multiple of 64", (long long)first_shot);
  if (first_shot > kMaxShot || B > kMaxShot - first_shot)
    return tsim_fail(TSIM_EINVAL, "first_shot + B = %lld + %lld exceeds 2^38", (long long)first_shot, (long long)B);
  if (col0 < 0 || n_cols < 0 || (int64_t)col0 + n_cols > h->n_out)
    return tsim_fail(TSIM_EINVAL, "outputs %d .. %d + %d of %d", col0, col0, n_cols, h->n_out);
  const int64_t out_used = out_packed ? (n_cols + 7) / 8 : n_cols;
  if (out_row_bytes < out_used || out_row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "out_row_bytes = %lld for %lld bytes per row", (long long)out_row_bytes, (long long)out_used);
  if (B == 0 || n_cols == 0) return TSIM_OK;
  if (!d_out) return tsim_fail(TSIM_EINVAL, "NULL buffer");
  FLT_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  void (*k)(fltk::Args) = out_packed ? (h->tab_lds ? fltk::k_faults<true, true> : fltk::k_faults<true, false>)
                                     : (h->tab_lds ? fltk::k_faults<false, true> : fltk::k_faults<false, false>);
  if (!h->attr_set) {
    FLT_TRY(hipFuncSetAttribute((const void *)fltk::k_faults<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    FLT_TRY(hipFuncSetAttribute((const void *)fltk::k_faults<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    FLT_TRY(hipFuncSetAttribute((const void *)fltk::k_faults<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    FLT_TRY(hipFuncSetAttribute((const void *)fltk::k_faults<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    h->attr_set = true;
  }
  fltk::Args A;
  A.f = h->form;
  A.B = B;
  A.g0 = first_shot;
  A.n0 = 0x6E6F6973u;  // the request's noise key: threefry2x32(key, ("nois", "falt"))
  A.n1 = 0x66616C74u;
  tsimk::threefry2x32(key_hi, key_lo, A.n0, A.n1);
  A.out = d_out;
  A.out_rb = out_row_bytes;
  A.out_w4 = out_row_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 4 == 0;
  A.col0 = col0;
  A.n_cols = n_cols;
  A.S = h->S;
  A.win = h->win;
  A.n_win = (n_cols + h->win - 1) / h->win;
  const int64_t tiles = (B + 63) / 64;
  const int nw = (int)std::min<int64_t>(h->waves, tiles);
  const size_t lds = (size_t)h->tab_bytes + (size_t)nw * 256 * (size_t)h->S;
  const int64_t blocks = std::min<int64_t>((tiles + nw - 1) / nw, 256 * 8);
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * nw), lds, s, A);
  FLT_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_faults_info(const tsim_faults *h, int64_t out[16]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  out[0] = h->n_out;
  out[1] = h->num_e;
  out[2] = h->n_sites;
  out[3] = h->n_classes;
  out[4] = h->device;
  out[5] = fltk::kGapK;
  out[6] = h->win;
  out[7] = ((int64_t)h->n_out + h->win - 1) / h->win;
  out[8] = h->S;
  out[9] = h->waves;
  out[10] = h->tab_bytes + (int64_t)h->waves * 256 * h->S;
  out[11] = h->tab_lds;
  out[12] = h->n_gaps;
  out[13] = h->n_cols;
  out[14] = h->max_class;
  out[15] = 32 * ((kLds / 256 - 1) | 1);
  return TSIM_OK;
}
