// tsim_faults.hip - the fault-driven detector sampler (tsim_faults_*): a handle of its own, bound to one device, holding the
// compiled form of tsim_amd/faults.py (classes of noise sites, their tables, the error bit -> outputs CSR); the kernel is
// csrc/tsim_faults.hip.h.  The same handle draws rows conditioned on exactly k fired sites (tsim_amd/fixed_weight.py) once
// tsim_faults_set_split gave it the table of the class counts; that kernel is csrc/tsim_faults_weight.hip.h.
#include "tsim_outputs_host.hip.h"
#include "tsim_faults_weight.hip.h"

namespace {
constexpr int64_t kLds = 160 * 1024;          // all the LDS a workgroup may take
constexpr int32_t kMaxClassSites = 1 << 25;   // the draw index has 26 bits: a class needs at most n_c + n_c / kGapK + 2 draws

// The LDS of a block: the tables (tab_bytes, 0 when they stay in global memory), then per wave one row of S 32-bit words per
// lane plus wave_extra bytes.  S is the outputs' words made odd when one wave's share fits, and the block then has as many
// waves (at most kMaxWaves) as fit; otherwise one wave with the widest odd row that fits, the outputs going through in windows
// of 32 S columns.  k_faults: wave_extra = 0.  k_faults_weight: wave_extra = 4 * kListWords = 8 KiB, the fired-position list.
void lds_rule(int64_t tab_bytes, int64_t wave_extra, int32_t n_out, int32_t *S_out, int32_t *waves_out, int32_t *win_out) {
  const int64_t avail = kLds - tab_bytes;
  const int64_t words_all = std::max<int64_t>(1, ((int64_t)n_out + 31) / 32);
  int64_t S = words_all | 1;  // odd
  int32_t waves = 1;
  if (256 * S + wave_extra <= avail) {
    waves = (int32_t)std::min<int64_t>(fltk::kMaxWaves, avail / (256 * S + wave_extra));
  } else {  // windows: the widest odd row one wave can keep
    S = (avail - wave_extra) / 256;
    if (!(S & 1)) --S;
  }
  *S_out = (int32_t)S;
  *waves_out = waves;
  *win_out = (int32_t)std::min<int64_t>(32 * S, 32 * words_all);
}
}  // namespace

struct tsim_faults {
  int device = -1;
  int32_t n_out = 0, num_e = 0, n_sites = 0, n_classes = 0, n_gaps = 0, n_cols = 0, max_class = 0;
  int32_t tab_lds = 0, S = 1, win = 32, waves = 1;
  int64_t tab_bytes = 0;
  tsimh::Uploads up;  // the form's arrays
  fltk::Form form{};
  hipStream_t stream = nullptr;
  bool attr_set = false;
  // ---- fixed weight (tsim_faults_set_split)
  std::vector<int32_t> class_n;   // sites per class
  int32_t always_class = -1;      // the first class whose gap row is all zero (p_fire = 1), -1: none
  int32_t kmax = -1;              // of the split table, -1: none
  uint32_t *split = nullptr;      // device, [n_classes][kmax + 1][kmax + 1]
  int32_t w_tab_lds = 0, w_S = 1, w_win = 32, w_waves = 1;
  int64_t w_tab_bytes = 0, split_bytes = 0;
  bool w_attr_set = false;
};

// both kernels by 2 * (byte rows) + (tables in global memory)
void (*const kFaults[4])(fltk::Args) = {fltk::k_faults<true, true>, fltk::k_faults<true, false>, fltk::k_faults<false, true>,
                                        fltk::k_faults<false, false>};
void (*const kFaultsWeight[4])(fltk::WeightArgs) = {fltk::k_faults_weight<true, true>, fltk::k_faults_weight<true, false>,
                                                    fltk::k_faults_weight<false, true>, fltk::k_faults_weight<false, false>};

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
  const int64_t words_all = std::max<int64_t>(1, ((int64_t)n_out + 31) / 32);
  int32_t S = 1, waves = 1, win = 32;
  lds_rule(tab_bytes, 0, n_out, &S, &waves, &win);
  std::vector<uint32_t> cwords;
  try {
    cwords.assign((size_t)words_all + 2, 0u);
  } catch (const std::bad_alloc &) {
    return tsim_fail(TSIM_ENOMEM, "out of host memory");
  }
  for (int32_t j = 0; j < n_out; ++j)
    if (d->out_const[j] & 1) cwords[j >> 5] |= 1u << (j & 31);
  if (const int rc = tsimh::open_device(device, nullptr)) return rc;
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
  h->S = S;
  h->win = win;
  h->waves = waves;
  try {
    h->class_n.resize((size_t)n_cls);
  } catch (const std::bad_alloc &) {
    delete h;
    return tsim_fail(TSIM_ENOMEM, "out of host memory");
  }
  for (int32_t c = n_cls - 1; c >= 0; --c) {
    h->class_n[c] = d->class_ptr[c + 1] - d->class_ptr[c];
    if (d->gap_thr[(size_t)fltk::kGapK * d->table_gap[c]] == 0) h->always_class = c;  // (a gap row does not increase)
  }
  fltk::Form &f = h->form;
  f.n_classes = n_cls;
  f.n_gaps = d->n_gaps;
  f.n_outcomes = d->n_outcomes;
  tsimh::Uploads &up = h->up;
  up.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
#define UP(field, n) f.field = up.put(d->field, (size_t)(n))
  UP(class_ptr, n_cls + 1); UP(site_e0, n_sites); UP(table_ptr, n_cls + 1); UP(table_gap, n_cls);
  UP(out_vals, d->n_outcomes); UP(out_thr, d->n_outcomes); UP(gap_thr, (size_t)fltk::kGapK * d->n_gaps);
  UP(col_ptr, num_e + 1); UP(cols, d->n_cols);
#undef UP
  f.const_words = up.put(cwords);
  if (const hipError_t e = up.err; e != hipSuccess) {
    tsim_faults_destroy(h);
    return tsim_fail(TSIM_EHIP, "fault sampler upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_faults_destroy(tsim_faults *h) {
  if (!h) return;
  h->up.release(h->device, h->stream);
  if (h->split) (void)hipFree(h->split);
  delete h;
}

// The arguments both kernels take; the noise key is threefry2x32(key, (n0, n1)) of the counter given in A.n0, A.n1.
static void fill_args(fltk::Args &A, const tsim_faults *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
                      int64_t out_row_bytes, int32_t col0, int32_t n_cols, int32_t S, int32_t win) {
  A.f = h->form;
  A.B = B;
  A.g0 = first_shot;
  tsimk::threefry2x32(key_hi, key_lo, A.n0, A.n1);
  A.out = d_out;
  A.out_rb = out_row_bytes;
  A.out_w4 = out_row_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 4 == 0;
  A.col0 = col0;
  A.n_cols = n_cols;
  A.S = S;
  A.win = win;
  A.n_win = (n_cols + win - 1) / win;
}

extern "C" int tsim_faults_sample_device(tsim_faults *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
                                         int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  bool run = false;
  const int rc = outh::check_request(h->n_out, B, &first_shot, col0, n_cols, nullptr, out_row_bytes, out_packed, d_out != nullptr, &run);
  if (rc != TSIM_OK || !run) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (const int ra = tsimh::allow_lds(kFaults, kLds, &h->attr_set)) return ra;
  fltk::Args A;
  A.n0 = 0x6E6F6973u;  // the request's noise key: threefry2x32(key, ("nois", "falt"))
  A.n1 = 0x66616C74u;
  fill_args(A, h, B, first_shot, key_hi, key_lo, d_out, out_row_bytes, col0, n_cols, h->S, h->win);
  const int64_t tiles = (B + 63) / 64;
  const int nw = (int)std::min<int64_t>(h->waves, tiles);
  const size_t lds = (size_t)h->tab_bytes + (size_t)nw * 256 * (size_t)h->S;
  const int64_t blocks = std::min<int64_t>((tiles + nw - 1) / nw, 256 * 8);
  hipLaunchKernelGGL(kFaults[2 * !out_packed + !h->tab_lds], dim3((unsigned)blocks), dim3(64 * nw), lds, s, A);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

// ---- fixed weight -----------------------------------------------------------------------------------------------------------

extern "C" int tsim_faults_set_split(tsim_faults *h, int32_t kmax, const uint32_t *split_thr) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  if (kmax < 0 || kmax > fltk::kMaxWeight) return tsim_fail(TSIM_EINVAL, "kmax = %d (0 .. %d)", kmax, fltk::kMaxWeight);
  if (!split_thr) return tsim_fail(TSIM_EINVAL, "NULL table");
  if (h->always_class >= 0)
    return tsim_fail(TSIM_ENOTSUP, "class %d fires with probability 1 (an all-zero gap row): it has no odds", h->always_class);
  const int64_t kw = kmax + 1, n_cls = h->n_classes, n_words = n_cls * kw * kw;
  if (n_words > 0x7FFFFFFF) return tsim_fail(TSIM_ENOTSUP, "a split table of %lld entries", (long long)n_words);
  // ---- what keeps the kernel's walk inside the classes: rows do not decrease, and an entry m of row (c, r) that would leave
  //      the later classes more than they hold is zero (never picked), for every row a split can reach
  int64_t rest = 0;  // sites of the classes after c
  for (int64_t c = n_cls - 1; c >= 0; --c) {
    for (int64_t r = 0; r <= kmax; ++r) {
      const uint32_t *row = split_thr + (c * kw + r) * kw;
      for (int64_t m = 0; m + 1 < kw; ++m)
        if (row[m + 1] < row[m]) return tsim_fail(TSIM_EINVAL, "split row (%lld, %lld) decreases", (long long)c, (long long)r);
      if (r > rest + h->class_n[c]) continue;  // (no split can reach it)
      for (int64_t m = 0; m < std::min<int64_t>(r, h->class_n[c]) && r - m > rest; ++m)
        if (row[m] != 0)
          return tsim_fail(TSIM_EINVAL, "split row (%lld, %lld): %lld sites here would leave %lld to the %lld sites of the later classes",
                           (long long)c, (long long)r, (long long)m, (long long)(r - m), (long long)rest);
    }
    rest += h->class_n[c];
  }
  HIP_TRY(hipSetDevice(h->device));
  if (h->split) {  // (hipFree waits for the launches that read it)
    HIP_TRY(hipFree(h->split));
    h->split = nullptr;
    h->kmax = -1;
  }
  void *p = nullptr;
  HIP_TRY(hipMalloc(&p, std::max<size_t>(1, (size_t)n_words) * 4));
  h->split = static_cast<uint32_t *>(p);
  if (n_words) HIP_TRY(hipMemcpy(p, split_thr, (size_t)n_words * 4, hipMemcpyHostToDevice));
  // ---- LDS: the outcome tables and the split table when they are small (no gap rows here), then lds_rule with the list
  int64_t tab_bytes = (2ll * h->form.n_outcomes + n_words) * 4;
  h->w_tab_lds = tab_bytes <= fltk::kTabLdsBytes;
  h->w_tab_bytes = h->w_tab_lds ? (tab_bytes + 15) / 16 * 16 : 0;
  lds_rule(h->w_tab_bytes, 4 * fltk::kListWords, h->n_out, &h->w_S, &h->w_waves, &h->w_win);
  h->split_bytes = n_words * 4;
  h->kmax = kmax;
  return TSIM_OK;
}

extern "C" int tsim_faults_sample_weight_device(tsim_faults *h, int32_t k, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo,
                                                uint8_t *d_out, int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols,
                                                void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  if (h->kmax < 0) return tsim_fail(TSIM_ESTATE, "no split table: call tsim_faults_set_split first");
  if (k < 0 || k > h->kmax) return tsim_fail(TSIM_EINVAL, "k = %d: the split table serves 0 .. %d", k, h->kmax);
  if (k > h->n_sites) return tsim_fail(TSIM_EINVAL, "k = %d of %d noise sites", k, h->n_sites);
  bool run = false;
  const int rc = outh::check_request(h->n_out, B, &first_shot, col0, n_cols, nullptr, out_row_bytes, out_packed, d_out != nullptr, &run);
  if (rc != TSIM_OK || !run) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (const int ra = tsimh::allow_lds(kFaultsWeight, kLds, &h->w_attr_set)) return ra;
  fltk::WeightArgs W;
  W.a.n0 = 0x6E6F6973u;  // the request's noise key: threefry2x32(key, ("nois", "fixw")), a stream of its own
  W.a.n1 = 0x66697877u;
  fill_args(W.a, h, B, first_shot, key_hi, key_lo, d_out, out_row_bytes, col0, n_cols, h->w_S, h->w_win);
  W.split = h->split;
  W.k = k;
  W.kmax = h->kmax;
  const int64_t tiles = (B + 63) / 64;
  const int nw = (int)std::min<int64_t>(h->w_waves, tiles);
  const size_t lds = (size_t)h->w_tab_bytes + (size_t)nw * (256 * (size_t)h->w_S + 4 * fltk::kListWords);
  const int64_t blocks = std::min<int64_t>((tiles + nw - 1) / nw, 256 * 8);
  hipLaunchKernelGGL(kFaultsWeight[2 * !out_packed + !h->w_tab_lds], dim3((unsigned)blocks), dim3(64 * nw), lds, s, W);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_faults_weight_info(const tsim_faults *h, int64_t out[8]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  const bool have = h->kmax >= 0;
  out[0] = h->kmax;
  out[1] = have ? h->w_waves : 0;
  out[2] = have ? h->w_tab_bytes + (int64_t)h->w_waves * (256ll * h->w_S + 4 * fltk::kListWords) : 0;
  out[3] = have ? h->w_tab_lds : 0;
  out[4] = have ? h->w_S : 0;
  out[5] = have ? h->w_win : 0;
  out[6] = have ? ((int64_t)h->n_out + h->w_win - 1) / h->w_win : 0;
  out[7] = h->split_bytes;
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
