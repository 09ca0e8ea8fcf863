// tsim_frame.hip - the Pauli-frame sampler (tsim_frame_*): a handle of its own, bound to one device, holding the compiled
// form of tsim_amd/frame.py (operation batches, noise sites and their tables, output lists) and the record-flip scratch; the
// kernels are csrc/tsim_frame.hip.h.
#include "tsim_host.hip.h"
#include "tsim_frame.hip.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {
constexpr int64_t kFrameLds = 160 * 1024;         // the frames of a tile: all the LDS a workgroup may take
constexpr int kMaxT = 32;                         // words per tile
constexpr int64_t kScratchBudget = 256ll << 20;   // bytes of F: a request is cut into launches that fit
constexpr int64_t kMaxLaunchWords = 1 << 14;      // 2^20 shots
constexpr int kOutLds = 64 * 1024;                // dynamic LDS per block of the output stage
constexpr int kWindow = 2048;                     // columns per window when one wave's LDS cannot hold every column's mask
constexpr int64_t kMaxWindowedRowPtr = 1ll << 28;
constexpr int64_t kMaxShot = 1ll << 38;
}  // namespace

struct tsim_frame {
  int device = -1;
  int32_t nq = 0, n_rec = 0, n_hidden = 0, n_random = 0, n_out = 0, n_ops = 0, n_batches = 0, n_sites = 0;
  int32_t log2T = 0, max_items = 0;
  int32_t win = 0, n_win = 1;
  int64_t max_words = 0;  // words per launch = row stride of F
  std::vector<void *> bufs;
  frmk::Form form{};
  int32_t *d_row_ptr = nullptr, *d_cols = nullptr;
  uint8_t *d_const = nullptr;
  uint64_t *d_F = nullptr;
  hipStream_t stream = nullptr;
  bool attr_set = false;
};

static void frame_release(tsim_frame *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : h->bufs) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

static int64_t out_lds_per_wave(int64_t win) { return win * 8 + m2dk::kStageBytes; }

template <typename T>
static hipError_t upload(tsim_frame *h, const T *src, size_t n, const T **dst) {
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T));
  if (e != hipSuccess) return e;
  h->bufs.push_back(p);
  *dst = static_cast<const T *>(p);
  return n ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
}

extern "C" int tsim_frame_create(int32_t device, const tsim_frame_desc *d, tsim_frame **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!d) return tsim_fail(TSIM_EINVAL, "desc is NULL");
  const int32_t nq = d->n_qubits, n_rec = d->n_records, n_hid = d->n_hidden, n_out = d->n_out;
  if (nq < 1 || n_rec < 0 || n_hid < 0 || d->n_random < 0 || n_out < 0 || d->n_ops < 0 || d->n_batches < 0 || d->n_sites < 0 ||
      d->n_bits < 0 || d->n_targets < 0 || d->n_tables < 0 || d->n_outcomes < 0 || d->n_gaps < 0 || d->n_cols < 0 ||
      (int64_t)n_rec + n_hid > 0x3FFFFFFF || (int64_t)n_rec + d->n_random > 0x7FFFFFC0ll)
    return tsim_fail(TSIM_EINVAL, "bad sizes");
  if (16ll * nq > kFrameLds)
    return tsim_fail(TSIM_ENOTSUP, "%d qubits (the auxiliary one included): the frames of ONE 64-shot word, 16 bytes per qubit, must fit "
                     "the %lld KiB of LDS of a workgroup - at most %lld qubits", nq, (long long)(kFrameLds / 1024), (long long)(kFrameLds / 16));
  if ((d->n_ops && (!d->op_kind || !d->op_a || !d->op_b || !d->op_c)) || !d->batch_ptr || !d->out_ptr || (n_out && !d->out_const) ||
      (d->n_cols && !d->out_cols) ||
      (d->n_sites && (!d->site_chan || !d->site_table || !d->site_bit || !d->bit_ptr || !d->table_ptr || !d->table_gap || !d->out_vals ||
                      !d->out_thr || !d->gap_thr)) || (d->n_targets && !d->targets))
    return tsim_fail(TSIM_EINVAL, "NULL array");
  const int32_t n_rows = n_rec + n_hid;
  // ---- every index the kernels follow is checked here
  if (d->batch_ptr[0] != 0 || d->batch_ptr[d->n_batches] != d->n_ops) return tsim_fail(TSIM_EINVAL, "batch_ptr must run from 0 to n_ops");
  if (d->n_sites) {
    if (d->site_bit[0] != 0 || d->site_bit[d->n_sites] != d->n_bits || d->bit_ptr[0] != 0 || d->bit_ptr[d->n_bits] != d->n_targets ||
        d->table_ptr[0] != 0 || d->table_ptr[d->n_tables] != d->n_outcomes)
      return tsim_fail(TSIM_EINVAL, "site_bit / bit_ptr / table_ptr must run from 0 to their array's length");
    for (int32_t i = 0; i < d->n_bits; ++i)
      if (d->bit_ptr[i + 1] < d->bit_ptr[i]) return tsim_fail(TSIM_EINVAL, "bit_ptr decreases at %d", i);
    for (int32_t t = 0; t < d->n_tables; ++t) {
      if (d->table_ptr[t + 1] <= d->table_ptr[t]) return tsim_fail(TSIM_EINVAL, "table %d has no outcome", t);
      if (d->table_gap[t] < 0 || d->table_gap[t] >= d->n_gaps) return tsim_fail(TSIM_EINVAL, "table %d: gap row %d of %d", t, d->table_gap[t], d->n_gaps);
      for (int32_t o = d->table_ptr[t]; o + 1 < d->table_ptr[t + 1]; ++o)
        if (d->out_thr[o + 1] < d->out_thr[o]) return tsim_fail(TSIM_EINVAL, "table %d: thresholds decrease", t);
    }
    for (int32_t g = 0; g < d->n_gaps; ++g)
      for (int k = 0; k + 1 < 64; ++k)
        if (d->gap_thr[64 * g + k + 1] > d->gap_thr[64 * g + k]) return tsim_fail(TSIM_EINVAL, "gap row %d increases", g);
    for (int32_t s = 0; s < d->n_sites; ++s) {
      const int32_t k = d->site_bit[s + 1] - d->site_bit[s], t = d->site_table[s];
      if (k < 1 || k > 32) return tsim_fail(TSIM_EINVAL, "site %d has %d error bits (1 .. 32)", s, k);
      if (t < 0 || t >= d->n_tables) return tsim_fail(TSIM_EINVAL, "site %d: table %d of %d", s, t, d->n_tables);
      for (int32_t o = d->table_ptr[t]; o < d->table_ptr[t + 1]; ++o)
        if (k < 32 && (d->out_vals[o] >> k)) return tsim_fail(TSIM_EINVAL, "site %d: outcome %u has a bit beyond its %d", s, d->out_vals[o], k);
    }
    for (int32_t i = 0; i < d->n_targets; ++i) {
      const int32_t tg = d->targets[i], idx = tg >> 2, kind = tg & 3;
      if (tg < 0 || kind > 2 || idx >= (kind == 2 ? n_rows : nq)) return tsim_fail(TSIM_EINVAL, "targets[%d] = %d", i, tg);
    }
  }
  int32_t max_items = 0;
  std::vector<int32_t> seen_b, seen_i;  // per qubit / record: the last batch and item that touched it
  try {
    seen_b.assign((size_t)nq + n_rows, -1);
    seen_i.assign((size_t)nq + n_rows, -1);
  } catch (const std::bad_alloc &) {
    return tsim_fail(TSIM_ENOMEM, "out of host memory");
  }
  auto touch = [&](int32_t b, int32_t i, int32_t r) {  // false: another item of the batch has it already
    if (seen_b[r] == b && seen_i[r] != i) return false;
    seen_b[r] = b;
    seen_i[r] = i;
    return true;
  };
  for (int32_t b = 0; b < d->n_batches; ++b) {
    const int32_t lo = d->batch_ptr[b], hi = d->batch_ptr[b + 1];
    if (hi <= lo || hi > d->n_ops) return tsim_fail(TSIM_EINVAL, "batch %d is empty or runs past the operations", b);
    if (hi - lo > (0x7FFFFFFF >> 5)) return tsim_fail(TSIM_ENOTSUP, "batch %d has %d items", b, hi - lo);
    max_items = std::max(max_items, hi - lo);
    const int kind = d->op_kind[lo];
    if (kind > frmk::kNoise) return tsim_fail(TSIM_EINVAL, "operation kind %d", kind);
    for (int32_t i = lo; i < hi; ++i) {
      const int32_t a = d->op_a[i], bb = d->op_b[i];
      bool ok = d->op_kind[i] == kind;
      switch (kind) {
        case frmk::kH: case frmk::kS: case frmk::kReset: ok = ok && a >= 0 && a < nq; break;
        case frmk::kCX: ok = ok && a >= 0 && a < nq && bb >= 0 && bb < nq && a != bb; break;
        case frmk::kMeasure: ok = ok && a >= -1 && a < nq && bb >= 0 && bb < n_rows; break;
        case frmk::kFeedback: ok = ok && a >= 0 && a < n_rows && bb >= 0 && bb < nq; break;
        default: ok = ok && a >= 0 && a < d->n_sites; break;
      }
      if (!ok) return tsim_fail(TSIM_EINVAL, "operation %d (kind %d: %d, %d) of batch %d", i, (int)d->op_kind[i], a, bb, b);
      switch (kind) {
        case frmk::kH: case frmk::kS: case frmk::kReset: ok = touch(b, i, a); break;
        case frmk::kCX: ok = touch(b, i, a) && touch(b, i, bb); break;
        case frmk::kMeasure: ok = (a < 0 || touch(b, i, a)) && touch(b, i, nq + bb); break;
        case frmk::kFeedback: ok = touch(b, i, nq + a) && touch(b, i, bb); break;
        default:
          for (int32_t t = d->bit_ptr[d->site_bit[a]]; ok && t < d->bit_ptr[d->site_bit[a + 1]]; ++t)
            ok = touch(b, i, (d->targets[t] & 3) == 2 ? nq + (d->targets[t] >> 2) : d->targets[t] >> 2);
          break;
      }
      if (!ok) return tsim_fail(TSIM_EINVAL, "batch %d: operation %d touches a qubit or record that another of its items touches", b, i);
    }
  }
  if (d->out_ptr[0] != 0 || d->out_ptr[n_out] != d->n_cols) return tsim_fail(TSIM_EINVAL, "out_ptr must run from 0 to n_cols");
  for (int32_t j = 0; j < n_out; ++j)
    if (d->out_ptr[j + 1] < d->out_ptr[j]) return tsim_fail(TSIM_EINVAL, "out_ptr decreases at output %d", j);
  const int32_t M = n_rec + d->n_random;
  for (int32_t k = 0; k < d->n_cols; ++k)
    if (d->out_cols[k] < 0 || d->out_cols[k] >= M)
      return tsim_fail(TSIM_EINVAL, "out_cols[%d] = %d is not a column (0 .. %d: %d records, then %d random symbols)", k, d->out_cols[k],
                       M - 1, n_rec, d->n_random);
  // ---- T: the most words whose frames fit
  int32_t log2T = 0;
  while ((2 << log2T) <= kMaxT && 16ll * nq * (2 << log2T) <= kFrameLds) ++log2T;
  const int64_t T = 1ll << log2T;
  int64_t max_words = std::min<int64_t>(kMaxLaunchWords, kScratchBudget / (8 * std::max<int64_t>(1, n_rows)));
  max_words = std::max<int64_t>(T, max_words / T * T);
  // ---- the output stage's windows (as tsim_affine_create builds them)
  const int32_t *row_ptr = d->out_ptr, *cols = d->out_cols;
  const int32_t nnz = d->n_cols;
  int32_t win = 0, n_win = 1;
  if (out_lds_per_wave(((int64_t)M + 63) / 64 * 64) <= kOutLds) {
    win = std::max(64, (M + 63) / 64 * 64);
  } else {
    win = kWindow;
    n_win = (int32_t)(((int64_t)M + kWindow - 1) / kWindow);
  }
  if ((int64_t)n_win * ((int64_t)n_out + 1) > kMaxWindowedRowPtr)
    return tsim_fail(TSIM_ENOTSUP, "%d columns x %d outputs: %d windows of %d columns, more than %lld row pointers", M, n_out, n_win, kWindow,
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
  tsim_frame *h = new (std::nothrow) tsim_frame();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->nq = nq;
  h->n_rec = n_rec;
  h->n_hidden = n_hid;
  h->n_random = d->n_random;
  h->n_out = n_out;
  h->n_ops = d->n_ops;
  h->n_batches = d->n_batches;
  h->n_sites = d->n_sites;
  h->log2T = log2T;
  h->max_items = max_items;
  h->win = win;
  h->n_win = n_win;
  h->max_words = max_words;
  frmk::Form &f = h->form;
  f.n_batches = d->n_batches;
  f.nq = nq;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  const size_t no = (size_t)d->n_ops, ns = (size_t)d->n_sites;
#define UP(field, n) if (e == hipSuccess) e = upload(h, d->field, (size_t)(n), &f.field)
  UP(op_kind, no); UP(op_a, no); UP(op_b, no); UP(op_c, no); UP(batch_ptr, d->n_batches + 1);
  UP(site_chan, ns); UP(site_table, ns); UP(site_bit, ns + 1); UP(bit_ptr, d->n_bits + 1); UP(targets, d->n_targets);
  UP(table_ptr, d->n_tables + 1); UP(table_gap, d->n_tables); UP(out_vals, d->n_outcomes); UP(out_thr, d->n_outcomes);
  UP(gap_thr, 64 * (size_t)d->n_gaps);
#undef UP
  const int32_t *drp = nullptr, *dc = nullptr;
  const uint8_t *dk = nullptr;
  if (e == hipSuccess) e = upload(h, row_ptr, (size_t)n_win * (n_out + 1), &drp);
  if (e == hipSuccess) e = upload(h, cols, (size_t)nnz, &dc);
  if (e == hipSuccess) e = upload(h, d->out_const, (size_t)n_out, &dk);
  if (e == hipSuccess) {
    void *p = nullptr;
    e = hipMalloc(&p, (size_t)std::max<int64_t>(1, n_rows) * (size_t)max_words * 8);
    if (e == hipSuccess) {
      h->bufs.push_back(p);
      h->d_F = static_cast<uint64_t *>(p);
    }
  }
  if (e != hipSuccess) {
    frame_release(h);
    delete h;
    return tsim_fail(TSIM_EHIP, "frame sampler upload: %s", hipGetErrorString(e));
  }
  h->d_row_ptr = const_cast<int32_t *>(drp);
  h->d_cols = const_cast<int32_t *>(dc);
  h->d_const = const_cast<uint8_t *>(dk);
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_frame_destroy(tsim_frame *h) {
  if (!h) return;
  frame_release(h);
  delete h;
}

extern "C" int tsim_frame_sample_device(tsim_frame *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
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
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int T = 1 << h->log2T;
  const size_t frame_lds = 16 * (size_t)h->nq * T;
  // threads of a block: what the largest batch keeps busy, 4 .. 16 waves (a block is often alone on its CU: waves hide latency)
  const int threads = (int)std::min<int64_t>(frmk::kMaxThreads, std::max<int64_t>(256, ((int64_t)h->max_items * T + 63) / 64 * 64));
  if (!h->attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void *)frmk::k_frame, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFrameLds));
    h->attr_set = true;
  }
  uint32_t n0 = 0x6E6F6973u, n1 = 0x6672616Du;  // the request's noise key: threefry2x32(key, ("nois", "fram"))
  tsimk::threefry2x32(key_hi, key_lo, n0, n1);
  const int per_wave = (int)out_lds_per_wave(h->win);
  const int nw = std::max(1, std::min(m2dk::kMaxWaves, kOutLds / per_wave));
  for (int64_t done = 0; done < B; done += h->max_words * 64) {  // launches whose flip words fit the scratch, in stream order
    const int64_t rows = std::min<int64_t>(B - done, h->max_words * 64), words = (rows + 63) / 64;
    frmk::Args A;
    A.f = h->form;
    A.F = h->d_F;
    A.stride = h->max_words;
    A.words = words;
    A.tile0 = (first_shot + done) / 64;
    A.log2T = h->log2T;
    A.n0 = n0;
    A.n1 = n1;
    hipLaunchKernelGGL(frmk::k_frame, dim3((unsigned)((words + T - 1) / T)), dim3(threads), frame_lds, s, A);
    HIP_TRY(hipGetLastError());
    uint8_t *dst = d_out + done * out_row_bytes;
    frmk::OutArgs O;
    m2dk::Args &a = O.m;
    a.in = nullptr;
    a.B = rows;
    a.in_rb = 0;
    a.M = h->n_rec + h->n_random;
    a.in_used = 0;
    a.in_contig = 0;
    a.in_w4 = 0;
    a.row_ptr = h->d_row_ptr;
    a.cols = h->d_cols;
    a.ref = h->d_const;
    a.col0 = col0;
    a.n_cols = n_cols;
    a.out = dst;
    a.out_rb = out_row_bytes;
    a.out_used = (int)out_used;
    a.out_contig = out_row_bytes == out_used && out_row_bytes <= 64;
    a.out_w4 = (out_row_bytes % 4 == 0 || a.out_contig) && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    a.n_out = h->n_out;
    a.win = h->win;
    a.n_win = h->n_win;
    O.F = h->d_F;
    O.stride = h->max_words;
    O.n_rec = h->n_rec;
    O.k0 = key_hi;
    O.k1 = key_lo;
    O.tile0 = A.tile0;
    const int64_t blocks = std::min<int64_t>((words + nw - 1) / nw, 256 * 8 * 4 / nw);
    void (*k)(frmk::OutArgs) = out_packed ? frmk::k_frame_out<true> : frmk::k_frame_out<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * nw), (size_t)nw * per_wave, s, O);
    HIP_TRY(hipGetLastError());
  }
  return TSIM_OK;
}

extern "C" int tsim_frame_info(const tsim_frame *h, int64_t out[16]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  out[0] = h->nq;
  out[1] = h->n_rec;
  out[2] = h->n_hidden;
  out[3] = h->n_random;
  out[4] = h->n_out;
  out[5] = h->n_ops;
  out[6] = h->n_batches;
  out[7] = h->n_sites;
  out[8] = h->device;
  out[9] = 1ll << h->log2T;
  out[10] = 16ll * h->nq * (1ll << h->log2T);
  out[11] = kFrameLds / 16;
  out[12] = h->win;
  out[13] = h->n_win;
  out[14] = h->max_words;
  out[15] = h->max_items;
  return TSIM_OK;
}
