// tsim_frame.hip - the Pauli-frame sampler (tsim_frame_*): a handle of its own, bound to one device, holding the compiled
// form of tsim_amd/frame.py (operation batches, noise sites and their tables, output lists) and the record-flip scratch; the
// kernels are csrc/tsim_frame.hip.h.
#include "tsim_outputs_host.hip.h"
#include "tsim_frame.hip.h"

namespace {
constexpr int64_t kFrameLds = 160 * 1024;         // the frames of a tile: all the LDS a workgroup may take
constexpr int kMaxT = 32;                         // words per tile
constexpr int64_t kScratchBudget = 256ll << 20;   // bytes of F: a request is cut into launches that fit
constexpr int64_t kMaxLaunchWords = 1 << 14;      // 2^20 shots
}  // namespace

struct tsim_frame {
  int device = -1;
  int32_t nq = 0, n_rec = 0, n_hidden = 0, n_random = 0, n_ops = 0, n_batches = 0, n_sites = 0;
  int32_t log2T = 0, max_items = 0;
  int64_t max_words = 0;  // words per launch = row stride of F
  frmk::Form form{};
  outh::Outputs o;     // the output stage, over the n_rec + n_random columns (csrc/tsim_outputs_host.hip.h)
  tsimh::Uploads up;   // the form's arrays, the output stage's lists and constant bits, F
  uint64_t *d_F = nullptr;
  hipStream_t stream = nullptr;
  bool attr_set = false;
};

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
  // ---- the output stage's windows; a form without a column still has one word of masks
  outh::Outputs o;
  if (o.plan(M, n_out, 64) > outh::kMaxWindowedRowPtr)
    return tsim_fail(TSIM_ENOTSUP, "%d columns x %d outputs: %d windows of %d columns, more than %lld row pointers", M, n_out, o.n_win,
                     outh::kWindow, (long long)outh::kMaxWindowedRowPtr);
  outh::Lists lists;
  if (const int rc = o.build(d->out_ptr, d->out_cols, &lists)) return rc;
  if (const int rc = tsimh::open_device(device, nullptr)) return rc;
  tsim_frame *h = new (std::nothrow) tsim_frame();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->nq = nq;
  h->n_rec = n_rec;
  h->n_hidden = n_hid;
  h->n_random = d->n_random;
  h->n_ops = d->n_ops;
  h->n_batches = d->n_batches;
  h->n_sites = d->n_sites;
  h->log2T = log2T;
  h->max_items = max_items;
  h->max_words = max_words;
  frmk::Form &f = h->form;
  f.n_batches = d->n_batches;
  f.nq = nq;
  tsimh::Uploads &up = h->up;
  up.err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  const size_t no = (size_t)d->n_ops, ns = (size_t)d->n_sites;
#define UP(field, n) f.field = up.put(d->field, (size_t)(n))
  UP(op_kind, no); UP(op_a, no); UP(op_b, no); UP(op_c, no); UP(batch_ptr, d->n_batches + 1);
  UP(site_chan, ns); UP(site_table, ns); UP(site_bit, ns + 1); UP(bit_ptr, d->n_bits + 1); UP(targets, d->n_targets);
  UP(table_ptr, d->n_tables + 1); UP(table_gap, d->n_tables); UP(out_vals, d->n_outcomes); UP(out_thr, d->n_outcomes);
  UP(gap_thr, 64 * (size_t)d->n_gaps);
#undef UP
  o.upload(up, lists, d->n_cols, d->out_const);
  h->o = o;
  h->d_F = static_cast<uint64_t *>(up.room((size_t)std::max<int64_t>(1, n_rows) * (size_t)max_words * 8));
  if (const hipError_t e = up.err; e != hipSuccess) {
    tsim_frame_destroy(h);
    return tsim_fail(TSIM_EHIP, "frame sampler upload: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_frame_destroy(tsim_frame *h) {
  if (!h) return;
  h->up.release(h->device, h->stream);
  delete h;
}

extern "C" int tsim_frame_sample_device(tsim_frame *h, int64_t B, int64_t first_shot, uint32_t key_hi, uint32_t key_lo, uint8_t *d_out,
                                        int64_t out_row_bytes, int32_t out_packed, int32_t col0, int32_t n_cols, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "sampler is NULL");
  bool run = false;
  const int rc = outh::check_request(h->o.n_out, B, &first_shot, col0, n_cols, nullptr, out_row_bytes, out_packed, d_out != nullptr, &run);
  if (rc != TSIM_OK || !run) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int T = 1 << h->log2T;
  const size_t frame_lds = 16 * (size_t)h->nq * T;
  // threads of a block: what the largest batch keeps busy, 4 .. 16 waves (a block is often alone on its CU: waves hide latency)
  const int threads = (int)std::min<int64_t>(frmk::kMaxThreads, std::max<int64_t>(256, ((int64_t)h->max_items * T + 63) / 64 * 64));
  void (*const frame_kernels[])(frmk::Args) = {frmk::k_frame};
  if (const int rc = tsimh::allow_lds(frame_kernels, kFrameLds, &h->attr_set)) return rc;
  uint32_t n0 = 0x6E6F6973u, n1 = 0x6672616Du;  // the request's noise key: threefry2x32(key, ("nois", "fram"))
  tsimk::threefry2x32(key_hi, key_lo, n0, n1);
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
    frmk::OutArgs O;
    O.m = h->o.args(rows, d_out + done * out_row_bytes, out_row_bytes, out_packed, col0, n_cols);
    O.F = h->d_F;
    O.stride = h->max_words;
    O.n_rec = h->n_rec;
    O.k0 = key_hi;
    O.k1 = key_lo;
    O.tile0 = A.tile0;
    const outh::Outputs::Launch g = h->o.geometry(words);
    void (*k)(frmk::OutArgs) = out_packed ? frmk::k_frame_out<true> : frmk::k_frame_out<false>;
    hipLaunchKernelGGL(k, dim3(g.blocks), dim3(64 * g.nw), g.lds, s, O);
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
  out[4] = h->o.n_out;
  out[5] = h->n_ops;
  out[6] = h->n_batches;
  out[7] = h->n_sites;
  out[8] = h->device;
  out[9] = 1ll << h->log2T;
  out[10] = 16ll * h->nq * (1ll << h->log2T);
  out[11] = kFrameLds / 16;
  out[12] = h->o.win;
  out[13] = h->o.n_win;
  out[14] = h->max_words;
  out[15] = h->max_items;
  return TSIM_OK;
}
