// tsim_shotdata.hip - stim's shot-data formats on the device (tsim_shotdata_*): a small handle per device holding the
// scan scratch, a result block and its pinned mirror, a stream and grow-only staging buffers; the kernels are
// csrc/tsim_shotdata.hip.h.
#include "tsim_host.hip.h"
#include "tsim_shotdata.hip.h"

#include <algorithm>
#include <new>

int tsim_launch_compact(const uint64_t *d_in, int64_t B, int32_t WO, int32_t nbits, uint8_t *d_out, hipStream_t s);  // tsim_format.hip

namespace {
constexpr int kSlots = 16;
constexpr int64_t kMaxItems = 1ll << 31;     // rows of an encode call, bytes of a decode chunk
constexpr int64_t kLaunchItems = 1ll << 30;  // work-items of one fixed-size encode launch
}  // namespace

struct tsim_shotdata {
  int device = -1;
  hipStream_t stream = nullptr;
  long long *d_scratch = nullptr;  // per-row offsets and per-block sums (grow-only)
  int64_t scratch_cap = 0;         // entries
  sdk::Res *d_res = nullptr, *h_res = nullptr;
  void *buf[2][kSlots] = {};  // [0] device, [1] pinned host staging for the callers
  int64_t buf_cap[2][kSlots] = {};
};

static void sd_release(tsim_shotdata *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  if (h->d_res) (void)hipFree(h->d_res);
  if (h->h_res) (void)hipHostFree(h->h_res);
  for (int k = 0; k < kSlots; ++k) {
    if (h->buf[0][k]) (void)hipFree(h->buf[0][k]);
    if (h->buf[1][k]) (void)hipHostFree(h->buf[1][k]);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

extern "C" int tsim_shotdata_create(int32_t device, tsim_shotdata **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  int count = 0;
  HIP_TRY(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) return tsim_fail(TSIM_EINVAL, "device %d of %d", device, count);
  tsim_shotdata *h = new (std::nothrow) tsim_shotdata();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->d_res), sizeof(sdk::Res));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&h->h_res), sizeof(sdk::Res), hipHostMallocDefault);
  if (e != hipSuccess) {
    sd_release(h);
    delete h;
    return tsim_fail(TSIM_EHIP, "tsim_shotdata_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_shotdata_destroy(tsim_shotdata *h) {
  if (!h) return;
  sd_release(h);
  delete h;
}

extern "C" int tsim_shotdata_staging(tsim_shotdata *h, int32_t slot, int32_t pinned, int64_t nbytes, void **ptr) {
  if (!h || !ptr) return tsim_fail(TSIM_EINVAL, "NULL handle or ptr");
  if (slot < 0 || slot >= kSlots || nbytes < 0) return tsim_fail(TSIM_EINVAL, "slot %d (0 .. %d), nbytes %lld", slot, kSlots - 1, (long long)nbytes);
  const int kind = pinned ? 1 : 0;
  HIP_TRY(hipSetDevice(h->device));
  if (h->buf_cap[kind][slot] < nbytes || !h->buf[kind][slot]) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->buf[kind][slot]) HIP_TRY(kind ? hipHostFree(h->buf[kind][slot]) : hipFree(h->buf[kind][slot]));
    h->buf[kind][slot] = nullptr;
    h->buf_cap[kind][slot] = 0;
    const int64_t cap = std::max<int64_t>(nbytes, 64) + 16;  // (dword atomics may touch up to 3 bytes past a row buffer)
    hipError_t e = kind ? hipHostMalloc(&h->buf[kind][slot], (size_t)cap, hipHostMallocDefault) : hipMalloc(&h->buf[kind][slot], (size_t)cap);
    if (e != hipSuccess) return tsim_fail(TSIM_ENOMEM, "staging of %lld bytes: %s", (long long)cap, hipGetErrorString(e));
    h->buf_cap[kind][slot] = cap;
  }
  *ptr = h->buf[kind][slot];
  return TSIM_OK;
}

extern "C" int tsim_shotdata_copy(tsim_shotdata *h, void *dst, const void *src, int64_t nbytes, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "NULL handle");
  if (nbytes < 0) return tsim_fail(TSIM_EINVAL, "negative size");
  if (nbytes == 0) return TSIM_OK;
  if (!dst || !src) return tsim_fail(TSIM_EINVAL, "NULL buffer");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDefault, stream ? (hipStream_t)stream : h->stream));
  return TSIM_OK;
}

extern "C" int tsim_shotdata_synchronize(tsim_shotdata *h, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(stream ? (hipStream_t)stream : h->stream));
  return TSIM_OK;
}

static int sd_scratch(tsim_shotdata *h, int64_t entries) {
  if (entries <= h->scratch_cap) return TSIM_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipDeviceSynchronize());  // (callers' streams may still use the old scratch)
  if (h->d_scratch) HIP_TRY(hipFree(h->d_scratch));
  h->d_scratch = nullptr;
  h->scratch_cap = 0;
  const int64_t cap = std::max<int64_t>(entries, 4096);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->d_scratch), (size_t)cap * sizeof(long long));
  if (e != hipSuccess) return tsim_fail(TSIM_ENOMEM, "scan scratch of %lld entries: %s", (long long)cap, hipGetErrorString(e));
  h->scratch_cap = cap;
  return TSIM_OK;
}

static int sd_check_sections(int32_t fmt, int32_t n_bits, int32_t nm, int32_t nd, int32_t no) {
  if (fmt < 0 || fmt > 5) return tsim_fail(TSIM_EINVAL, "format %d (0 .. 5: 01, b8, r8, ptb64, hits, dets)", fmt);
  if (n_bits < 0 || n_bits > (1 << 30)) return tsim_fail(TSIM_EINVAL, "n_bits = %d (0 .. 2^30)", n_bits);
  if (fmt == sdk::FDETS && (nm < 0 || nd < 0 || no < 0 || (int64_t)nm + nd + no != n_bits))
    return tsim_fail(TSIM_EINVAL, "dets sections %d + %d + %d do not add up to %d columns", nm, nd, no, n_bits);
  return TSIM_OK;
}

static unsigned sd_blocks(int64_t items, int64_t per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

template <int F>
static void sd_launch_len(const sdk::EncArgs &a, unsigned nb, hipStream_t s) {
  hipLaunchKernelGGL(sdk::k_enc_len<F>, dim3(nb), dim3(sdk::kBlock), 0, s, a);
}
template <int F>
static void sd_launch_write(const sdk::EncArgs &a, unsigned nb, hipStream_t s) {
  hipLaunchKernelGGL(sdk::k_enc_write<F>, dim3(nb), dim3(sdk::kBlock), 0, s, a);
}

extern "C" int tsim_shotdata_encode(tsim_shotdata *h, int32_t format, const uint8_t *d_rows, int64_t n, int64_t row_bytes,
                                    int32_t n_bits, int32_t num_m, int32_t num_d, int32_t num_o, uint8_t *d_out, int64_t out_cap,
                                    int64_t *out_bytes, void *stream) {
  if (!h || !out_bytes) return tsim_fail(TSIM_EINVAL, "NULL handle or out_bytes");
  if (int r = sd_check_sections(format, n_bits, num_m, num_d, num_o)) return r;
  const int64_t used = ((int64_t)n_bits + 7) / 8;
  if (n < 0 || n >= kMaxItems) return tsim_fail(TSIM_EINVAL, "n = %lld rows (0 .. 2^31 - 1)", (long long)n);
  if (row_bytes < used) return tsim_fail(TSIM_EINVAL, "row_bytes = %lld for %lld bytes per row", (long long)row_bytes, (long long)used);
  if (format == sdk::FPTB64 && n % 64 != 0) return tsim_fail(TSIM_EINVAL, "ptb64 needs a multiple of 64 rows, got %lld", (long long)n);
  if (n > 0 && used > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  if (out_cap < 0) return tsim_fail(TSIM_EINVAL, "negative out_cap");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  sdk::EncArgs a{};
  a.rows = d_rows;
  a.n = n;
  a.rb = row_bytes;
  a.bits = n_bits;
  a.used = (int)used;
  a.w8 = row_bytes % 8 == 0 && reinterpret_cast<uintptr_t>(d_rows) % 8 == 0;
  a.nm = num_m;
  a.nd = num_d;
  a.out = d_out;
  int64_t total = 0;
  switch (format) {
    case sdk::F01: total = n * ((int64_t)n_bits + 1); break;
    case sdk::FB8: total = n * used; break;
    case sdk::FPTB64: total = n / 64 * 8 * (int64_t)n_bits; break;
    default: break;
  }
  if (format == sdk::FR8 || format == sdk::FHITS || format == sdk::FDETS) {
    if (n == 0) {
      *out_bytes = 0;
      return TSIM_OK;
    }
    const int64_t nb = (n + sdk::kBlock - 1) / sdk::kBlock;
    if (int r = sd_scratch(h, n + nb)) return r;
    a.off = h->d_scratch;
    a.sums = h->d_scratch + n;
    if (format == sdk::FR8) sd_launch_len<sdk::FR8>(a, (unsigned)nb, s);
    else if (format == sdk::FHITS) sd_launch_len<sdk::FHITS>(a, (unsigned)nb, s);
    else sd_launch_len<sdk::FDETS>(a, (unsigned)nb, s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sdk::k_scan_sums, dim3(1), dim3(sdk::kScanBlock), 0, s, a.sums, (long long)nb, &h->d_res->total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h->h_res->total, &h->d_res->total, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    total = h->h_res->total;
    *out_bytes = total;
    if (total > out_cap) return 1;
    if (!d_out) return tsim_fail(TSIM_EINVAL, "d_out is NULL");
    if (format == sdk::FR8) sd_launch_write<sdk::FR8>(a, (unsigned)nb, s);
    else if (format == sdk::FHITS) sd_launch_write<sdk::FHITS>(a, (unsigned)nb, s);
    else sd_launch_write<sdk::FDETS>(a, (unsigned)nb, s);
    HIP_TRY(hipGetLastError());
    return TSIM_OK;
  }
  *out_bytes = total;
  if (total > out_cap) return 1;
  if (total == 0) return TSIM_OK;
  if (!d_out) return tsim_fail(TSIM_EINVAL, "d_out is NULL");
  if (format == sdk::FPTB64 && reinterpret_cast<uintptr_t>(d_out) % 8 != 0) return tsim_fail(TSIM_EINVAL, "ptb64 output must be 8-byte aligned");
  // launches of at most kLaunchItems work-items: rows in pieces (a multiple of 64 rows, so ptb64 groups stay whole)
  const int64_t nch = ((int64_t)n_bits + 1 + 7) / 8, nw = ((int64_t)n_bits + 63) / 64;
  const int64_t per_row = format == sdk::F01 ? nch : (format == sdk::FB8 ? std::max<int64_t>(used, 1) : std::max<int64_t>(nw, 1));
  const int64_t piece = std::max<int64_t>(64, kLaunchItems / per_row / 64 * 64);
  const unsigned tail = (n_bits & 7) ? ((1u << (n_bits & 7)) - 1u) : 255u;
  for (int64_t r0 = 0; r0 < n; r0 += piece) {
    const int64_t m = std::min(piece, n - r0);
    sdk::EncArgs p = a;
    p.rows = d_rows + r0 * row_bytes;
    p.n = m;
    if (format == sdk::F01) {
      p.out = d_out + r0 * ((int64_t)n_bits + 1);
      hipLaunchKernelGGL(sdk::k_enc_01, dim3(sd_blocks(m * nch, sdk::kBlock)), dim3(sdk::kBlock), 0, s, p);
    } else if (format == sdk::FB8) {
      uint8_t *out = d_out + r0 * used;
      if (a.w8) {  // padded uint64 rows: the library's compaction
        if (int r = tsim_launch_compact(reinterpret_cast<const uint64_t *>(p.rows), m, (int32_t)(row_bytes / 8), n_bits, out, s)) return r;
      } else {
        hipLaunchKernelGGL(sdk::k_copy_rows, dim3(sd_blocks(m * used, sdk::kBlock)), dim3(sdk::kBlock), 0, s, p.rows, (long long)row_bytes,
                           out, (long long)used, (long long)m, (int)used, tail);
      }
    } else {  // ptb64
      p.out = d_out + r0 / 64 * 8 * (int64_t)n_bits;
      hipLaunchKernelGGL(sdk::k_enc_ptb64, dim3(sd_blocks(m / 64 * nw, sdk::kBlock / 64)), dim3(sdk::kBlock), 0, s, p);
    }
    HIP_TRY(hipGetLastError());
  }
  return TSIM_OK;
}

template <int F>
static int sd_decode_scan(tsim_shotdata *h, const sdk::DecArgs &a, hipStream_t s) {
  const int64_t nb = (a.n_in + sdk::kBlock - 1) / sdk::kBlock;
  hipLaunchKernelGGL(sdk::k_sum_bytes<F>, dim3((unsigned)nb), dim3(sdk::kBlock), 0, s, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(sdk::k_scan_sums, dim3(1), dim3(sdk::kScanBlock), 0, s, a.sums, (long long)nb, &h->d_res->total);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(sdk::k_dec_rows<F == sdk::FR8 ? sdk::FR8 : sdk::FHITS>, dim3(1), dim3(1), 0, s, a);
  HIP_TRY(hipGetLastError());
  if (F == sdk::FR8) hipLaunchKernelGGL(sdk::k_dec_r8, dim3((unsigned)nb), dim3(sdk::kBlock), 0, s, a);
  else hipLaunchKernelGGL(sdk::k_dec_text<F>, dim3((unsigned)nb), dim3(sdk::kBlock), 0, s, a);
  HIP_TRY(hipGetLastError());
  return TSIM_OK;
}

extern "C" int tsim_shotdata_decode(tsim_shotdata *h, int32_t format, const uint8_t *d_in, int64_t n_in, int32_t is_final,
                                    int32_t n_bits, int32_t num_m, int32_t num_d, int32_t num_o, uint8_t *d_rows, int64_t row_bytes,
                                    int64_t max_rows, int64_t result[4], void *stream) {
  if (!h || !result) return tsim_fail(TSIM_EINVAL, "NULL handle or result");
  if (int r = sd_check_sections(format, n_bits, num_m, num_d, num_o)) return r;
  const int64_t used = ((int64_t)n_bits + 7) / 8;
  if ((format == sdk::FB8 || format == sdk::FPTB64) && n_bits < 1) return tsim_fail(TSIM_EINVAL, "b8 and ptb64 need n_bits >= 1 to be read");
  if (n_in < 0 || n_in >= kMaxItems) return tsim_fail(TSIM_EINVAL, "n_in = %lld (0 .. 2^31 - 1)", (long long)n_in);
  if (row_bytes < used) return tsim_fail(TSIM_EINVAL, "row_bytes = %lld for %lld bytes per row", (long long)row_bytes, (long long)used);
  if (max_rows < 0) return tsim_fail(TSIM_EINVAL, "negative max_rows");
  if (format == sdk::FPTB64 && max_rows % 64 != 0) return tsim_fail(TSIM_EINVAL, "ptb64 needs max_rows a multiple of 64");
  if (n_in > 0 && !d_in) return tsim_fail(TSIM_EINVAL, "d_in is NULL");
  if (max_rows > 0 && used > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  sdk::Res init{0, 0, 0, ~0ull};
  sdk::DecArgs a{};
  a.in = d_in;
  a.n_in = n_in;
  a.final_chunk = is_final ? 1 : 0;
  a.bits = n_bits;
  a.used = (int)used;
  a.nm = num_m;
  a.nd = num_d;
  a.rows = d_rows;
  a.rb = row_bytes;
  a.max_rows = max_rows;
  a.res = h->d_res;
  if (format == sdk::F01 || format == sdk::FB8 || format == sdk::FPTB64) {
    const int64_t unit = format == sdk::F01 ? (int64_t)n_bits + 1 : (format == sdk::FB8 ? used : 8 * (int64_t)n_bits);
    const int64_t per = format == sdk::FPTB64 ? 64 : 1;  // rows per unit
    int64_t units = std::min(n_in / unit, max_rows / per);
    int64_t rem = n_in - units * unit;
    int64_t rows = units * per, consumed = units * unit, last_len = unit;
    bool partial = false;
    if (is_final && rem > 0 && units == n_in / unit) {  // the file ends inside a row (or group)
      if (format == sdk::F01 && units < max_rows) {
        partial = true;  // decoded (and checked) as a row of rem bytes: rem == n is a last line without its '\n'
        last_len = rem;
        if (rem >= n_bits) {
          rows += 1;
          consumed = n_in;
        }
      } else if (format != sdk::F01) {
        init.fault = ((unsigned long long)n_in << 8) | sdk::kTruncated;
      }
    }
    init.rows = rows;
    init.consumed = consumed;
    HIP_TRY(hipMemcpyAsync(h->d_res, &init, sizeof(init), hipMemcpyHostToDevice, s));
    a.n_rows = units + (partial ? 1 : 0);
    a.last_len = last_len;
    if (format == sdk::F01 && a.n_rows > 0) {
      const int64_t nch = n_bits > 0 ? (n_bits + 7) / 8 : 1;
      hipLaunchKernelGGL(sdk::k_dec_01, dim3(sd_blocks(a.n_rows * nch, sdk::kBlock)), dim3(sdk::kBlock), 0, s, a);
    } else if (format == sdk::FB8 && units > 0) {
      const unsigned tail = (n_bits & 7) ? ((1u << (n_bits & 7)) - 1u) : 255u;
      hipLaunchKernelGGL(sdk::k_copy_rows, dim3(sd_blocks(units * used, sdk::kBlock)), dim3(sdk::kBlock), 0, s, d_in, (long long)used,
                         d_rows, (long long)row_bytes, (long long)units, (int)used, tail);
    } else if (format == sdk::FPTB64 && units > 0) {
      a.n_rows = units;
      const int64_t waves = units * (((int64_t)n_bits + 63) / 64);
      hipLaunchKernelGGL(sdk::k_dec_ptb64, dim3(sd_blocks(waves, sdk::kBlock / 64)), dim3(sdk::kBlock), 0, s, a);
    }
    HIP_TRY(hipGetLastError());
  } else {
    if (n_in == 0) {
      result[0] = result[1] = 0;
      result[2] = -1;
      result[3] = 0;
      return TSIM_OK;
    }
    const int64_t nb = (n_in + sdk::kBlock - 1) / sdk::kBlock;
    if (int r = sd_scratch(h, nb)) return r;
    a.sums = h->d_scratch;
    HIP_TRY(hipMemcpyAsync(h->d_res, &init, sizeof(init), hipMemcpyHostToDevice, s));
    if (max_rows > 0 && row_bytes > 0) HIP_TRY(hipMemsetAsync(d_rows, 0, (size_t)(max_rows * row_bytes), s));
    int r = format == sdk::FR8 ? sd_decode_scan<sdk::FR8>(h, a, s)
                               : (format == sdk::FHITS ? sd_decode_scan<sdk::FHITS>(h, a, s) : sd_decode_scan<sdk::FDETS>(h, a, s));
    if (r) return r;
  }
  HIP_TRY(hipMemcpyAsync(h->h_res, h->d_res, sizeof(sdk::Res), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const sdk::Res &res = *h->h_res;
  result[0] = res.rows;
  result[1] = res.consumed;
  result[2] = res.fault == ~0ull ? -1 : (int64_t)(res.fault >> 8);
  result[3] = res.fault == ~0ull ? 0 : (int64_t)(res.fault & 255);
  return TSIM_OK;
}
