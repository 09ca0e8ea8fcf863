// tsim_rowtab.hip - the distinct patterns of bit-packed device rows with exact counts, and a lookup decoder over such a
// table (tsim_rowtab_*): a handle of its own, bound to one device, holding the key columns, the slots and the counters;
// the kernels are csrc/tsim_rowtab.hip.h.
#include "tsim_host.hip.h"
#include "tsim_rowtab.hip.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace {
constexpr int64_t kMaxCapacity = 1ll << 30;
constexpr int kMaxProbe = 1024;                // slots looked at before a row counts as overflow
constexpr int64_t kRowsPerLaunch = 1ll << 30;  // a block's uint32 partials cannot overflow
constexpr int kBlocksPerCU = 4;                // resident k_claim blocks per CU (LDS: 4 KiB cache + 4 x 8.3 KiB staging)
}  // namespace

struct tsim_rowtab {
  int device = -1;
  int32_t n_cols = 0, n_key = 0, W = 0;
  bool direct = false, exact = false, loaded = false;
  int64_t capacity = 0, rows_added = 0, launches = 0, bytes = 0;
  int grid = 1;
  int32_t *d_kcol = nullptr;
  unsigned long long *d_tags = nullptr, *d_counts = nullptr, *d_keys = nullptr, *d_values = nullptr, *d_stats = nullptr;
};

static void rowtab_release(tsim_rowtab *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  for (void *p : {(void *)h->d_kcol, (void *)h->d_tags, (void *)h->d_counts, (void *)h->d_keys, (void *)h->d_values, (void *)h->d_stats})
    if (p) (void)hipFree(p);
}

extern "C" int tsim_rowtab_create(int32_t device, int32_t n_cols, const int32_t *key_cols, int32_t n_key, int64_t capacity,
                                  tsim_rowtab **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_cols < 1 || n_cols > (1 << 30)) return tsim_fail(TSIM_EINVAL, "n_cols = %d (1 .. 2^30)", n_cols);
  if (n_key < 1 || n_key > n_cols) return tsim_fail(TSIM_EINVAL, "n_key = %d (1 .. %d)", n_key, n_cols);
  if (!key_cols) return tsim_fail(TSIM_EINVAL, "key_cols is NULL");
  if (capacity < 1 || capacity > kMaxCapacity) return tsim_fail(TSIM_EINVAL, "capacity = %lld (1 .. 2^30)", (long long)capacity);
  bool direct = true;
  for (int i = 0; i < n_key; ++i) {
    if (key_cols[i] < 0 || key_cols[i] >= n_cols)
      return tsim_fail(TSIM_EINVAL, "key_cols[%d] = %d is not a column (0 .. %d)", i, key_cols[i], n_cols - 1);
    direct = direct && key_cols[i] == i;
  }
  std::vector<int32_t> sorted(key_cols, key_cols + n_key);
  std::sort(sorted.begin(), sorted.end());
  for (int i = 1; i < n_key; ++i)
    if (sorted[i] == sorted[i - 1]) return tsim_fail(TSIM_EINVAL, "key column %d is listed twice", sorted[i]);
  int cus = 0;
  if (const int rc = tsimh::open_device(device, &cus)) return rc;
  tsim_rowtab *h = new (std::nothrow) tsim_rowtab();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->n_cols = n_cols;
  h->n_key = n_key;
  h->W = (n_key + 63) / 64;
  h->direct = direct;
  h->exact = n_key <= 63;
  h->capacity = 1;
  while (h->capacity < capacity) h->capacity *= 2;
  h->grid = std::max(1, cus) * kBlocksPerCU;
  const size_t cap = (size_t)h->capacity, key_bytes = h->exact ? 0 : cap * h->W * 8;
  h->bytes = (int64_t)(cap * 16 + key_bytes + 4 * (size_t)n_key + 32);
  hipError_t e = hipMalloc(&h->d_kcol, sizeof(int32_t) * (size_t)n_key);
  if (e == hipSuccess) e = hipMalloc(&h->d_tags, cap * 8);
  if (e == hipSuccess) e = hipMalloc(&h->d_counts, cap * 8);
  if (e == hipSuccess && key_bytes) e = hipMalloc(&h->d_keys, key_bytes);
  if (e == hipSuccess) e = hipMalloc(&h->d_stats, 32);
  if (e == hipSuccess) e = hipMemcpy(h->d_kcol, key_cols, sizeof(int32_t) * (size_t)n_key, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_tags, 0, cap * 8);
  if (e == hipSuccess) e = hipMemset(h->d_counts, 0, cap * 8);
  if (e == hipSuccess) e = hipMemset(h->d_stats, 0, 32);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    rowtab_release(h);
    delete h;
    return tsim_fail(e == hipErrorOutOfMemory ? TSIM_ENOMEM : TSIM_EHIP, "row table of %lld slots, %d key columns: %s",
                     (long long)cap, n_key, hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_rowtab_destroy(tsim_rowtab *h) {
  if (!h) return;
  rowtab_release(h);
  delete h;
}

// the arguments every kernel shares; returns 0 or an error code (nothing launched)
static int rowtab_args(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor, const uint8_t *d_test,
                       rowtabk::Args *a) {
  if (!h) return tsim_fail(TSIM_EINVAL, "row table is NULL");
  if (n < 0) return tsim_fail(TSIM_EINVAL, "negative n");
  const int64_t used = tsimh::row_used(h->n_cols, row_bytes);
  if (used < 0) return (int)used;
  if (n > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  a->rb = row_bytes;
  a->n_cols = h->n_cols;
  a->used = (int)used;
  a->xr = d_xor;
  a->test = d_test;
  a->n_key = h->n_key;
  a->W = h->W;
  a->direct = h->direct;
  a->kcol = h->d_kcol;
  a->exact = h->exact;
  tsimh::choose_staging(*a, d_rows, row_bytes);
  a->tags = h->d_tags;
  a->counts = h->d_counts;
  a->keys = h->d_keys;
  a->values = h->d_values;
  a->cap_mask = h->capacity - 1;
  a->probe = (int)std::min<int64_t>(h->capacity, kMaxProbe);
  a->stats = h->d_stats;
  return TSIM_OK;
}

static unsigned rowtab_blocks(const tsim_rowtab *h, int64_t n) {
  const int64_t tiles = (n + 63) / 64;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + rowtabk::kWaves - 1) / rowtabk::kWaves, h->grid));
}

extern "C" int tsim_rowtab_add_device(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                      const uint8_t *d_test, void *stream) {
  rowtabk::Args a{};
  if (int rc = rowtab_args(h, d_rows, n, row_bytes, d_xor, d_test, &a)) return rc;
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t stage = (size_t)rowtabk::kWaves * a.stage_bytes;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * row_bytes;
    const unsigned blocks = rowtab_blocks(h, a.n);
    hipLaunchKernelGGL(rowtabk::k_claim, dim3(blocks), dim3(64 * rowtabk::kWaves), rowtabk::kCache * 16 + 16 + stage, s, a);
    HIP_TRY(hipGetLastError());
    ++h->launches;
    if (!h->exact) {  // (the next launch of the stream: every key k_claim stored is visible)
      hipLaunchKernelGGL(rowtabk::k_verify, dim3(blocks), dim3(64 * rowtabk::kWaves), 16 + stage, s, a);
      HIP_TRY(hipGetLastError());
      ++h->launches;
    }
  }
  h->rows_added += n;
  return TSIM_OK;
}

static int rowtab_stats(tsim_rowtab *h, uint64_t st[4], hipStream_t s) {
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(st, h->d_stats, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return TSIM_OK;
}

extern "C" int tsim_rowtab_read(tsim_rowtab *h, uint8_t *keys_out, uint64_t *counts_out, int64_t max_entries, int64_t *n_entries,
                                void *stream) {
  if (!h || !n_entries) return tsim_fail(TSIM_EINVAL, "NULL argument");
  *n_entries = 0;
  if (max_entries < 0 || (max_entries > 0 && (!keys_out || !counts_out))) return tsim_fail(TSIM_EINVAL, "no room for %lld entries", (long long)max_entries);
  hipStream_t s = (hipStream_t)stream;
  uint64_t st[4];
  if (int rc = rowtab_stats(h, st, s)) return rc;
  if (st[3])
    return tsim_fail(TSIM_ESTATE, "%llu rows met a slot that holds another key with their fingerprint: the counts are not valid",
                     (unsigned long long)st[3]);
  const size_t cap = (size_t)h->capacity, W = (size_t)h->W, kb = ((size_t)h->n_key + 7) / 8;
  std::vector<uint64_t> tags(cap), counts(cap), keys(h->exact ? 0 : cap * W);
  HIP_TRY(hipMemcpyAsync(tags.data(), h->d_tags, cap * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(counts.data(), h->d_counts, cap * 8, hipMemcpyDeviceToHost, s));
  if (!h->exact) HIP_TRY(hipMemcpyAsync(keys.data(), h->d_keys, cap * W * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int64_t found = 0;
  for (size_t i = 0; i < cap; ++i) {
    if (!tags[i]) continue;
    if (found < max_entries) {
      const uint64_t key1 = tags[i] & ~rowtabk::kUsed;
      std::memcpy(keys_out + (size_t)found * kb, h->exact ? &key1 : &keys[i * W], kb);  // (little-endian host)
      counts_out[found] = counts[i];
    }
    ++found;
  }
  *n_entries = found;
  if (found > max_entries) return tsim_fail(TSIM_EINVAL, "%lld entries, room for %lld", (long long)found, (long long)max_entries);
  return TSIM_OK;
}

extern "C" int tsim_rowtab_reset(tsim_rowtab *h, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "row table is NULL");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(h->d_tags, 0, (size_t)h->capacity * 8, s));
  HIP_TRY(hipMemsetAsync(h->d_counts, 0, (size_t)h->capacity * 8, s));
  HIP_TRY(hipMemsetAsync(h->d_stats, 0, 32, s));
  h->rows_added = 0;
  h->loaded = false;
  return TSIM_OK;
}

extern "C" int tsim_rowtab_info(tsim_rowtab *h, int64_t out[8]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());  // (the counters live on the device: every add so far is waited for)
  uint64_t st[4];
  if (int rc = rowtab_stats(h, st, nullptr)) return rc;
  out[0] = h->capacity;
  out[1] = (int64_t)st[1];
  out[2] = h->rows_added;
  out[3] = (int64_t)st[0];
  out[4] = (int64_t)st[2];
  out[5] = (int64_t)st[3];
  out[6] = h->launches;
  out[7] = h->bytes;
  return TSIM_OK;
}

extern "C" int tsim_rowtab_load(tsim_rowtab *h, const uint8_t *keys, const uint64_t *values, int64_t n) {
  if (!h) return tsim_fail(TSIM_EINVAL, "row table is NULL");
  if (n < 0 || (n > 0 && (!keys || !values))) return tsim_fail(TSIM_EINVAL, "NULL keys or values");
  if (n > h->capacity) return tsim_fail(TSIM_EINVAL, "%lld entries for %lld slots", (long long)n, (long long)h->capacity);
  const size_t cap = (size_t)h->capacity, W = (size_t)h->W, kb = ((size_t)h->n_key + 7) / 8;
  const int probe = (int)std::min<int64_t>(h->capacity, kMaxProbe);
  std::vector<uint64_t> tags(cap, 0), vals(cap, 0), image(h->exact ? 0 : cap * W, 0), key(W);
  for (int64_t r = 0; r < n; ++r) {
    std::fill(key.begin(), key.end(), 0);
    std::memcpy(key.data(), keys + (size_t)r * kb, kb);
    if (h->n_key % 64) key[W - 1] &= ~0ull >> (64 - h->n_key % 64);  // pad bits never belong to a pattern
    uint64_t fp = 0;
    if (h->exact) fp = key[0];
    else
      for (size_t w = 0; w < W; ++w) fp += rowtabk::word_hash(key[w], (int)w);
    const uint64_t tag = fp | rowtabk::kUsed;
    size_t i = (size_t)(rowtabk::mix64(tag) & (uint64_t)(h->capacity - 1));
    int p = 0;
    for (; p < probe && tags[i]; ++p, i = (i + 1) & (cap - 1))
      if (tags[i] == tag)
        return tsim_fail(TSIM_EINVAL, "key %lld %s", (long long)r,
                         h->exact || std::equal(key.begin(), key.end(), image.begin() + i * W) ? "is listed twice"
                                                                                                   : "shares its fingerprint with another key");
    if (p == probe) return tsim_fail(TSIM_ENOTSUP, "no free slot for key %lld within %d probes: raise the capacity", (long long)r, probe);
    tags[i] = tag;
    vals[i] = values[r];
    if (!h->exact) std::copy(key.begin(), key.end(), image.begin() + i * W);
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!h->d_values) {
    hipError_t e = hipMalloc(&h->d_values, cap * 8);
    if (e != hipSuccess) return tsim_fail(e == hipErrorOutOfMemory ? TSIM_ENOMEM : TSIM_EHIP, "values of %lld slots: %s", (long long)cap, hipGetErrorString(e));
    h->bytes += (int64_t)cap * 8;
  }
  HIP_TRY(hipMemcpy(h->d_tags, tags.data(), cap * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_values, vals.data(), cap * 8, hipMemcpyHostToDevice));
  if (!h->exact) HIP_TRY(hipMemcpy(h->d_keys, image.data(), cap * W * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->d_counts, 0, cap * 8));
  uint64_t st[4] = {0, (uint64_t)n, 0, 0};
  HIP_TRY(hipMemcpy(h->d_stats, st, 32, hipMemcpyHostToDevice));
  h->rows_added = 0;
  h->loaded = true;
  return TSIM_OK;
}

extern "C" int tsim_rowtab_decode_device(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                         const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, void *stream) {
  rowtabk::Args a{};
  if (int rc = rowtab_args(h, d_rows, n, row_bytes, d_xor, d_test, &a)) return rc;
  if (obs_lo < 0 || obs_hi < obs_lo || obs_hi > h->n_cols || obs_hi - obs_lo > 64)
    return tsim_fail(TSIM_EINVAL, "observable columns %d .. %d of %d (at most 64)", obs_lo, obs_hi, h->n_cols);
  if (!d_counters || reinterpret_cast<uintptr_t>(d_counters) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_counters is NULL or not 8-byte aligned");
  if (!h->loaded) return tsim_fail(TSIM_ESTATE, "the table holds no values: tsim_rowtab_load comes first");
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(h->device));
  a.obs_lo = obs_lo;
  a.obs_hi = obs_hi;
  a.dec = reinterpret_cast<unsigned long long *>(d_counters);
  const size_t stage = (size_t)rowtabk::kWaves * a.stage_bytes;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * row_bytes;
    hipLaunchKernelGGL(rowtabk::k_decode, dim3(rowtab_blocks(h, a.n)), dim3(64 * rowtabk::kWaves), 16 + stage, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    ++h->launches;
  }
  return TSIM_OK;
}

extern "C" int tsim_rowtab_decode_pred_device(tsim_rowtab *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                              const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                              void *stream) {
  if (!d_pred) return tsim_rowtab_decode_device(h, d_rows, n, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters, stream);
  rowtabk::Args a{};
  if (int rc = rowtab_args(h, d_rows, n, row_bytes, d_xor, d_test, &a)) return rc;
  if (obs_lo < 0 || obs_hi < obs_lo || obs_hi > h->n_cols || obs_hi - obs_lo > 64)
    return tsim_fail(TSIM_EINVAL, "observable columns %d .. %d of %d (at most 64)", obs_lo, obs_hi, h->n_cols);
  if (!d_counters || reinterpret_cast<uintptr_t>(d_counters) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_counters is NULL or not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_pred) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_pred is not 8-byte aligned");
  if (!h->loaded) return tsim_fail(TSIM_ESTATE, "the table holds no values: tsim_rowtab_load comes first");
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(h->device));
  a.obs_lo = obs_lo;
  a.obs_hi = obs_hi;
  a.dec = reinterpret_cast<unsigned long long *>(d_counters);
  const size_t stage = (size_t)rowtabk::kWaves * a.stage_bytes;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * row_bytes;
    a.pred = reinterpret_cast<unsigned long long *>(d_pred) + r0;
    hipLaunchKernelGGL(rowtabk::k_decode_pred, dim3(rowtab_blocks(h, a.n)), dim3(64 * rowtabk::kWaves), 16 + stage, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    ++h->launches;
  }
  return TSIM_OK;
}
