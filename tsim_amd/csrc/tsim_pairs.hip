// tsim_pairs.hip - pair counts over bit-packed device rows (tsim_pairs_*): a handle of its own, bound to one device,
// holding the selected columns, the bit-plane workspace of one slab of rows and the uint64 counter matrix; the kernels
// are csrc/tsim_pairs.hip.h.
#include "tsim_host.hip.h"
#include "tsim_pairs.hip.h"

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

namespace {
constexpr int kMaxPairCols = 4096;
constexpr int64_t kWorkspaceBytes = 32ll << 20;                   // the planes of one slab
constexpr int64_t kMinSlab = 1ll << 16, kMaxSlab = 1ll << 20;     // rows per slab (uint32 partials: below 2^32)
constexpr int kTargetBlocks = 1024;                               // k_gemm blocks per slab aimed at: 4 resident per CU, one round
constexpr int kMinGroupsPerBlock = 4;                             // ... while a block keeps 4096 rows per flush
}  // namespace

struct tsim_pairs {
  int device = -1;
  int32_t n_cols = 0, k = 0, kpad = 0, n_ach = 0;
  int64_t slab = 0, ws_bytes = 0, launches = 0;
  int32_t *d_scol = nullptr, *d_sslot = nullptr, *d_ach = nullptr, *d_aoff = nullptr;
  unsigned long long *d_plane = nullptr, *d_counts = nullptr;
};

static void pairs_release(tsim_pairs *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  for (void *p : {(void *)h->d_scol, (void *)h->d_sslot, (void *)h->d_ach, (void *)h->d_aoff, (void *)h->d_plane, (void *)h->d_counts})
    if (p) (void)hipFree(p);
}

extern "C" int tsim_pairs_create(int32_t device, int32_t n_cols, const int32_t *pair_cols, int32_t n_pair, tsim_pairs **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_cols < 1 || n_cols > (1 << 30)) return tsim_fail(TSIM_EINVAL, "n_cols = %d (1 .. 2^30)", n_cols);
  if (n_pair < 1 || n_pair > kMaxPairCols) return tsim_fail(TSIM_EINVAL, "n_pair = %d (1 .. %d)", n_pair, kMaxPairCols);
  if (!pair_cols) return tsim_fail(TSIM_EINVAL, "pair_cols is NULL");
  for (int i = 0; i < n_pair; ++i)
    if (pair_cols[i] < 0 || pair_cols[i] >= n_cols)
      return tsim_fail(TSIM_EINVAL, "pair_cols[%d] = %d is not a column (0 .. %d)", i, pair_cols[i], n_cols - 1);
  // the columns in ascending order with their slots, and the chunks of a row that hold any
  std::vector<int32_t> order((size_t)n_pair), scol((size_t)n_pair), ach, aoff;
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return pair_cols[x] < pair_cols[y]; });
  for (int i = 0; i < n_pair; ++i) {
    scol[i] = pair_cols[order[i]];
    if (i > 0 && scol[i] == scol[i - 1])
      return tsim_fail(TSIM_EINVAL, "pair_cols[%d] = pair_cols[%d] = %d", std::min(order[i - 1], order[i]), std::max(order[i - 1], order[i]), scol[i]);
    const int32_t ch = scol[i] / (8 * pairsk::kChunk);
    if (ach.empty() || ach.back() != ch) {
      ach.push_back(ch);
      aoff.push_back(i);
    }
  }
  aoff.push_back(n_pair);
  if (const int rc = tsimh::open_device(device, nullptr)) return rc;
  tsim_pairs *h = new (std::nothrow) tsim_pairs();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->n_cols = n_cols;
  h->k = n_pair;
  h->kpad = (n_pair + pairsk::kTile - 1) / pairsk::kTile * pairsk::kTile;
  h->n_ach = (int32_t)ach.size();
  h->slab = kMaxSlab;
  while (h->slab > kMinSlab && h->slab / 8 * h->kpad > kWorkspaceBytes) h->slab /= 2;
  h->ws_bytes = h->slab / 8 * h->kpad;
  const size_t cb = sizeof(uint64_t) * (size_t)n_pair * n_pair;
  hipError_t e = hipMalloc(&h->d_scol, sizeof(int32_t) * (size_t)n_pair);
  if (e == hipSuccess) e = hipMalloc(&h->d_sslot, sizeof(int32_t) * (size_t)n_pair);
  if (e == hipSuccess) e = hipMalloc(&h->d_ach, sizeof(int32_t) * ach.size());
  if (e == hipSuccess) e = hipMalloc(&h->d_aoff, sizeof(int32_t) * aoff.size());
  if (e == hipSuccess) e = hipMalloc(&h->d_plane, (size_t)h->ws_bytes);
  if (e == hipSuccess) e = hipMalloc(&h->d_counts, cb);
  if (e == hipSuccess) e = hipMemcpy(h->d_scol, scol.data(), sizeof(int32_t) * (size_t)n_pair, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_sslot, order.data(), sizeof(int32_t) * (size_t)n_pair, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_ach, ach.data(), sizeof(int32_t) * ach.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_aoff, aoff.data(), sizeof(int32_t) * aoff.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_plane, 0, (size_t)h->ws_bytes);  // (the slots past k are read, never counted)
  if (e == hipSuccess) e = hipMemset(h->d_counts, 0, cb);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    pairs_release(h);
    delete h;
    return tsim_fail(e == hipErrorOutOfMemory ? TSIM_ENOMEM : TSIM_EHIP, "pair counter of %d columns: %s", n_pair, hipGetErrorString(e));
  }
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_pairs_destroy(tsim_pairs *h) {
  if (!h) return;
  pairs_release(h);
  delete h;
}

extern "C" int tsim_pairs_add_device(tsim_pairs *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                     const uint8_t *d_test, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "pair counter is NULL");
  if (n < 0) return tsim_fail(TSIM_EINVAL, "negative n");
  const int64_t used = tsimh::row_used(h->n_cols, row_bytes);
  if (used < 0) return (int)used;
  if (n > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(h->device));

  pairsk::PlaneArgs p{};
  p.rb = row_bytes;
  p.n_cols = h->n_cols;
  p.used = (int)used;
  p.xr = d_xor;
  p.test = d_test;
  p.k = h->k;
  p.kpad = h->kpad;
  p.scol = h->d_scol;
  p.sslot = h->d_sslot;
  p.ach = h->d_ach;
  p.aoff = h->d_aoff;
  p.n_ach = h->n_ach;
  p.w4 = reinterpret_cast<uintptr_t>(d_rows) % 4 == 0 && row_bytes % 4 == 0;
  p.plane = h->d_plane;
  pairsk::GemmArgs g{};
  g.plane = reinterpret_cast<const uint32_t *>(h->d_plane);
  g.kpad = h->kpad;
  g.k = h->k;
  g.counts = h->d_counts;
  const int nt = h->kpad / pairsk::kTile, n_tiles = nt * (nt + 1) / 2;
  constexpr int64_t kGroupRows = 64 * pairsk::kGroup;
  hipStream_t s = (hipStream_t)stream;
  for (int64_t r0 = 0; r0 < n; r0 += h->slab) {  // (the launches of a stream run in order: the workspace is reused)
    p.n = std::min(h->slab, n - r0);
    p.rows = d_rows + r0 * row_bytes;
    const int64_t groups = (p.n + kGroupRows - 1) / kGroupRows;
    hipLaunchKernelGGL(pairsk::k_planes, dim3((unsigned)(groups * pairsk::kGroup / pairsk::kWaves)), dim3(64 * pairsk::kWaves), 0, s, p);
    HIP_TRY(hipGetLastError());
    g.groups = (int)groups;
    const int64_t split = std::max<int64_t>(1, std::min<int64_t>(kTargetBlocks / n_tiles,
                                                                 (groups + kMinGroupsPerBlock - 1) / kMinGroupsPerBlock));
    hipLaunchKernelGGL(pairsk::k_gemm, dim3((unsigned)n_tiles, (unsigned)split), dim3(256), 0, s, g);
    HIP_TRY(hipGetLastError());
    h->launches += 2;
  }
  return TSIM_OK;
}

extern "C" int tsim_pairs_read(tsim_pairs *h, uint64_t *out, void *stream) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  const size_t k = (size_t)h->k;
  HIP_TRY(hipMemcpyAsync(out, h->d_counts, sizeof(uint64_t) * k * k, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  // the kernel fills [a][b] for tile(a) <= tile(b) only: the rest is the mirror image
  for (size_t a = pairsk::kTile; a < k; ++a) {
    const size_t lim = a / pairsk::kTile * pairsk::kTile;
    for (size_t b = 0; b < lim; ++b) out[a * k + b] = out[b * k + a];
  }
  return TSIM_OK;
}

extern "C" int tsim_pairs_reset(tsim_pairs *h, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "pair counter is NULL");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemsetAsync(h->d_counts, 0, sizeof(uint64_t) * (size_t)h->k * h->k, (hipStream_t)stream));
  return TSIM_OK;
}

extern "C" int tsim_pairs_info(const tsim_pairs *h, int64_t out[4]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  out[0] = h->k;
  out[1] = h->ws_bytes;
  out[2] = h->slab;
  out[3] = h->launches;
  return TSIM_OK;
}
