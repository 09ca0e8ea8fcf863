// tsim_uf.hip - the union-find decoder over bit-packed device rows (tsim_uf_*): a handle of its own, bound to one device,
// holding the decoding graph's tables; the kernel is csrc/tsim_uf.hip.h, the rule tsim_amd/decode.py.
#include "../../include/tsim_hip.h"
#include "tsim_uf.hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

int tsim_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define UF_TRY(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return tsim_fail(TSIM_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace {
constexpr int kMaxGraph = 65535;               // nodes, and edges: uint16 indices
constexpr int64_t kRowsPerLaunch = 1ll << 30;  // a block's uint32 partials cannot overflow
}  // namespace

struct tsim_uf {
  int device = -1;
  ufk::Args a{};  // the graph's part of the kernel's arguments
  int grid = 1;
  int64_t launches = 0, bytes = 0;
  uint32_t *d_edge_uv = nullptr, *d_adj_ptr = nullptr;
  unsigned long long *d_edge_obs = nullptr, *d_stats = nullptr;
  uint16_t *d_adj_edge = nullptr;
  uint8_t *d_cap = nullptr;
  int max_cap = 0;  // 0: unweighted
  int n_heralds = 0;
  int32_t *d_her = nullptr;   // node_det, col_herald, herald_ptr, herald_edges: one allocation (heralds only)
  uint8_t *d_masks = nullptr;  // dmask, hmask
};

static void uf_release(tsim_uf *h) {
  if (h->device >= 0) (void)hipSetDevice(h->device);
  for (void *p : {(void *)h->d_edge_uv, (void *)h->d_adj_ptr, (void *)h->d_edge_obs, (void *)h->d_stats, (void *)h->d_adj_edge, (void *)h->d_cap,
                  (void *)h->d_her, (void *)h->d_masks})
    if (p) (void)hipFree(p);
}

extern "C" int tsim_uf_create(int32_t device, const tsim_uf_desc *desc, tsim_uf **out) {
  return tsim_uf_create_weighted(device, desc, nullptr, out);
}

extern "C" int tsim_uf_create_weighted(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, tsim_uf **out) {
  return tsim_uf_create_heralds(device, desc, edge_cap, nullptr, out);
}

extern "C" int tsim_uf_create_heralds(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her,
                                      tsim_uf **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!desc) return tsim_fail(TSIM_EINVAL, "desc is NULL");
  const int N = desc->n_nodes, E = desc->n_edges;
  if (N < 2) return tsim_fail(TSIM_EINVAL, "n_nodes = %d (the boundary and at least one detector)", N);
  if (E < 0) return tsim_fail(TSIM_EINVAL, "n_edges = %d", E);
  if (N > kMaxGraph || E > kMaxGraph)
    return tsim_fail(TSIM_ENOTSUP, "%d nodes and %d edges (at most %d each: indices are uint16)", N, E, kMaxGraph);
  const long long n_det = her ? (long long)N - 1 + her->n_heralds : N - 1;  // detector columns of a row
  if (her && (her->n_heralds < 0 || her->n_det_cols != n_det))
    return tsim_fail(TSIM_EINVAL, "n_det_cols = %d for %d nodes and %d heralds (nodes - 1 + heralds expected)", her->n_det_cols, N, her->n_heralds);
  if (desc->n_cols < n_det || desc->n_cols > (1 << 30))
    return tsim_fail(TSIM_EINVAL, "n_cols = %d for %lld detectors (up to 2^30)", desc->n_cols, n_det);
  if (E > 0 && (!desc->edge_u || !desc->edge_v || !desc->edge_obs)) return tsim_fail(TSIM_EINVAL, "an edge array is NULL");
  for (int e = 0; e < E; ++e) {
    const int32_t u = desc->edge_u[e], v = desc->edge_v[e];
    if (u < 0 || v >= N) return tsim_fail(TSIM_EINVAL, "edge %d = (%d, %d) leaves the nodes 0 .. %d", e, u, v, N - 1);
    if (u >= v) return tsim_fail(TSIM_EINVAL, "edge %d = (%d, %d): u < v expected", e, u, v);
    if (e > 0 && (desc->edge_u[e - 1] > u || (desc->edge_u[e - 1] == u && desc->edge_v[e - 1] >= v)))
      return tsim_fail(TSIM_EINVAL, "edge %d = (%d, %d) does not come after edge %d: the pairs must be strictly ascending", e, u, v, e - 1);
  }
  int max_cap = 0;
  if (edge_cap)
    for (int e = 0; e < E; ++e) {
      if (edge_cap[e] < 1 || edge_cap[e] > ufk::kMaxCap)
        return tsim_fail(TSIM_EINVAL, "edge %d has cap %d (1 .. %d: a 4-bit counter that may overshoot by one)", e, edge_cap[e], ufk::kMaxCap);
      max_cap = std::max<int>(max_cap, edge_cap[e]);
    }
  // the heralds: every column a node or one herald, the lists inside the edges
  const int H = her ? her->n_heralds : 0, mask_bytes = (desc->n_cols + 7) / 8;
  int n_listed = 0;
  std::vector<int32_t> her_tab;  // node_det [N - 1], col_herald [n_det], herald_ptr [H + 1], herald_edges [n_listed]
  std::vector<uint8_t> masks;    // dmask, hmask: mask_bytes each
  if (her) {
    if (!her->node_det || !her->herald_ptr || (H > 0 && !her->herald_det)) return tsim_fail(TSIM_EINVAL, "a herald array is NULL");
    std::vector<int32_t> col_herald((size_t)n_det, -1);
    masks.assign(2 * (size_t)mask_bytes, 0);
    for (int v = 0; v < N - 1; ++v) {
      const int32_t c = her->node_det[v];
      if (c < 0 || c >= n_det) return tsim_fail(TSIM_EINVAL, "node_det[%d] = %d leaves the columns 0 .. %lld", v, c, n_det - 1);
      if (v > 0 && her->node_det[v - 1] >= c) return tsim_fail(TSIM_EINVAL, "node_det[%d] = %d: the columns of the nodes must be strictly ascending", v, c);
      masks[c >> 3] |= (uint8_t)(1u << (c & 7));
    }
    for (int i = 0; i < H; ++i) {
      const int32_t c = her->herald_det[i];
      if (c < 0 || c >= n_det) return tsim_fail(TSIM_EINVAL, "herald_det[%d] = %d leaves the columns 0 .. %lld", i, c, n_det - 1);
      if ((masks[c >> 3] | masks[(size_t)mask_bytes + (c >> 3)]) >> (c & 7) & 1)
        return tsim_fail(TSIM_EINVAL, "column %d is named twice (a column is a node or one herald)", c);
      masks[(size_t)mask_bytes + (c >> 3)] |= (uint8_t)(1u << (c & 7));
      col_herald[c] = i;
    }
    if (her->herald_ptr[0] != 0) return tsim_fail(TSIM_EINVAL, "herald_ptr[0] = %d", her->herald_ptr[0]);
    for (int i = 0; i < H; ++i)
      if (her->herald_ptr[i + 1] < her->herald_ptr[i])
        return tsim_fail(TSIM_EINVAL, "herald_ptr[%d] = %d after %d: it must not fall", i + 1, her->herald_ptr[i + 1], her->herald_ptr[i]);
    n_listed = her->herald_ptr[H];
    if (n_listed > 0 && !her->herald_edges) return tsim_fail(TSIM_EINVAL, "herald_edges is NULL");
    for (int k = 0; k < n_listed; ++k)
      if (her->herald_edges[k] < 0 || her->herald_edges[k] >= E)
        return tsim_fail(TSIM_EINVAL, "herald_edges[%d] = %d of %d edges", k, her->herald_edges[k], E);
    her_tab.insert(her_tab.end(), her->node_det, her->node_det + (N - 1));
    her_tab.insert(her_tab.end(), col_herald.begin(), col_herald.end());
    her_tab.insert(her_tab.end(), her->herald_ptr, her->herald_ptr + H + 1);
    if (n_listed) her_tab.insert(her_tab.end(), her->herald_edges, her->herald_edges + n_listed);
    her_tab.push_back(0);
  }
  ufk::Args a{};
  a.n_nodes = N;
  a.n_edges = E;
  a.n_cols = desc->n_cols;
  a.n_det_cols = (int)n_det;
  a.w32 = std::max(1, (E + 31) / 32);
  a.w_cnt = edge_cap ? std::max(1, (E + 7) / 8) : 0;
  const long long shot = ufk::layout(&a);
  if (16 + shot > ufk::kLdsBlock)
    return tsim_fail(TSIM_ENOTSUP, "one shot's state takes %lld bytes of LDS (%d nodes, %d edges), a block has %d", shot, N, E, ufk::kLdsBlock - 16);
  a.shot_bytes = (int)shot;
  int best = 0, per_cu = 1;  // the waves of a block: as many shots on a CU as its LDS holds, in the fewest blocks
  for (int w = 1; w <= ufk::kMaxWaves; ++w) {
    const long long block = 16 + w * shot;
    if (block > ufk::kLdsBlock) break;
    const int blocks = (int)std::min<long long>(ufk::kLdsCU / block, 32 / w);
    if (blocks * w >= best) best = blocks * w, a.waves = w, per_cu = blocks;
  }
  // the tables: edge ends in one word, the edges at every node
  std::vector<uint32_t> uv((size_t)std::max(1, E)), ptr((size_t)N + 1, 0);
  std::vector<uint16_t> adj((size_t)std::max(1, 2 * E));
  for (int e = 0; e < E; ++e) {
    uv[e] = (uint32_t)desc->edge_u[e] | (uint32_t)desc->edge_v[e] << 16;
    ++ptr[desc->edge_u[e] + 1];
    ++ptr[desc->edge_v[e] + 1];
  }
  for (int v = 0; v < N; ++v) ptr[v + 1] += ptr[v];
  std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
  for (int e = 0; e < E; ++e) {
    adj[at[desc->edge_u[e]]++] = (uint16_t)e;
    adj[at[desc->edge_v[e]]++] = (uint16_t)e;
  }
  int count = 0;
  UF_TRY(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) return tsim_fail(TSIM_EINVAL, "device %d of %d", device, count);
  UF_TRY(hipSetDevice(device));
  int cus = 0;
  UF_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  tsim_uf *h = new (std::nothrow) tsim_uf();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->grid = std::max(1, cus) * per_cu;
  const size_t ne = uv.size(), na = adj.size();
  h->max_cap = max_cap;
  h->n_heralds = H;
  h->bytes = (int64_t)(ne * 12 + ptr.size() * 4 + na * 2 + 16 + (edge_cap ? ne : 0) + her_tab.size() * 4 + masks.size());
  hipError_t e = hipMalloc(&h->d_edge_uv, ne * 4);
  if (e == hipSuccess && her) e = hipMalloc(&h->d_her, her_tab.size() * 4);
  if (e == hipSuccess && her) e = hipMalloc(&h->d_masks, masks.size() + 8);
  if (e == hipSuccess && her) e = hipMemcpy(h->d_her, her_tab.data(), her_tab.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && her) e = hipMemset(h->d_masks, 0, masks.size() + 8);
  if (e == hipSuccess && her && !masks.empty()) e = hipMemcpy(h->d_masks, masks.data(), masks.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&h->d_edge_obs, ne * 8);
  if (e == hipSuccess) e = hipMalloc(&h->d_adj_ptr, ptr.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&h->d_adj_edge, na * 2);
  if (e == hipSuccess) e = hipMalloc(&h->d_stats, 16);
  if (e == hipSuccess && edge_cap) e = hipMalloc(&h->d_cap, ne);
  if (e == hipSuccess && edge_cap) e = hipMemset(h->d_cap, 1, ne);
  if (e == hipSuccess && edge_cap && E) e = hipMemcpy(h->d_cap, edge_cap, (size_t)E, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_edge_uv, uv.data(), ne * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_edge_obs, 0, ne * 8);
  if (e == hipSuccess && E) e = hipMemcpy(h->d_edge_obs, desc->edge_obs, (size_t)E * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_adj_ptr, ptr.data(), ptr.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_adj_edge, adj.data(), na * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_stats, 0, 16);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    uf_release(h);
    delete h;
    return tsim_fail(e == hipErrorOutOfMemory ? TSIM_ENOMEM : TSIM_EHIP, "decoding graph of %d nodes, %d edges: %s", N, E, hipGetErrorString(e));
  }
  a.edge_uv = h->d_edge_uv;
  a.edge_obs = h->d_edge_obs;
  a.adj_ptr = h->d_adj_ptr;
  a.adj_edge = h->d_adj_edge;
  a.cap = h->d_cap;
  a.stats = h->d_stats;
  if (her) {
    a.node_det = h->d_her;
    a.col_herald = a.node_det + (N - 1);
    a.herald_ptr = a.col_herald + n_det;
    a.herald_edges = a.herald_ptr + H + 1;
    a.dmask = h->d_masks;
    a.hmask = h->d_masks + mask_bytes;
  }
  h->a = a;
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_uf_destroy(tsim_uf *h) {
  if (!h) return;
  uf_release(h);
  delete h;
}

extern "C" int tsim_uf_info(tsim_uf *h, int64_t out[16]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  UF_TRY(hipSetDevice(h->device));
  UF_TRY(hipDeviceSynchronize());  // (the statistics live on the device: every decode so far is waited for)
  uint64_t st[2];
  UF_TRY(hipMemcpy(st, h->d_stats, 16, hipMemcpyDeviceToHost));
  std::fill(out, out + 16, 0);
  out[0] = h->a.n_nodes;
  out[1] = h->a.n_edges;
  out[2] = h->a.shot_bytes;
  out[3] = h->a.waves;
  out[4] = h->launches;
  out[5] = (int64_t)st[0];
  out[6] = h->bytes;
  out[7] = (int64_t)st[1];
  out[8] = h->a.n_cols;
  out[9] = h->grid;
  out[10] = h->max_cap;
  out[11] = h->n_heralds;
  out[12] = h->a.n_det_cols;
  return TSIM_OK;
}

namespace {
struct SoftOut {  // what tsim_uf_decode_soft_device adds to tsim_uf_decode_device
  int metric, n_bins;
  uint64_t *d_hist;
  uint32_t *d_soft;
};

template <bool Soft>
void uf_launch(const ufk::Args &a, unsigned blocks, size_t lds, hipStream_t stream) {
  if (a.node_det) {
    if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, true, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
    else hipLaunchKernelGGL((ufk::k_uf<false, true, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  } else if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, false, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  else hipLaunchKernelGGL((ufk::k_uf<false, false, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
}
}  // namespace

// both decode entry points; soft == NULL: tsim_uf_decode_device
static int uf_decode(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor, const uint8_t *d_test,
                     int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred, const SoftOut *soft, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "decoder is NULL");
  if (n < 0) return tsim_fail(TSIM_EINVAL, "negative n");
  ufk::Args a = h->a;
  const int64_t used = ((int64_t)a.n_cols + 7) / 8;
  if (row_bytes < used || row_bytes > 0x7FFFFFFF)
    return tsim_fail(TSIM_EINVAL, "row_bytes = %lld for %lld bytes per row", (long long)row_bytes, (long long)used);
  if (n > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  if (obs_lo < 0 || obs_hi < obs_lo || obs_hi > a.n_cols || obs_hi - obs_lo > 64)
    return tsim_fail(TSIM_EINVAL, "observable columns %d .. %d of %d (at most 64)", obs_lo, obs_hi, a.n_cols);
  if (!d_counters || reinterpret_cast<uintptr_t>(d_counters) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_counters is NULL or not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_pred) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_pred is not 8-byte aligned");
  if (soft) {
    if (soft->metric < 0 || soft->metric > 3) return tsim_fail(TSIM_EINVAL, "metric = %d (0 rounds, 1 full_edges, 2 largest_cluster, 3 correction_weight)", soft->metric);
    if (soft->n_bins < 2 || soft->n_bins > 1024) return tsim_fail(TSIM_EINVAL, "n_bins = %d (2 .. 1024)", soft->n_bins);
    if (!soft->d_hist || reinterpret_cast<uintptr_t>(soft->d_hist) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_hist is NULL or not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(soft->d_soft) % 16 != 0) return tsim_fail(TSIM_EINVAL, "d_soft is not 16-byte aligned");
    a.metric = soft->metric;
    a.n_bins = soft->n_bins;
    a.hist = reinterpret_cast<unsigned long long *>(soft->d_hist);
  }
  if (n == 0) return TSIM_OK;
  UF_TRY(hipSetDevice(h->device));
  a.rb = row_bytes;
  a.used = (int)used;
  a.xr = d_xor;
  a.test = d_test;
  a.w8 = reinterpret_cast<uintptr_t>(d_rows) % 8 == 0 && row_bytes % 8 == 0;
  a.obs_lo = obs_lo;
  a.obs_hi = obs_hi;
  a.dec = reinterpret_cast<unsigned long long *>(d_counters);
  const size_t lds = 16 + (size_t)a.waves * a.shot_bytes;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * row_bytes;
    a.pred = d_pred ? reinterpret_cast<unsigned long long *>(d_pred) + r0 : nullptr;
    const int64_t tiles = (a.n + 63) / 64;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + a.waves - 1) / a.waves, h->grid));
    if (soft) {
      a.soft = soft->d_soft ? soft->d_soft + 4 * r0 : nullptr;
      uf_launch<true>(a, blocks, lds, (hipStream_t)stream);
    } else {
      uf_launch<false>(a, blocks, lds, (hipStream_t)stream);
    }
    UF_TRY(hipGetLastError());
    ++h->launches;
  }
  return TSIM_OK;
}

extern "C" int tsim_uf_decode_device(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                     const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                     void *stream) {
  return uf_decode(h, d_rows, n, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters, d_pred, nullptr, stream);
}

extern "C" int tsim_uf_decode_soft_device(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                          const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                          int32_t metric, int32_t n_bins, uint64_t *d_hist, uint32_t *d_soft, void *stream) {
  const SoftOut soft{metric, n_bins, d_hist, d_soft};
  return uf_decode(h, d_rows, n, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters, d_pred, &soft, stream);
}
