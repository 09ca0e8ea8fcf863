// tsim_uf.hip - the union-find decoder over bit-packed device rows (tsim_uf_*): a handle of its own, bound to one device,
// holding the decoding graph's tables; the kernel is csrc/tsim_uf.hip.h, the rule tsim_amd/decode.py.
#include "tsim_uf_host.hip.h"
#include "tsim_uf_match.hip.h"

#include <new>

struct tsim_uf {
  int device = -1;
  ufk::Args a{};  // the graph's part of the kernel's arguments
  int grid = 1;
  int64_t launches = 0;
  int max_cap = 0;  // 0: unweighted
  int n_heralds = 0;
  ufk::TableArgs table{};  // cluster matching: the match table (a.match_k != 0)
  ufk::GapTableArgs gtable{};  // the complementary gap: the class table (a.gap != 0) ...
  int64_t w0 = -1;             // ... and the lightest logical without a defect, -1: none
  tsimh::Uploads up;  // the tables a points to
};

hipError_t ufh::launch_match_table(int n_nodes, const uint32_t *edge_uv, const unsigned long long *edge_obs, const uint16_t *w,
                                   const uint32_t *adj_ptr, const uint16_t *adj_edge, uint32_t *dist, unsigned long long *mask, uint16_t *parent) {
  ufk::TableArgs t{};
  t.n_nodes = n_nodes, t.edge_uv = edge_uv, t.edge_obs = edge_obs, t.w = w, t.adj_ptr = adj_ptr, t.adj_edge = adj_edge;
  t.dist = dist, t.mask = mask, t.parent = parent;
  hipLaunchKernelGGL(ufk::k_match_table, dim3(n_nodes), dim3(ufk::kTableThreads), ufk::table_lds(n_nodes), nullptr, t);
  return hipGetLastError();
}

extern "C" int tsim_uf_create(int32_t device, const tsim_uf_desc *desc, tsim_uf **out) {
  return tsim_uf_create_weighted(device, desc, nullptr, out);
}

extern "C" int tsim_uf_create_weighted(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, tsim_uf **out) {
  return tsim_uf_create_heralds(device, desc, edge_cap, nullptr, out);
}

// every create call; match_w != NULL: tsim_uf_create_matching, with max_defects; gap_obs >= 0: tsim_uf_create_matching_gap;
// max_hubs != 0: tsim_uf_create_matching_heralds, with erased_w
static int uf_create(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her, const uint16_t *match_w,
                     int32_t max_defects, int32_t gap_obs, tsim_uf **out, int32_t erased_w = 0, int32_t max_hubs = 0);

extern "C" int tsim_uf_create_heralds(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her,
                                      tsim_uf **out) {
  return uf_create(device, desc, edge_cap, her, nullptr, 0, -1, out);
}

extern "C" int tsim_uf_create_matching(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const uint16_t *match_w,
                                       int32_t max_defects, tsim_uf **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!match_w) return tsim_fail(TSIM_EINVAL, "match_w is NULL");
  if (max_defects < 1 || max_defects > ufk::kMaxMatchDefects)
    return tsim_fail(TSIM_EINVAL, "max_defects = %d (1 .. %d)", max_defects, ufk::kMaxMatchDefects);
  return uf_create(device, desc, edge_cap, nullptr, match_w, max_defects, -1, out);
}

extern "C" int tsim_uf_create_matching_gap(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const uint16_t *match_w,
                                           int32_t max_defects, int32_t observable, tsim_uf **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!match_w) return tsim_fail(TSIM_EINVAL, "match_w is NULL");
  if (max_defects < 1 || max_defects > ufk::kMaxMatchDefects)
    return tsim_fail(TSIM_EINVAL, "max_defects = %d (1 .. %d)", max_defects, ufk::kMaxMatchDefects);
  if (observable < 0 || observable > 63) return tsim_fail(TSIM_EINVAL, "observable = %d (0 .. 63)", observable);
  return uf_create(device, desc, edge_cap, nullptr, match_w, max_defects, observable, out);
}

extern "C" int tsim_uf_create_matching_heralds(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her,
                                               const uint16_t *match_w, int32_t max_defects, int32_t erased_w, int32_t max_hubs,
                                               int32_t observable, tsim_uf **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!her) return tsim_fail(TSIM_EINVAL, "her is NULL (a graph without heralds: tsim_uf_create_matching)");
  if (!match_w) return tsim_fail(TSIM_EINVAL, "match_w is NULL");
  if (max_defects < 1 || max_defects > ufk::kMaxMatchDefects)
    return tsim_fail(TSIM_EINVAL, "max_defects = %d (1 .. %d)", max_defects, ufk::kMaxMatchDefects);
  if (erased_w < 1 || erased_w > 65535) return tsim_fail(TSIM_EINVAL, "erased_w = %d (1 .. 65535)", erased_w);
  if (max_hubs < max_defects || max_hubs > ufk::kMaxMatchHubs)
    return tsim_fail(TSIM_EINVAL, "max_hubs = %d (max_defects = %d .. %d)", max_hubs, max_defects, ufk::kMaxMatchHubs);
  if (observable < -1 || observable > 63) return tsim_fail(TSIM_EINVAL, "observable = %d (0 .. 63, or -1: no gap)", observable);
  return uf_create(device, desc, edge_cap, her, match_w, max_defects, observable, out, erased_w, max_hubs);
}

static int uf_create(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her, const uint16_t *match_w,
                     int32_t max_defects, int32_t gap_obs, tsim_uf **out, int32_t erased_w, int32_t max_hubs) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!desc) return tsim_fail(TSIM_EINVAL, "desc is NULL");
  const int N = desc->n_nodes, E = desc->n_edges;
  if (N < 2) return tsim_fail(TSIM_EINVAL, "n_nodes = %d (the boundary and at least one detector)", N);
  if (E < 0) return tsim_fail(TSIM_EINVAL, "n_edges = %d", E);
  if (N > ufh::kMaxIndex || E > ufh::kMaxIndex)
    return tsim_fail(TSIM_ENOTSUP, "%d nodes and %d edges (at most %d each: indices are uint16)", N, E, ufh::kMaxIndex);
  long long n_det = 0;
  int max_cap = 0;
  if (const int rc = ufh::check_graph(desc, edge_cap, her, &n_det, &max_cap)) return rc;
  if (match_w) {
    for (int e = 0; e < E; ++e)
      if (match_w[e] < 1) return tsim_fail(TSIM_EINVAL, "edge %d has match weight 0 (1 .. 65535)", e);
    if (N > ufk::kMaxMatchNodes)
      return tsim_fail(TSIM_ENOTSUP, "%d nodes (a match table has at most %d: 12 bytes per pair of nodes)", N, ufk::kMaxMatchNodes);
  }
  const int H = her ? her->n_heralds : 0, mask_bytes = (desc->n_cols + 7) / 8;
  std::vector<int32_t> her_tab;  // node_det [N - 1], col_herald [n_det], herald_ptr [H + 1], herald_edges [n_listed], a spare entry
  std::vector<uint8_t> masks;    // dmask, hmask: mask_bytes each, and 8 bytes of zeros
  if (her) {
    std::vector<int32_t> col_herald((size_t)n_det, -1);
    masks.assign(2 * (size_t)mask_bytes + 8, 0);
    if (const int rc = ufh::check_heralds(desc, her, n_det, masks.data(), masks.data() + mask_bytes, col_herald.data())) return rc;
    her_tab.insert(her_tab.end(), her->node_det, her->node_det + (N - 1));
    her_tab.insert(her_tab.end(), col_herald.begin(), col_herald.end());
    her_tab.insert(her_tab.end(), her->herald_ptr, her->herald_ptr + H + 1);
    if (her->herald_ptr[H]) her_tab.insert(her_tab.end(), her->herald_edges, her->herald_edges + her->herald_ptr[H]);
    her_tab.push_back(0);
  }
  ufk::Args a{};
  a.n_nodes = N;
  a.n_edges = E;
  a.n_cols = desc->n_cols;
  a.n_det_cols = (int)n_det;
  a.w32 = std::max(1, (E + 31) / 32);
  a.w_cnt = edge_cap ? std::max(1, (E + 7) / 8) : 0;
  a.match_k = match_w ? max_defects : 0;
  a.gap = match_w && gap_obs >= 0;
  a.max_hubs = max_hubs;
  a.erased_w = (uint32_t)erased_w;
  a.gap_obs = std::max(0, gap_obs);
  const long long shot = ufk::layout(&a);
  if (16 + shot > ufk::kLdsBlock)
    return tsim_fail(TSIM_ENOTSUP, "one shot's state takes %lld bytes of LDS (%d nodes, %d edges%s), a block has %d", shot, N, E,
                     max_hubs ? ", the dynamic programs of max_defects and the hub graph of max_hubs"
                     : a.gap  ? ", the dynamic programs of max_defects: the winners and the classes"
                     : match_w ? ", the dynamic program of max_defects"
                              : "",
                     ufk::kLdsBlock - 16);
  a.shot_bytes = (int)shot;
  int per_cu = 1;
  ufh::choose_waves(shot, &a.waves, &per_cu);
  // the tables: edge ends in one word, the edges at every node (never an empty buffer)
  const size_t ne = (size_t)std::max(1, E);
  std::vector<uint32_t> uv(ne), ptr((size_t)N + 1, 0);
  std::vector<uint16_t> adj((size_t)std::max(1, 2 * E));
  std::vector<uint64_t> obs(ne, 0);
  std::vector<uint8_t> cap(edge_cap ? ne : 0, 1);
  for (int e = 0; e < E; ++e) {
    uv[e] = (uint32_t)desc->edge_u[e] | (uint32_t)desc->edge_v[e] << 16;
    obs[e] = desc->edge_obs[e];
    if (edge_cap) cap[e] = edge_cap[e];
    ++ptr[desc->edge_u[e] + 1];
    ++ptr[desc->edge_v[e] + 1];
  }
  for (int v = 0; v < N; ++v) ptr[v + 1] += ptr[v];
  std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
  for (int e = 0; e < E; ++e) {
    adj[at[desc->edge_u[e]]++] = (uint16_t)e;
    adj[at[desc->edge_v[e]]++] = (uint16_t)e;
  }
  int cus = 0;
  if (const int rc = tsimh::open_device(device, &cus)) return rc;
  tsim_uf *h = new (std::nothrow) tsim_uf();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->grid = std::max(1, cus) * per_cu;
  h->max_cap = max_cap;
  h->n_heralds = H;
  tsimh::Uploads &up = h->up;
  a.edge_uv = up.put(uv);
  a.edge_obs = reinterpret_cast<const unsigned long long *>(up.put(obs));
  a.adj_ptr = up.put(ptr);
  a.adj_edge = up.put(adj);
  if (edge_cap) a.cap = up.put(cap);
  const uint64_t zero[6] = {0, 0, 0, 0, 0, 0};
  a.stats = reinterpret_cast<unsigned long long *>(up.put(zero, max_hubs ? 6 : match_w ? 4 : 2));
  if (match_w) {  // the match table, built here once
    const std::vector<uint16_t> w(match_w, match_w + E);
    const size_t pairs = (size_t)N * (size_t)N;
    ufk::TableArgs &t = h->table;
    t.n_nodes = N, t.edge_uv = a.edge_uv, t.edge_obs = a.edge_obs, t.adj_ptr = a.adj_ptr, t.adj_edge = a.adj_edge;
    t.w = up.put(w);
    if (max_hubs) a.match_w = t.w;
    t.dist = static_cast<uint32_t *>(up.room(pairs * sizeof(uint32_t)));
    t.mask = static_cast<unsigned long long *>(up.room(pairs * sizeof(uint64_t)));
    up.bytes += (int64_t)(pairs * 12);
    if (up.err == hipSuccess) up.err = ufh::launch_match_table(N, t.edge_uv, t.edge_obs, t.w, t.adj_ptr, t.adj_edge, t.dist, t.mask, nullptr);
    a.mdist = t.dist, a.mmask = t.mask;
    if (a.gap) {  // the class table, after it
      ufk::GapTableArgs &g = h->gtable;
      g.n_nodes = N, g.observable = gap_obs, g.edge_uv = a.edge_uv, g.edge_obs = a.edge_obs, g.w = t.w, g.adj_ptr = a.adj_ptr, g.adj_edge = a.adj_edge;
      g.dist2 = static_cast<uint32_t *>(up.room(pairs * 2 * sizeof(uint32_t)));
      g.w0 = static_cast<uint32_t *>(up.room((size_t)N * sizeof(uint32_t)));
      up.bytes += (int64_t)(pairs * 8 + (size_t)N * 4);
      if (up.err == hipSuccess) {
        hipLaunchKernelGGL(ufk::k_gap_table, dim3(N), dim3(ufk::kTableThreads), ufk::gap_table_lds(N), nullptr, g);
        up.err = hipGetLastError();
      }
      a.gdist = g.dist2;
    }
  }
  if (her) {
    a.node_det = up.put(her_tab);
    a.col_herald = a.node_det + (N - 1);
    a.herald_ptr = a.col_herald + n_det;
    a.herald_edges = a.herald_ptr + H + 1;
    a.dmask = up.put(masks.data(), 2 * (size_t)mask_bytes, 8);
    a.hmask = a.dmask + mask_bytes;
  }
  if (up.err == hipSuccess) up.err = hipDeviceSynchronize();
  if (up.err == hipSuccess && a.gap) {  // W0: the least of the sources' sums
    std::vector<uint32_t> sums((size_t)N);
    up.err = hipMemcpy(sums.data(), h->gtable.w0, sums.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    const uint32_t least = *std::min_element(sums.begin(), sums.end());
    h->w0 = up.err == hipSuccess && least != ufk::kMatchInf ? (int64_t)least : -1;
  }
  if (up.err != hipSuccess) {
    const hipError_t e = up.err;
    tsim_uf_destroy(h);
    return tsim_fail(e == hipErrorOutOfMemory ? TSIM_ENOMEM : TSIM_EHIP, "decoding graph of %d nodes, %d edges: %s", N, E, hipGetErrorString(e));
  }
  h->a = a;
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_uf_destroy(tsim_uf *h) {
  if (!h) return;
  h->up.release(h->device);
  delete h;
}

extern "C" int tsim_uf_info(tsim_uf *h, int64_t out[16]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());  // (the statistics live on the device: every decode so far is waited for)
  uint64_t st[2];
  HIP_TRY(hipMemcpy(st, h->a.stats, 16, hipMemcpyDeviceToHost));
  std::fill(out, out + 16, 0);
  out[0] = h->a.n_nodes;
  out[1] = h->a.n_edges;
  out[2] = h->a.shot_bytes;
  out[3] = h->a.waves;
  out[4] = h->launches;
  out[5] = (int64_t)st[0];
  out[6] = h->up.bytes;
  out[7] = (int64_t)st[1];
  out[8] = h->a.n_cols;
  out[9] = h->grid;
  out[10] = h->max_cap;
  out[11] = h->n_heralds;
  out[12] = h->a.n_det_cols;
  if (h->a.match_k) {
    HIP_TRY(hipMemcpy(st, h->a.stats + 2, 16, hipMemcpyDeviceToHost));
    out[13] = h->a.match_k;
    out[14] = (int64_t)st[0];
    out[15] = (int64_t)st[1];
  }
  return TSIM_OK;
}

extern "C" int tsim_uf_erasure_info(tsim_uf *h, int64_t out[4]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!h->a.max_hubs) return tsim_fail(TSIM_EINVAL, "the handle matches no clusters under heralds (tsim_uf_create_matching_heralds makes one)");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  uint64_t st[2];
  HIP_TRY(hipMemcpy(st, h->a.stats + 4, 16, hipMemcpyDeviceToHost));
  out[0] = h->a.erased_w;
  out[1] = h->a.max_hubs;
  out[2] = (int64_t)st[0];
  out[3] = (int64_t)st[1];
  return TSIM_OK;
}

namespace {
struct SoftOut {  // what tsim_uf_decode_soft_device adds to tsim_uf_decode_device; gap_cap != 0: what tsim_uf_decode_gap_device adds
  int metric, n_bins;
  uint64_t *d_hist;
  uint32_t *d_soft;  // four values per row, or the gap call's deficit per row
  uint32_t gap_cap = 0, gap_step = 0;
};

void uf_launch_gap(const ufk::Args &a, unsigned blocks, size_t lds, hipStream_t stream) {
  if (a.max_hubs) {  // (a handle of tsim_uf_create_matching_heralds with an observable)
    if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, true, false, true, true, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
    else hipLaunchKernelGGL((ufk::k_uf<false, true, false, true, true, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
    return;
  }
  if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, false, false, true, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  else hipLaunchKernelGGL((ufk::k_uf<false, false, false, true, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
}

template <bool Soft>
void uf_launch(const ufk::Args &a, unsigned blocks, size_t lds, hipStream_t stream) {
  if constexpr (!Soft)
    if (a.max_hubs) {  // (a handle of tsim_uf_create_matching_heralds: its own kernel; the classes run in the gap call only)
      if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, true, false, true, false, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
      else hipLaunchKernelGGL((ufk::k_uf<false, true, false, true, false, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
      return;
    }
  if constexpr (!Soft)
    if (a.match_k) {  // (a handle of tsim_uf_create_matching: no heralds, no soft outputs)
      if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, false, false, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
      else hipLaunchKernelGGL((ufk::k_uf<false, false, false, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
      return;
    }
  if (a.node_det) {
    if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, true, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
    else hipLaunchKernelGGL((ufk::k_uf<false, true, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  } else if (a.cap) hipLaunchKernelGGL((ufk::k_uf<true, false, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  else hipLaunchKernelGGL((ufk::k_uf<false, false, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
}
}  // namespace

// the decode entry points; soft == NULL: tsim_uf_decode_device
static int uf_decode(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor, const uint8_t *d_test,
                     int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred, const SoftOut *soft, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "decoder is NULL");
  ufk::Args a = h->a;
  if (const int rc = ufh::check_rows(a, d_rows, n, row_bytes, obs_lo, obs_hi, d_counters, d_pred)) return rc;
  const bool gap = soft && soft->gap_cap;
  if (gap) {
    a.gap_cap = soft->gap_cap, a.gap_step = soft->gap_step;
    a.n_bins = soft->n_bins;
    a.hist = reinterpret_cast<unsigned long long *>(soft->d_hist);
  } else if (soft) {
    if (a.match_k) return tsim_fail(TSIM_EINVAL, "a cluster-matching handle has no soft outputs");
    if (const int rc = ufh::check_soft(a, soft->metric, soft->n_bins, soft->d_hist, soft->d_soft)) return rc;
  }
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(h->device));
  ufh::fill_rows(a, d_rows, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters);
  return ufh::launch_rows(a, d_rows, n, d_pred, h->grid, &h->launches, [&](ufk::Args &a, int64_t r0, unsigned blocks, size_t lds) {
    if (gap) {
      a.soft = soft->d_soft ? soft->d_soft + r0 : nullptr;
      uf_launch_gap(a, blocks, lds, (hipStream_t)stream);
    } else if (soft) {
      a.soft = soft->d_soft ? soft->d_soft + 4 * r0 : nullptr;
      uf_launch<true>(a, blocks, lds, (hipStream_t)stream);
    } else {
      uf_launch<false>(a, blocks, lds, (hipStream_t)stream);
    }
  });
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

extern "C" int tsim_uf_decode_gap_device(tsim_uf *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                         const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                         int64_t gap_cap, int64_t gap_step, int32_t n_bins, uint64_t *d_hist, uint32_t *d_gap, void *stream) {
  if (gap_cap < 1 || gap_cap > 0x7FFFFFFEll) return tsim_fail(TSIM_EINVAL, "gap_cap = %lld (1 .. 2^31 - 2)", (long long)gap_cap);
  if (gap_step < 1 || gap_step > 0x7FFFFFFEll) return tsim_fail(TSIM_EINVAL, "gap_step = %lld (1 .. 2^31 - 2)", (long long)gap_step);
  if (n_bins < 2 || n_bins > 1024) return tsim_fail(TSIM_EINVAL, "n_bins = %d (2 .. 1024)", n_bins);
  if (!d_hist || reinterpret_cast<uintptr_t>(d_hist) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_hist is NULL or not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_gap) % 4 != 0) return tsim_fail(TSIM_EINVAL, "d_gap is not 4-byte aligned");
  if (!h) return tsim_fail(TSIM_EINVAL, "decoder is NULL");
  if (!h->a.gap) return tsim_fail(TSIM_EINVAL, "the handle has no class table (tsim_uf_create_matching_gap makes one)");
  SoftOut soft{0, n_bins, d_hist, d_gap};
  soft.gap_cap = (uint32_t)gap_cap, soft.gap_step = (uint32_t)gap_step;
  return uf_decode(h, d_rows, n, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters, d_pred, &soft, stream);
}

extern "C" int tsim_uf_gap_table(tsim_uf *h, uint32_t *dist2, int64_t *w0) {
  if (!h || !dist2 || !w0) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!h->a.gap) return tsim_fail(TSIM_EINVAL, "the handle has no class table (tsim_uf_create_matching_gap makes one)");
  const size_t pairs = (size_t)h->a.n_nodes * (size_t)h->a.n_nodes;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy(dist2, h->gtable.dist2, pairs * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *w0 = h->w0;
  return TSIM_OK;
}

extern "C" int tsim_uf_match_table(tsim_uf *h, uint32_t *dist, uint64_t *mask) {
  if (!h || !dist || !mask) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!h->a.match_k) return tsim_fail(TSIM_EINVAL, "the handle has no match table (tsim_uf_create_matching makes one)");
  const size_t pairs = (size_t)h->a.n_nodes * (size_t)h->a.n_nodes;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy(dist, h->table.dist, pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(mask, h->table.mask, pairs * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return TSIM_OK;
}
