// tsim_uf_host.hip.h - the host side that the two union-find handles share (tsim_uf.hip, tsim_ufw.hip): the checks of a graph,
// its caps and its heralds, the waves of a block, and the row arguments and launch loop of a decode
// call, on the prelude of tsim_host.hip.h.  Host code only; every check comes before the first device call of its caller.
#pragma once

#include "tsim_host.hip.h"
#include "tsim_uf.hip.h"

#include <algorithm>
#include <vector>

namespace ufh {
constexpr int kMaxIndex = 65535;               // nodes, and edges, of a graph a wave decodes: uint16 indices
constexpr int64_t kRowsPerLaunch = 1ll << 30;  // a block's uint32 partials cannot overflow

// The graph (u < v inside the nodes, pairs strictly ascending), its row columns and its caps.  0, or an error code after
// tsim_fail.  n_det: the detector columns of a row; max_cap: 0 without caps.
inline int check_graph(const tsim_uf_desc *desc, const uint8_t *edge_cap, const tsim_uf_heralds *her, long long *n_det_out, int *max_cap_out) {
  const int N = desc->n_nodes, E = desc->n_edges;
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
  *n_det_out = n_det, *max_cap_out = max_cap;
  return TSIM_OK;
}

// The heralds of a graph that check_graph passed: every column a node or one herald, the lists inside the edges.  Sets the
// columns of the nodes in dmask and of the heralds in hmask (ceil(n_cols / 8) zeroed bytes each) and, unless it is NULL,
// col_herald[c] = i for the column c of herald i (n_det entries of -1).  0, or an error code after tsim_fail.
inline int check_heralds(const tsim_uf_desc *desc, const tsim_uf_heralds *her, long long n_det, uint8_t *dmask, uint8_t *hmask,
                         int32_t *col_herald) {
  const int N = desc->n_nodes, E = desc->n_edges, H = her->n_heralds;
  if (!her->node_det || !her->herald_ptr || (H > 0 && !her->herald_det)) return tsim_fail(TSIM_EINVAL, "a herald array is NULL");
  for (int v = 0; v < N - 1; ++v) {
    const int32_t c = her->node_det[v];
    if (c < 0 || c >= n_det) return tsim_fail(TSIM_EINVAL, "node_det[%d] = %d leaves the columns 0 .. %lld", v, c, n_det - 1);
    if (v > 0 && her->node_det[v - 1] >= c) return tsim_fail(TSIM_EINVAL, "node_det[%d] = %d: the columns of the nodes must be strictly ascending", v, c);
    dmask[c >> 3] |= (uint8_t)(1u << (c & 7));
  }
  for (int i = 0; i < H; ++i) {
    const int32_t c = her->herald_det[i];
    if (c < 0 || c >= n_det) return tsim_fail(TSIM_EINVAL, "herald_det[%d] = %d leaves the columns 0 .. %lld", i, c, n_det - 1);
    if ((dmask[c >> 3] | hmask[c >> 3]) >> (c & 7) & 1)
      return tsim_fail(TSIM_EINVAL, "column %d is named twice (a column is a node or one herald)", c);
    hmask[c >> 3] |= (uint8_t)(1u << (c & 7));
    if (col_herald) col_herald[c] = i;
  }
  if (her->herald_ptr[0] != 0) return tsim_fail(TSIM_EINVAL, "herald_ptr[0] = %d", her->herald_ptr[0]);
  for (int i = 0; i < H; ++i)
    if (her->herald_ptr[i + 1] < her->herald_ptr[i])
      return tsim_fail(TSIM_EINVAL, "herald_ptr[%d] = %d after %d: it must not fall", i + 1, her->herald_ptr[i + 1], her->herald_ptr[i]);
  const int n_listed = her->herald_ptr[H];
  if (n_listed > 0 && !her->herald_edges) return tsim_fail(TSIM_EINVAL, "herald_edges is NULL");
  for (int k = 0; k < n_listed; ++k)
    if (her->herald_edges[k] < 0 || her->herald_edges[k] >= E)
      return tsim_fail(TSIM_EINVAL, "herald_edges[%d] = %d of %d edges", k, her->herald_edges[k], E);
  return TSIM_OK;
}

// Starts k_match_table (csrc/tsim_uf_match.hip.h; the kernel lives in tsim_uf.hip) on the null stream of the current device: the
// match table of a graph of n_nodes nodes, or of one window's slices of the windows' tables, under the match weights w.  mask
// and parent may be NULL: not wanted.
hipError_t launch_match_table(int n_nodes, const uint32_t *edge_uv, const unsigned long long *edge_obs, const uint16_t *w, const uint32_t *adj_ptr,
                              const uint16_t *adj_edge, uint32_t *dist, unsigned long long *mask, uint16_t *parent);

// the waves of a block whose shots take `shot` bytes of LDS each (16 + shot fit a block): as many shots on a CU as its LDS
// holds, in the fewest blocks
inline void choose_waves(long long shot, int *waves, int *per_cu) {
  int best = 0;
  *per_cu = 1;
  for (int w = 1; w <= ufk::kMaxWaves; ++w) {
    const long long block = 16 + w * shot;
    if (block > ufk::kLdsBlock) break;
    const int blocks = (int)std::min<long long>(ufk::kLdsCU / block, 32 / w);
    if (blocks * w >= best) best = blocks * w, *waves = w, *per_cu = blocks;
  }
}

// The row arguments of a decode call, for a.n_cols columns.  0, or an error code after tsim_fail.
template <class Args>
int check_rows(const Args &a, const uint8_t *d_rows, int64_t n, int64_t row_bytes, int32_t obs_lo, int32_t obs_hi, const uint64_t *d_counters,
               const uint64_t *d_pred) {
  if (n < 0) return tsim_fail(TSIM_EINVAL, "negative n");
  if (const int64_t used = tsimh::row_used(a.n_cols, row_bytes); used < 0) return (int)used;
  if (n > 0 && !d_rows) return tsim_fail(TSIM_EINVAL, "d_rows is NULL");
  if (obs_lo < 0 || obs_hi < obs_lo || obs_hi > a.n_cols || obs_hi - obs_lo > 64)
    return tsim_fail(TSIM_EINVAL, "observable columns %d .. %d of %d (at most 64)", obs_lo, obs_hi, a.n_cols);
  if (!d_counters || reinterpret_cast<uintptr_t>(d_counters) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_counters is NULL or not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_pred) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_pred is not 8-byte aligned");
  return TSIM_OK;
}

// What a soft decode call adds to the row arguments, set into a's metric, n_bins and hist.  0, or an error code after tsim_fail.
template <class Args>
int check_soft(Args &a, int32_t metric, int32_t n_bins, uint64_t *d_hist, const uint32_t *d_soft) {
  if (metric < 0 || metric > 3) return tsim_fail(TSIM_EINVAL, "metric = %d (0 rounds, 1 full_edges, 2 largest_cluster, 3 correction_weight)", metric);
  if (n_bins < 2 || n_bins > 1024) return tsim_fail(TSIM_EINVAL, "n_bins = %d (2 .. 1024)", n_bins);
  if (!d_hist || reinterpret_cast<uintptr_t>(d_hist) % 8 != 0) return tsim_fail(TSIM_EINVAL, "d_hist is NULL or not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_soft) % 16 != 0) return tsim_fail(TSIM_EINVAL, "d_soft is not 16-byte aligned");
  a.metric = metric;
  a.n_bins = n_bins;
  a.hist = reinterpret_cast<unsigned long long *>(d_hist);
  return TSIM_OK;
}

// what every launch of a decode call reads the same (check_rows passed)
template <class Args>
void fill_rows(Args &a, const uint8_t *d_rows, int64_t row_bytes, const uint8_t *d_xor, const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi,
               uint64_t *d_counters) {
  a.rb = row_bytes;
  a.used = (a.n_cols + 7) / 8;
  a.xr = d_xor;
  a.test = d_test;
  a.w8 = reinterpret_cast<uintptr_t>(d_rows) % 8 == 0 && row_bytes % 8 == 0;
  a.obs_lo = obs_lo;
  a.obs_hi = obs_hi;
  a.dec = reinterpret_cast<unsigned long long *>(d_counters);
}

// the n rows in launches of at most kRowsPerLaunch: launch(a, first row, blocks, LDS bytes) starts the kernel on a's rows
template <class Args, class Launch>
int launch_rows(Args &a, const uint8_t *d_rows, int64_t n, uint64_t *d_pred, int grid, int64_t *launches, Launch launch) {
  const size_t lds = 16 + (size_t)a.waves * a.shot_bytes;
  for (int64_t r0 = 0; r0 < n; r0 += kRowsPerLaunch) {
    a.n = std::min(kRowsPerLaunch, n - r0);
    a.rows = d_rows + r0 * a.rb;
    a.pred = d_pred ? reinterpret_cast<unsigned long long *>(d_pred) + r0 : nullptr;
    const int64_t tiles = (a.n + 63) / 64;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + a.waves - 1) / a.waves, grid));
    launch(a, r0, blocks, lds);
    HIP_TRY(hipGetLastError());
    ++*launches;
  }
  return TSIM_OK;
}
}  // namespace ufh
