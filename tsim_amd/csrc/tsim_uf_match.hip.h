// tsim_uf_match.hip.h - the match table of a cluster-matching union-find handle (tsim_uf_create_matching): per source node the
// least sum of the edges' match weights to every node and the observables of that path ("Match table" in the module docstring
// of tsim_amd/decode.py, which is also its numpy statement).  Built once, by tsim_uf_create_matching; k_uf<., ., ., true> of
// tsim_uf.hip.h reads it.
//
// One block per source a.  The row lives in LDS: dist[v] uint32 (kMatchInf: no path), mask[v] uint64, pe[v] uint16 the parent
// edge (kNoEdge: none), done[v] uint16.  Three steps, each to its fixpoint, so no order of the threads can change a number:
//   distances  every node v >= 1 with a finite distance offers dist[v] + w[e] to the other end of each of its edges by
//              atomicMin, until a sweep lowers nothing.  Node 0 never offers: no path continues from the boundary.
//   parents    a thread per node v != a with a finite distance: the first edge of its list (ascending edge index) whose other
//              end x >= 1 has dist[x] + w[e] == dist[v].
//   masks      mask[v] = mask[x] ^ edge_obs[pe[v]] once the parent's is known: done[v] is the round after which it is (1 for
//              the source), and a round only takes parents of earlier rounds.  Weights are >= 1, so parents lie strictly
//              nearer and the parent edges are a tree.
// A finite distance is at most 2047 * 65535 < 2^27, so no sum passes kMatchInf.  Every index comes from the tables
// tsim_uf_create_matching has checked; the two stores of a row go to 64-bit addresses.
// tsim_ufw_create_matching builds one table per distinct window with the same kernel ("Cluster matching in windows" in the
// docstring): there `parent` receives the parent edges pe[] (kNoEdge for the source and where there is no path), which k_ufw
// walks, and `mask` is NULL: the masks step does not run and no mask is stored.
#pragma once
#include "tsim_uf.hip.h"

namespace ufk {

constexpr int kTableThreads = 256;
constexpr uint16_t kNoEdge = 0xFFFFu;  // (an edge index is at most 65534)

struct TableArgs {
  int n_nodes;
  const uint32_t *edge_uv;  // [n_edges] u | v << 16
  const unsigned long long *edge_obs;
  const uint16_t *w;        // [n_edges] the match weights, 1 .. 65535
  const uint32_t *adj_ptr;  // [n_nodes + 1]
  const uint16_t *adj_edge;
  uint32_t *dist;           // [n_nodes * n_nodes]
  unsigned long long *mask; // [n_nodes * n_nodes], or NULL: no masks
  uint16_t *parent;         // [n_nodes * n_nodes] the parent edges, or NULL: not wanted
};

__host__ __device__ inline size_t table_lds(int n_nodes) { return 16 * (size_t)n_nodes; }  // 8 + 4 + 2 + 2 bytes per node

__global__ void __launch_bounds__(kTableThreads) k_match_table(TableArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  const int N = a.n_nodes, src = blockIdx.x, tid = threadIdx.x;
  unsigned long long *mask = reinterpret_cast<unsigned long long *>(lds_raw);
  uint32_t *dist = reinterpret_cast<uint32_t *>(lds_raw + 8 * (size_t)N);
  uint16_t *pe = reinterpret_cast<uint16_t *>(lds_raw + 12 * (size_t)N);
  uint16_t *done = reinterpret_cast<uint16_t *>(lds_raw + 14 * (size_t)N);
  const auto other = [&](int e, int v) {
    const uint32_t uv = a.edge_uv[e];
    return (int)(uv & 0xFFFFu) == v ? (int)(uv >> 16) : (int)(uv & 0xFFFFu);
  };
  for (int v = tid; v < N; v += kTableThreads) dist[v] = v == src ? 0u : kMatchInf, mask[v] = 0, pe[v] = kNoEdge, done[v] = v == src;
  __syncthreads();
  for (;;) {
    bool moved = false;
    for (int v = tid; v < N; v += kTableThreads) {
      const uint32_t dv = dist[v];
      if (v == 0 || dv == kMatchInf) continue;
      for (uint32_t k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
        const int e = a.adj_edge[k], x = other(e, v);
        const uint32_t cand = dv + a.w[e];
        if (cand < dist[x] && cand < atomicMin(&dist[x], cand)) moved = true;
      }
    }
    if (!__syncthreads_or(moved)) break;
  }
  for (int v = tid; v < N; v += kTableThreads) {
    const uint32_t dv = dist[v];
    if (v == src || dv == kMatchInf) continue;
    for (uint32_t k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
      const int e = a.adj_edge[k], x = other(e, v);
      if (x == 0 || dist[x] == kMatchInf || dist[x] + a.w[e] != dv) continue;
      pe[v] = (uint16_t)e;
      break;
    }
  }
  __syncthreads();
  for (int round = 1; a.mask; ++round) {  // (at most n_nodes rounds: done[] stays below 2050)
    bool moved = false;
    for (int v = tid; v < N; v += kTableThreads) {
      const int e = pe[v];
      if (done[v] || e == kNoEdge) continue;
      const int x = other(e, v), dx = done[x];
      if (dx == 0 || dx > round) continue;  // (dx == round + 1: set in this round, its mask may not be written yet)
      mask[v] = mask[x] ^ a.edge_obs[e];
      done[v] = (uint16_t)(round + 1);
      moved = true;
    }
    if (!__syncthreads_or(moved)) break;
  }
  for (int v = tid; v < N; v += kTableThreads) {
    const size_t at = (size_t)src * (size_t)N + (size_t)v;
    a.dist[at] = dist[v];
    if (a.mask) a.mask[at] = dist[v] == kMatchInf ? 0ull : mask[v];
    if (a.parent) a.parent[at] = pe[v];
  }
}

// The class table of a handle of tsim_uf_create_matching_gap ("Complementary gap" in the docstring): dist2[a][v][b], the least
// sum of the match weights over walks from a to v whose edges' bit `observable` of edge_obs XOR to b, over the arcs of the
// table above.  One block per source a, the two distances of every node in LDS (8 bytes a node): every state (v, b), v >= 1, of
// finite distance offers dist2[v][b] + w[e] to the state (x, b ^ c(e)) of the other end of each of its edges by atomicMin, until
// a sweep lowers nothing.  Node 0 never offers.  No parents and no masks: a least fixpoint of minima does not depend on the
// order of the threads.  A finite entry is a shortest path over at most 2 n_nodes states, so it is below 4095 * 65535 < 2^28
// and no sum passes kMatchInf.  w0[a] = dist2[a][0][0] + dist2[a][0][1] where a >= 1 and both are finite, else kMatchInf: the
// host takes the minimum.  Indices come from the checked tables; stores go to 64-bit addresses.
struct GapTableArgs {
  int n_nodes, observable;
  const uint32_t *edge_uv;
  const unsigned long long *edge_obs;
  const uint16_t *w;
  const uint32_t *adj_ptr;
  const uint16_t *adj_edge;
  uint32_t *dist2;  // [n_nodes * n_nodes * 2]
  uint32_t *w0;     // [n_nodes]
};

__host__ __device__ inline size_t gap_table_lds(int n_nodes) { return 8 * (size_t)n_nodes; }

__global__ void __launch_bounds__(kTableThreads) k_gap_table(GapTableArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  const int N = a.n_nodes, src = blockIdx.x, tid = threadIdx.x;
  uint32_t *d2 = reinterpret_cast<uint32_t *>(lds_raw);  // the state (v, b) at 2 v + b
  for (int v = tid; v < N; v += kTableThreads) d2[2 * v] = v == src ? 0u : kMatchInf, d2[2 * v + 1] = kMatchInf;
  __syncthreads();
  for (;;) {
    bool moved = false;
    for (int v = tid; v < N; v += kTableThreads) {
      const uint32_t d0 = d2[2 * v], d1 = d2[2 * v + 1];
      if (v == 0 || (d0 == kMatchInf && d1 == kMatchInf)) continue;
      for (uint32_t k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
        const int e = a.adj_edge[k];
        const uint32_t uv = a.edge_uv[e];
        const int x = (int)(uv & 0xFFFFu) == v ? (int)(uv >> 16) : (int)(uv & 0xFFFFu);
        const uint32_t c = (uint32_t)(a.edge_obs[e] >> a.observable) & 1u, w = a.w[e];
        if (d0 != kMatchInf) {
          const uint32_t cand = d0 + w;
          uint32_t *to = &d2[2 * x + (int)c];
          if (cand < *to && cand < atomicMin(to, cand)) moved = true;
        }
        if (d1 != kMatchInf) {
          const uint32_t cand = d1 + w;
          uint32_t *to = &d2[2 * x + (int)(c ^ 1u)];
          if (cand < *to && cand < atomicMin(to, cand)) moved = true;
        }
      }
    }
    if (!__syncthreads_or(moved)) break;
  }
  for (int v = tid; v < N; v += kTableThreads) {
    const size_t at = 2 * ((size_t)src * (size_t)N + (size_t)v);
    a.dist2[at] = d2[2 * v];
    a.dist2[at + 1] = d2[2 * v + 1];
  }
  if (tid == 0) a.w0[src] = src >= 1 && d2[0] != kMatchInf && d2[1] != kMatchInf ? d2[0] + d2[1] : kMatchInf;
}

}  // namespace ufk
