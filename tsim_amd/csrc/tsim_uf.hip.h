// tsim_uf.hip.h - the union-find (cluster-growth) decoder over bit-packed device rows (tsim_uf_*); the rule is the module
// docstring of tsim_amd/decode.py, which is also its numpy statement.  Rows, xor, test and the keep rule are the row contract of
// tsim_bitrows.hip.h, read straight from global memory (row_word); a row's syndrome is row ^ xor at columns 0 .. n_nodes - 2.
//
// One wave owns a tile of 64 rows (a persistent grid).  Pass 1, row r = lane r: the keep mask, "has a defect" and the
// observables, read straight from the row; a row without defects is finished here and touches no per-shot state.  Pass 2:
// the kept rows with defects, one after the other, each decoded by the whole wave on the wave's own state in LDS:
//   label[v]  uint16  the cluster of v: min-label propagation over the full edges, by plain stores repeated to the fixpoint
//                     (a store only ever lowers a label to another label of the same cluster, so the fixpoint is the
//                     smallest index of the cluster whichever store wins a race: the root the forest rule wants)
//   lp[v]     uint32  level << 16 | parent edge: atomicMin of (level(u) + 1) << 16 | e over the full edges, to the fixpoint,
//                     is the breadth-first level and the smallest-index edge to the level above
//   s[v]      uint8   the defect, then the peeling state (32-bit LDS XOR on the word that holds the byte)
//   par[v]    uint8   the parity of the defects of the cluster whose root is v (same XOR)
//   half, full        bitmaps over the edges: grown >= 1, grown == 2.  A round visits the nodes of the active clusters and
//                     ORs the half bit of every edge at such a node; the visit that finds it set (from an earlier round, or
//                     from the other end in this round) ORs the full bit - grown + active(u) + active(v), capped at 2, in
//                     any order of the visits
//   cnt       uint32  (weighted growth, in the place of `half`) grown[e] as a 4-bit counter, eight edges to a word: a visit
//                     adds 1 to the edge's nibble; the visit whose old nibble is cap[e] - 1 ORs the full bit.  An edge that
//                     is not full starts a round at <= cap - 1 and is visited at most once from each end, so the nibble ends
//                     at <= cap + 1 <= 15 (caps are 1 .. 14) and never carries; past the cap it means nothing, fullness is
//                     the full bit - grown + active(u) + active(v), capped at cap[e], in any order of the visits
//   wlist     uint16  the 32-bit words of `full` that are not zero (appended by the lane that set a word's first bit; the
//                     order is arbitrary and nothing depends on it): labels, levels and peeling sweep these words only, a
//                     lane per word, so no step of a shot sweeps all edges
// The edge table (u | v << 16), the observable masks, the caps (uint8, weighted growth only) and the node adjacency (CSR) are
// read-only in global memory.
// Heralded erasures (k_uf<Weighted, true>, tsim_uf_create_heralds): herald detectors are no nodes.  Pass 1 takes "has a defect"
// from the columns of dmask (the non-herald detectors), so a row with heralds only is finished there; s[v] comes from column
// node_det[v - 1]; and before the first round a pre-grow step sets the full bit of every edge listed under a herald whose
// column is set (a lane per 8-byte word of the row, col_herald[c] -> herald_ptr -> herald_edges), appending a word of `full`
// to wlist when it was zero: the append rule of the growth.  half and the counters stay zero: visits test `full` first.
// Soft outputs (k_uf<Weighted, Heralds, true>, tsim_uf_decode_soft_device; "Soft outputs" in the docstring): four numbers of a
// decoded row, read off the state above when growth ends, miss or not, without a byte of LDS of their own.  rounds: grow()
// counts them.  full_edges: the popcount of the listed words of `full`.  largest_cluster: lp[] is dead between grow() and
// forest(), so every end of a full edge adds 1 to lp[label[x]], once, and the largest count is taken.  correction_weight: counted
// by the lane that flips an edge, in the function handed to peel().  The three per-lane numbers are reduced over the wave in
// registers.  Of a tile's rows those of bin 0 (every kept row without a defect among them) are counted by ballot into
// registers and flushed once per wave; the others go to the histogram by global 64-bit adds, one per distinct bin of the tile
// (SoftBins, which k_ufw shares).
// Cluster matching (k_uf<Weighted, false, false, true>, tsim_uf_create_matching; "Decoding a row" of the cluster-matching section
// of the docstring): growth is the one above.  Then lp[], dead until forest(), counts the defects of every cluster at its root,
// par[], dead after growth, marks the roots (1: matched, 1 .. K defects; 2: peeled, more), and a sweep of the nodes compacted by
// ballot lists the defects of the matched clusters in ascending node order in lp[].  Each matched cluster in turn, by the whole
// wave: its defects are compacted out of that list the same way, its K (K + 1) / 2 + K distances are read from the match table
// (global memory; tsim_uf_match.hip.h builds it) into LDS, the dynamic program runs by layers of popcount(S), lanes over the
// subsets, keeping per subset the cost (uint32: at most 12 finite terms below 2^27 each, so the 64-bit sum of the rule fits) and
// the candidate that won, and one lane walks the winners back from the full set, XORing the table's masks.  forest() and peel()
// run only when a peeled cluster exists, and a flip counts only when its child node lies in one.
// The complementary gap (k_uf<Weighted, false, false, true, true>, tsim_uf_create_matching_gap; "Complementary gap" in the docstring):
// the winner program above runs as it is, and beside it, in the same layers, the class program g[S] = (least cost of a pairing
// of S whose paths' class bits XOR to 0, to 1), a uint2 per subset in LDS, from the class distances of the cluster's pairs
// (dist2 of tsim_uf_match.hip.h, a uint2 per pair, read from global memory into LDS with the distances).  A finite class
// distance is below 2^28 and a pairing has at most 12 terms, so a finite cost is below 3 * 2^30 and kCostInf = 2^32 - 1 is never
// reached by a sum.  The cluster's gap, the zero of a peeled cluster and of a miss fold into one wave-uniform number per row,
// whose deficit cap - gap is binned as the soft kernel bins its metric.  The arrays exist only in the layout of such a handle
// (Args::gap): a handle of tsim_uf_create_matching keeps its bytes per shot and its waves per block.
// Cluster matching under heralds (k_uf<Weighted, true, false, true, Gap, true>, tsim_uf_create_matching_heralds; "Cluster matching
// under heralds" in the docstring): pregrow_heralds also sets the edge's bit in `ebits`, the row's erased edges.  After
// mark_clusters bit 1 of s[v] tags every non-boundary end of an erased edge.  A cluster of 1 .. K defects in turn, by the whole
// wave: its hubs are its defects, then its tagged nodes that are no defect, both compacted by ballot in ascending node order;
// more than H hubs make it a peeled cluster (par[r] = 2).  The hubs' n * n + n static distances and masks (uint2 class pairs with
// Gap) are read from the tables into LDS, every erased edge of the cluster lowers the entry of its pair of hubs (the pairs of a
// graph are distinct, so one lane writes an entry), the distances relax in the ordered k loop of the docstring, lanes over
// (i, j) - row and column k stand still in step k - and the classes relax in place until a sweep lowers nothing: a least
// fixpoint, whichever lane writes first.  The boundary folds into the defects' rows, the results go where match_cluster reads
// its distances, and the layered programs run as they are; lane 0 walks the winners back over the masks in LDS.  An erased edge
// is an edge of the graph, so a finite hub distance is at most the static one of its pair, below 2^27 (2^28 for a class): the
// bounds of the programs stand.  Every step is a fixpoint, a minimum over a fixed set or the ordered k loop.
// Every index into LDS comes from tables tsim_uf_create has checked; every address is formed in 64 bits.
#pragma once
#include "tsim_bitrows.hip.h"

namespace ufk {

using namespace bitrows;  // wsync, mask_word, below, row_word, row_obs

constexpr int kMaxWaves = 4;             // shots (waves) per block at most
constexpr uint32_t kNone = 0xFFFFFFFFu;  // lp of a node no level has reached
constexpr int kLdsBlock = 64 * 1024;     // LDS a block may ask for
constexpr int kLdsCU = 160 * 1024;
constexpr int kMaxCap = 14;              // of an edge: its 4-bit counter may pass the cap by one
constexpr int kMaxMatchNodes = 2048;     // of a graph with a match table (uint32 + uint64 per pair of nodes)
constexpr int kMaxMatchDefects = 12;     // K at most: 2^K subsets of a cluster's defects in LDS
constexpr int kMaxMatchHubs = 32;        // H at most: [H][H] hub distances in LDS
constexpr uint32_t kMatchInf = 0x7FFFFFFFu;  // a distance of the match table: no path
constexpr uint32_t kCostInf = 0xFFFFFFFFu;   // a cost of the dynamic program: no pairing
constexpr uint8_t kViaBoundary = 15, kViaNone = 255;  // the candidate that won a subset: a defect 0 .. 11, the boundary, none

struct Args {
  const uint8_t *rows;
  long long n, rb;            // rows, row stride in bytes
  int n_cols, used;           // columns; bytes of a row that hold them
  const uint8_t *xr, *test;   // optional rows of `used` bytes (NULL: none)
  int w8;                     // the row pointer and rb are multiples of 8
  int n_nodes, n_edges, w32;  // w32: 32-bit words of an edge bitmap
  const uint32_t *edge_uv;    // [n_edges] u | v << 16
  const unsigned long long *edge_obs;
  const uint8_t *cap;         // [n_edges] 1 .. 14, or NULL: every cap is 2 (the half / full bitmaps)
  int w_cnt;                  // 32-bit words of the 4-bit counters (weighted growth), 0 without caps
  const uint32_t *adj_ptr;    // [n_nodes + 1]
  const uint16_t *adj_edge;   // the edges at a node
  int obs_lo, obs_hi;
  int waves, shot_bytes;      // waves of a block; LDS bytes of one wave's state
  int off_lp, off_s, off_par, off_half, off_full, off_wlist, off_misc;
  unsigned long long *dec;    // [0] kept [1] wrong [2] missed
  unsigned long long *pred;   // [n] or NULL
  unsigned long long *stats;  // [0] most growth rounds [1] rows decoded in LDS [2] clusters matched [3] clusters peeled
  //                             [4] matched clusters with an erased edge [5] clusters peeled for their hubs (the last two pairs: such handles only)
  // heralded erasures (NULL / 0 on a handle without heralds)
  int n_det_cols;              // detector columns of a row: the nodes but the boundary, and the heralds
  const int32_t *node_det;     // [n_nodes - 1] the column of node v at v - 1
  const uint8_t *dmask, *hmask;  // rows of ceil(n_cols / 8) bytes: the columns of the nodes, of the heralds
  const int32_t *col_herald;   // [n_det_cols] the herald of a herald column
  const int32_t *herald_ptr;   // [n_heralds + 1]
  const int32_t *herald_edges;
  // soft outputs (k_uf<., ., true> only)
  int metric, n_bins;          // 0 rounds 1 full_edges 2 largest_cluster 3 correction_weight; the bin of x is min(x, n_bins - 1)
  unsigned long long *hist;    // [2 * n_bins] kept rows per bin, then the wrong ones among them
  uint32_t *soft;              // [4 * n] the four values of every row (16-byte aligned), or NULL
  // cluster matching (k_uf<., false, false, true> only; 0 / NULL on other handles)
  int match_k;                 // K in 1 .. 12: a cluster of 1 .. K defects is matched, a larger one peeled
  int off_mcost, off_mch, off_mcl, off_mpd;
  const uint32_t *mdist;       // [n_nodes * n_nodes] the match table: distances (kMatchInf: none) ...
  const unsigned long long *mmask;  // ... and the observables of the paths
  // the complementary gap (k_uf<., false, false, true, true> only; 0 / NULL on other handles)
  int gap;                     // 1 on a handle of tsim_uf_create_matching_gap: layout() adds the class program's arrays
  int off_gcost, off_gpd;
  uint32_t gap_cap, gap_step;  // G >= 1 and the width of a bin of the deficit G - gap
  const uint32_t *gdist;       // [n_nodes * n_nodes * 2] the class table: the two distances of a pair side by side (8-byte aligned)
  // cluster matching under heralds (k_uf<., true, false, true, ., true> only; 0 / NULL on other handles)
  int max_hubs;                // H in K .. 32: a cluster of 1 .. K defects and at most H hubs is matched; 0 on other handles
  int gap_obs;                 // the observable of the class table: the class of an erased edge is this bit of its mask
  uint32_t erased_w;           // w_h: an erased edge e of the cluster weighs min(match_w[e], w_h)
  int off_ebits, off_hub, off_hd, off_hm, off_hb, off_hmb, off_bm, off_hd2, off_hb2;
  const uint16_t *match_w;     // [n_edges] the match weights
};

// the layout of one wave's state, shared by the host (sizes, limits) and the kernel
__host__ __device__ inline int a16(long long x) { return (int)((x + 15) / 16 * 16); }
__host__ inline long long layout(Args *a) {
  const long long N = a->n_nodes, W = a->w32;
  long long at = a16(2 * N);
  a->off_lp = (int)at, at += a16(4 * N);
  a->off_s = (int)at, at += a16(N);
  a->off_par = (int)at, at += a16(N);
  a->off_half = (int)at, at += a16(4 * (a->w_cnt ? (long long)a->w_cnt : W));  // (the counters lie where `half` would)
  a->off_full = (int)at, at += a16(4 * W);
  a->off_wlist = (int)at, at += a16(2 * W);
  a->off_misc = (int)at, at += 16;
  if (const long long K = a->match_k) {  // the dynamic program: costs, winners, the cluster's defects, its distances [K][K + 1]
    a->off_mcost = (int)at, at += a16(4ll << K);
    a->off_mch = (int)at, at += a16(1ll << K);
    a->off_mcl = (int)at, at += a16(2 * K);
    a->off_mpd = (int)at, at += a16(4 * K * (K + 1));
    if (a->gap) {  // the class program: two costs per subset, two distances per pair
      a->off_gcost = (int)at, at += a16(8ll << K);
      a->off_gpd = (int)at, at += a16(8 * K * (K + 1));
    }
    if (const long long H = a->max_hubs) {  // the hub graph: the erased edges, the hubs, distances and masks [H][H] and [H], folded masks [K]
      a->off_ebits = (int)at, at += a16(4 * W);
      a->off_hub = (int)at, at += a16(2 * H);
      a->off_hd = (int)at, at += a16(4 * H * H);
      a->off_hm = (int)at, at += a16(8 * H * H);
      a->off_hb = (int)at, at += a16(4 * H);
      a->off_hmb = (int)at, at += a16(8 * H);
      a->off_bm = (int)at, at += a16(8 * K);
      if (a->gap) {
        a->off_hd2 = (int)at, at += a16(8 * H * H);
        a->off_hb2 = (int)at, at += a16(8 * H);
      }
    }
  }
  return at;
}

// pass 1 of a lane's row: *fail = the test columns that are set, *defects = the detector columns that are set (after xor);
// dmask: the detector columns as a mask row, NULL for the columns 0 .. nd - 1
template <class R>
__device__ __forceinline__ void scan_row(const R &a, const uint8_t *row, bool valid, const uint8_t *dmask, int nd, uint64_t *fail,
                                         uint64_t *defects) {
  *fail = 0, *defects = 0;
  for (int b = 0; b < a.used; b += 8) {
    const uint64_t tw = mask_word(a.test, b, a.used) & below(b, a.n_cols),  // (pad bits are not columns)
        dw = dmask ? mask_word(dmask, b, a.used) : below(b, nd);
    if ((tw | dw) == 0) continue;
    const uint64_t w = (valid ? row_word(a, row, b) : 0ull) ^ mask_word(a.xr, b, a.used);
    *fail |= w & tw;
    *defects |= w & dw;
  }
}

struct State {
  uint16_t *label;
  uint32_t *lp, *s32, *par32, *half, *full, *misc;  // misc: [0] listed words [1] deepest level [2] [3] the prediction
  //                                                   (half: the 4-bit counters when the growth is weighted)
  uint8_t *s, *par;
  uint16_t *wlist;
  uint32_t *mcost, *mpd;  // cluster matching only
  uint8_t *mch;
  uint16_t *mcl;
  uint2 *gcost, *gpd;  // the complementary gap only: .x class 0, .y class 1
  uint32_t *ebits, *hd, *hb;  // cluster matching under heralds only: the erased edges (a bitmap), hub distances [n][n], to the boundary [n]
  uint16_t *hub;
  unsigned long long *hm, *hmb, *bm;  // the masks of hd, of hb, and of the defects' folded boundary distances
  uint2 *hd2, *hb2;                   // with the gap: the class distances of hd and hb
};

// a wave's state at `base`, by the offsets layout() has put into `a`
template <class L>
__device__ __forceinline__ State state_at(const L &a, uint8_t *base) {
  State st;
  st.label = reinterpret_cast<uint16_t *>(base);
  st.lp = reinterpret_cast<uint32_t *>(base + a.off_lp);
  st.s = base + a.off_s;
  st.s32 = reinterpret_cast<uint32_t *>(st.s);
  st.par = base + a.off_par;
  st.par32 = reinterpret_cast<uint32_t *>(st.par);
  st.half = reinterpret_cast<uint32_t *>(base + a.off_half);
  st.full = reinterpret_cast<uint32_t *>(base + a.off_full);
  st.wlist = reinterpret_cast<uint16_t *>(base + a.off_wlist);
  st.misc = reinterpret_cast<uint32_t *>(base + a.off_misc);
  return st;
}
// the same with the arrays of the dynamic program (a handle of tsim_uf_create_matching, of tsim_ufw_create_matching)
template <class L>
__device__ __forceinline__ State match_state_at(const L &a, uint8_t *base) {
  State st = state_at(a, base);
  st.mcost = reinterpret_cast<uint32_t *>(base + a.off_mcost);
  st.mch = base + a.off_mch;
  st.mcl = reinterpret_cast<uint16_t *>(base + a.off_mcl);
  st.mpd = reinterpret_cast<uint32_t *>(base + a.off_mpd);
  return st;
}
// the same with the arrays of the class program (a handle of tsim_uf_create_matching_gap)
__device__ __forceinline__ State gap_state_at(const Args &a, uint8_t *base) {
  State st = match_state_at(a, base);
  st.gcost = reinterpret_cast<uint2 *>(base + a.off_gcost);
  st.gpd = reinterpret_cast<uint2 *>(base + a.off_gpd);
  return st;
}

// the same with the arrays of the hub graph (a handle of tsim_uf_create_matching_heralds)
__device__ __forceinline__ State hub_state_at(const Args &a, uint8_t *base) {
  State st = a.gap ? gap_state_at(a, base) : match_state_at(a, base);
  st.ebits = reinterpret_cast<uint32_t *>(base + a.off_ebits);
  st.hub = reinterpret_cast<uint16_t *>(base + a.off_hub);
  st.hd = reinterpret_cast<uint32_t *>(base + a.off_hd);
  st.hm = reinterpret_cast<unsigned long long *>(base + a.off_hm);
  st.hb = reinterpret_cast<uint32_t *>(base + a.off_hb);
  st.hmb = reinterpret_cast<unsigned long long *>(base + a.off_hmb);
  st.bm = reinterpret_cast<unsigned long long *>(base + a.off_bm);
  st.hd2 = reinterpret_cast<uint2 *>(base + a.off_hd2);
  st.hb2 = reinterpret_cast<uint2 *>(base + a.off_hb2);
  return st;
}

// The steps of one shot, each by the whole wave.  `G` is the graph they run on: Args here, one window's tables in
// tsim_ufw.hip.h (n_nodes, w32, w_cnt, edge_uv, edge_obs, cap, adj_ptr, adj_edge).  decode_shot below is their order.

// f(e, u, v) for every full edge, a lane per listed word
template <class G, class F>
__device__ __forceinline__ void full_edges(const G &a, const State &st, int n_words, int lane, F f) {
  for (int i = lane; i < n_words; i += 64) {
    const int w = st.wlist[i];
    uint32_t bits = st.full[w];
    while (bits) {
      const int e = 32 * w + __builtin_ctz(bits);
      bits &= bits - 1;
      const uint32_t uv = a.edge_uv[e];
      f(e, (int)(uv & 0xFFFFu), (int)(uv >> 16));
    }
  }
}

// s[v] = the defect of node v, from the row; every node its own cluster
template <bool Heralds>
__device__ __forceinline__ void load_defects(const Args &a, const State &st, const uint8_t *row, int lane) {
  const int N = a.n_nodes;
  for (int v = lane; v < N; v += 64) {
    uint32_t bit = 0;
    if (v) {
      int c = v - 1;
      if constexpr (Heralds) c = a.node_det[c];
      uint32_t byte = row[c >> 3];
      if (a.xr) byte ^= a.xr[c >> 3];
      bit = (byte >> (c & 7)) & 1u;
    }
    st.s[v] = (uint8_t)bit;
    st.label[v] = (uint16_t)v;
  }
}

// no edge has grown, no word is listed, the prediction is 0
template <bool Weighted, class G>
__device__ __forceinline__ void clear_edges(const G &a, const State &st, int lane) {
  if constexpr (Weighted) {
    for (int i = lane; i < a.w_cnt; i += 64) st.half[i] = 0;
    for (int i = lane; i < a.w32; i += 64) st.full[i] = 0;
  } else {
    for (int i = lane; i < a.w32; i += 64) st.half[i] = 0, st.full[i] = 0;
  }
  if (lane < 4) st.misc[lane] = 0;
  wsync();
}

// the edges of the heralds that are set start full; Erasure: and are the row's erased edges, a bit each in ebits (zeroed)
template <bool Erasure = false>
__device__ __forceinline__ void pregrow_heralds(const Args &a, const State &st, const uint8_t *row, int lane) {
  const int det_bytes = (a.n_det_cols + 7) >> 3;
  for (int b = 8 * lane; b < det_bytes; b += 8 * 64) {
    const uint64_t hw = mask_word(a.hmask, b, a.used);
    if (hw == 0) continue;
    const uint64_t w0 = (row_word(a, row, b) ^ mask_word(a.xr, b, a.used)) & hw;
    for (uint64_t w = w0; w; w &= w - 1) {
      const int h = a.col_herald[8 * b + __builtin_ctzll(w)];
      for (int k = a.herald_ptr[h]; k < a.herald_ptr[h + 1]; ++k) {
        const int e = a.herald_edges[k], fw = e >> 5;
        if constexpr (Erasure) atomicOr(&st.ebits[fw], 1u << (e & 31));
        if (atomicOr(&st.full[fw], 1u << (e & 31)) == 0) st.wlist[atomicAdd(&st.misc[0], 1u)] = (uint16_t)fw;  // (each word once)
      }
    }
  }
  wsync();
}

// growth to its end: true for a miss; *rounds is wave-uniform
template <bool Weighted, class G>
__device__ __forceinline__ bool grow(const G &a, const State &st, int lane, int *rounds) {
  const int N = a.n_nodes;
  *rounds = 0;
  for (;;) {
    const int n_words = (int)st.misc[0];
    for (;;) {  // the clusters: labels to their fixpoint (they stay upper bounds from round to round: clusters only merge)
      bool moved = false;
      full_edges(a, st, n_words, lane, [&](int, int u, int v) {
        const uint16_t lu = st.label[u], lv = st.label[v];
        if (lu < lv) st.label[v] = lu, moved = true;
        else if (lv < lu) st.label[u] = lv, moved = true;
      });
      wsync();
      if (!__builtin_amdgcn_ballot_w64(moved)) break;
    }
    for (int i = lane; i < (N + 3) / 4; i += 64) st.par32[i] = 0;
    wsync();
    for (int v = lane; v < N; v += 64)
      if (st.s[v]) {
        const int l = st.label[v];
        atomicXor(&st.par32[l >> 2], 1u << (8 * (l & 3)));
      }
    wsync();
    bool active = false, changed = false;
    for (int v = lane; v < N; v += 64) {
      const int l = st.label[v];
      if (l == 0 || !st.par[l]) continue;
      active = true;
      for (uint32_t k = a.adj_ptr[v]; k < a.adj_ptr[v + 1]; ++k) {
        const int e = a.adj_edge[k], w = e >> 5;
        const uint32_t bit = 1u << (e & 31);
        if (st.full[w] & bit) continue;  // (bits are only ever set: a set bit read here is final)
        if constexpr (Weighted) {
          const int sh = 4 * (e & 7);
          const uint32_t old = (atomicAdd(&st.half[e >> 3], 1u << sh) >> sh) & 15u, cap = a.cap[e];
          if (old >= cap) continue;  // (filled from the other end in this round)
          changed = true;
          if (old + 1 < cap) continue;
          // (old == cap - 1: one visit only sees it, so the bit is set once)
          if (atomicOr(&st.full[w], bit) == 0) st.wlist[atomicAdd(&st.misc[0], 1u)] = (uint16_t)w;
        } else {
          if (!(atomicOr(&st.half[w], bit) & bit)) {
            changed = true;
            continue;
          }
          const uint32_t was = atomicOr(&st.full[w], bit);
          if (was & bit) continue;
          changed = true;
          if (was == 0) st.wlist[atomicAdd(&st.misc[0], 1u)] = (uint16_t)w;  // (each word once: at most w32 entries)
        }
      }
    }
    wsync();
    if (!__builtin_amdgcn_ballot_w64(active)) return false;
    if (!__builtin_amdgcn_ballot_w64(changed)) return true;
    ++*rounds;
  }
}

// the forest: lp[v] = level << 16 | parent edge, the deepest level in misc[1]
template <class G>
__device__ __forceinline__ void forest(const G &a, const State &st, int lane) {
  const int N = a.n_nodes;
  const int n_words = (int)st.misc[0];
  for (int v = lane; v < N; v += 64) st.lp[v] = st.label[v] == v ? 0u : kNone;
  wsync();
  for (;;) {
    bool moved = false;
    full_edges(a, st, n_words, lane, [&](int e, int u, int v) {
      const uint32_t pu = st.lp[u], pv = st.lp[v];
      if (pu != kNone) {
        const uint32_t cand = ((pu >> 16) + 1) << 16 | (uint32_t)e;
        if (cand < pv && cand < atomicMin(&st.lp[v], cand)) moved = true;
      }
      if (pv != kNone) {
        const uint32_t cand = ((pv >> 16) + 1) << 16 | (uint32_t)e;
        if (cand < pu && cand < atomicMin(&st.lp[u], cand)) moved = true;
      }
    });
    wsync();
    if (!__builtin_amdgcn_ballot_w64(moved)) break;
  }
  full_edges(a, st, n_words, lane, [&](int, int u, int v) { atomicMax(&st.misc[1], max(st.lp[u], st.lp[v]) >> 16); });
  wsync();
}

// peeling: an edge is looked at by the level of the end whose parent edge it is.  flip(e, u, v) is called by the lane that
// flips edge e = (u, v) and returns the observables this flips; the return value is this lane's XOR of them.
template <class G, class F>
__device__ __forceinline__ uint64_t peel(const G &a, const State &st, int lane, F flip) {
  const int n_words = (int)st.misc[0];
  uint64_t flips = 0;
  for (int level = (int)st.misc[1]; level >= 1; --level) {
    full_edges(a, st, n_words, lane, [&](int e, int u, int v) {
      const uint32_t want = (uint32_t)level << 16 | (uint32_t)e;
      int child = -1, parent = 0;
      if (st.lp[v] == want) child = v, parent = u;
      else if (st.lp[u] == want) child = u, parent = v;
      if (child < 0 || !st.s[child]) return;
      atomicXor(&st.s32[parent >> 2], 1u << (8 * (parent & 3)));  // (the parent is of the level above: nobody reads it in this pass)
      flips ^= flip(e, u, v);
    });
    wsync();
  }
  return flips;
}

// the wave's XOR of the lanes' flips, kept in two 32-bit words of LDS (zero, or what earlier calls left)
__device__ __forceinline__ uint64_t fold_flips(uint32_t *words, uint64_t flips) {
  if (flips) {
    atomicXor(&words[0], (uint32_t)flips);
    atomicXor(&words[1], (uint32_t)(flips >> 32));
  }
  wsync();
  return (uint64_t)words[0] | (uint64_t)words[1] << 32;
}

// the wave's sum / maximum of a value per lane, in every lane (a butterfly in registers)
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += (uint32_t)__shfl_xor((int)x, m, 64);
  return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, m, 64));
  return x;
}
// the same for a sum in the high and a maximum in the low 16 bits (the sum stays below 2^16), in one butterfly
__device__ __forceinline__ uint32_t wave_sum_max(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, m, 64);
    x = ((x >> 16) + (y >> 16)) << 16 | max(x & 0xFFFFu, y & 0xFFFFu);
  }
  return x;
}

// the soft outputs of the state growth has left, miss or not: soft[0] full edges, soft[1] the nodes of the largest cluster
// (wave-uniform).  The labels are the clusters of the full edges (grow() ends on a round that changed no edge); lp[] is free
// until forest() fills it.
// A cluster of more than one node is made of ends of full edges, its root among them, so only those are visited, in two sweeps
// of the full edges: lp[x] = 0 at every end (and the edges are counted); then the first visit of an end sets bit 31 of lp[x]
// and adds 1 to lp[label[x]], whose low bits so count the cluster's nodes: the add that completes a cluster reads its size
// less one, so the largest value any add has read, plus one, is the largest cluster (1 when no edge is full).
template <class G>
__device__ __forceinline__ void soft_of_growth(const G &a, const State &st, int lane, uint32_t *soft) {
  constexpr uint32_t kSeen = 0x80000000u;
  const int n_words = (int)st.misc[0];
  uint32_t full = 0, most = 1;  // (both at most 65535: edges, nodes)
  full_edges(a, st, n_words, lane, [&](int, int u, int v) { st.lp[u] = 0, st.lp[v] = 0, ++full; });
  wsync();
  full_edges(a, st, n_words, lane, [&](int, int u, int v) {
    if (!(atomicOr(&st.lp[u], kSeen) & kSeen)) most = max(most, (atomicAdd(&st.lp[st.label[u]], 1u) & ~kSeen) + 1u);
    if (!(atomicOr(&st.lp[v], kSeen) & kSeen)) most = max(most, (atomicAdd(&st.lp[st.label[v]], 1u) & ~kSeen) + 1u);
  });
  wsync();  // (forest() writes lp[] next)
  const uint32_t both = wave_sum_max(full << 16 | most);
  soft[0] = both >> 16;
  soft[1] = both & 0xFFFFu;
}

// The binning of a soft value x per row, for k_uf and k_ufw (`A`: their Args, n_bins and hist): the bin of x is min(x, n_bins - 1).
// Of a tile's rows those of bin 0 (every kept row without a defect among them) are counted by ballot into registers; the others
// go to the histogram by global 64-bit adds, one per distinct bin of the tile.  Lane 0 flushes the registers once per wave into
// stat[3], the block's count of bin 0 in LDS (zeroed by the kernel), which one thread adds to hist[0] after the block's barrier.
struct SoftBins {
  uint32_t bin0 = 0, bin0_wrong = 0;  // wave-uniform: the kept rows of bin 0, the wrong ones among them

  // a tile: lane = row; kept and wrong (kept, and predicted wrongly) are this lane's row's
  template <class A>
  __device__ __forceinline__ void tile(const A &a, uint32_t x, bool kept, bool wrong, int lane) {
    const uint32_t bin = min(x, (uint32_t)a.n_bins - 1u);
    bin0 += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && bin == 0));
    bin0_wrong += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(wrong && bin == 0));
    uint64_t todo = __builtin_amdgcn_ballot_w64(kept && bin != 0);
    while (todo) {  // one add per distinct bin of the tile (and one for its wrong rows)
      const uint32_t b = (uint32_t)__shfl((int)bin, __builtin_ctzll(todo), 64);
      const uint64_t same = __builtin_amdgcn_ballot_w64(kept && bin == b), bad = __builtin_amdgcn_ballot_w64(wrong && bin == b);
      if (lane == 0) {
        atomicAdd(&a.hist[b], (unsigned long long)__popcll(same));
        if (bad) atomicAdd(&a.hist[(size_t)a.n_bins + b], (unsigned long long)__popcll(bad));
      }
      todo &= ~same;
    }
  }
  // after the wave's tiles, by its lane 0
  template <class A>
  __device__ __forceinline__ void wave_done(const A &a, uint32_t *stat) const {
    if (bin0) atomicAdd(&stat[3], bin0);
    if (bin0_wrong) atomicAdd(&a.hist[a.n_bins], (unsigned long long)bin0_wrong);  // (rare: wrong without a defect, or in bin 0)
  }
  // after the block's barrier, by every thread
  template <class A>
  __device__ __forceinline__ static void block_done(const A &a, const uint32_t *stat) {
    if (threadIdx.x == 3 && stat[3]) atomicAdd(&a.hist[0], (unsigned long long)stat[3]);
  }
};

// The steps of cluster matching, between grow() and forest(), each by the whole wave.
// the lanes with `flag`, compacted in lane order behind the *at entries there are: this lane's place (if it has the flag)
__device__ __forceinline__ int compact(bool flag, int lane, int *at) {
  const uint64_t b = __builtin_amdgcn_ballot_w64(flag);
  const int pos = *at + __popcll(b & ((1ull << lane) - 1ull));
  *at += __popcll(b);
  return pos;
}

// The clusters growth has left (not a miss) on the graph `a` (Args, or a window of tsim_ufw.hip.h), K = max_defects: par[r] of a
// root r = 1 for a MATCHED cluster (1 .. K defects), 2 for a PEELED one (more), 0 for one without a defect;
// lp[0 .. *n_list - 1] = the defects of the matched clusters, ascending.  counts[0] and counts[1]: the matched and the peeled
// clusters (wave-uniform).
template <class G>
__device__ __forceinline__ void mark_clusters(const G &a, int K, const State &st, int lane, int *n_list, uint32_t *counts) {
  const int N = a.n_nodes;
  for (int v = lane; v < N; v += 64) st.lp[v] = 0;
  wsync();
  for (int v = lane; v < N; v += 64)
    if (st.s[v]) atomicAdd(&st.lp[st.label[v]], 1u);  // (s[0] = 0: the boundary is no defect)
  wsync();
  uint32_t both = 0;  // matched << 16 | peeled, at most 65535 clusters in all
  for (int v = lane; v < N; v += 64) {
    const uint32_t m = st.lp[v];  // (0 off the roots)
    const uint8_t mark = m == 0 ? 0 : m <= (uint32_t)K ? 1 : 2;
    st.par[v] = mark;
    both += mark == 1 ? 0x10000u : mark == 2 ? 1u : 0u;
  }
  wsync();  // (the counts are read: lp[] is free for the list)
  int at = 0;
  for (int v0 = 0; v0 < N; v0 += 64) {
    const int v = v0 + lane;
    const bool flag = v < N && st.s[v] && st.par[st.label[v]] == 1;
    const int pos = compact(flag, lane, &at);
    if (flag) st.lp[pos] = (uint32_t)v;  // (pos <= v: at most one entry per node)
  }
  wsync();
  *n_list = at;
  both = wave_sum(both);
  counts[0] = both >> 16;
  counts[1] = both & 0xFFFFu;
}

// The layered programs of a cluster of m defects over mpd (and, with Gap, gpd), rows of m + 1 entries: the distances of defect i
// to the defects j > i, at [m] to the boundary; mcost[0] (and gcost[0]) are set.  Per subset the winner's cost and candidate in
// mcost / mch, with Gap the two classes' costs in gcost.
template <bool Gap>
__device__ __forceinline__ void pair_programs(const State &st, int lane, int m) {
  const int n_sets = 1 << m, W = m + 1;
  for (int layer = 1; layer <= m; ++layer) {  // f[S] reads subsets of one and of two defects less
    for (int S = lane; S < n_sets; S += 64) {
      if (__popc((unsigned)S) != layer) continue;
      const int i = __builtin_ctz(S), R = S & (S - 1);
      uint32_t best = kCostInf;
      uint8_t via = kViaNone;
      const uint32_t fR = st.mcost[R], b = st.mpd[i * W + m];
      if (fR != kCostInf && b != kMatchInf) best = fR + b, via = kViaBoundary;
      for (int rest = R; rest; rest &= rest - 1) {  // ascending j; strict < keeps the first of least cost
        const int j = __builtin_ctz(rest);
        const uint32_t f = st.mcost[R ^ (1 << j)], d = st.mpd[i * W + j];
        if (f != kCostInf && d != kMatchInf && f + d < best) best = f + d, via = (uint8_t)j;
      }
      st.mcost[S] = best;
      st.mch[S] = via;
      if constexpr (Gap) {  // a pure minimum of costs: g[S][b] over the class cb of the pair's path and g[.][b ^ cb] of the rest
        uint32_t g0 = kCostInf, g1 = kCostInf;
        const auto offer = [&](const uint2 f, const uint2 d) {
          if (f.x != kCostInf && d.x != kMatchInf) g0 = min(g0, f.x + d.x);
          if (f.y != kCostInf && d.y != kMatchInf) g0 = min(g0, f.y + d.y);
          if (f.x != kCostInf && d.y != kMatchInf) g1 = min(g1, f.x + d.y);
          if (f.y != kCostInf && d.x != kMatchInf) g1 = min(g1, f.y + d.x);
        };
        offer(st.gcost[R], st.gpd[i * W + m]);
        for (int rest = R; rest; rest &= rest - 1) {
          const int j = __builtin_ctz(rest);
          offer(st.gcost[R ^ (1 << j)], st.gpd[i * W + j]);
        }
        st.gcost[S] = make_uint2(g0, g1);
      }
    }
    wsync();
  }
}

// The defects of the cluster of root r, which are the entries of label r in lp[from .. n_list), into mcl[], ascending: how many
// (a matched cluster has 1 .. K).
__device__ __forceinline__ int cluster_defects(const State &st, int lane, int from, int n_list, int r, int K) {
  int m = 0;
  for (int i0 = from; i0 < n_list; i0 += 64) {
    const int i = i0 + lane;
    const int v = i < n_list ? (int)st.lp[i] : 0;
    const bool flag = i < n_list && st.label[v] == r;
    const int pos = compact(flag, lane, &m);
    if (flag && pos < K) st.mcl[pos] = (uint16_t)v;  // (a matched cluster has at most K defects: pos < K)
  }
  wsync();
  return min(m, K);
}

// The distances of the m defects in mcl[] from `dist`, the match table of a graph of N nodes, into mpd, rows of m + 1 entries as
// pair_programs reads them; mcost[0].  The caller's wsync() comes before the programs.
__device__ __forceinline__ void cluster_distances(const State &st, int lane, int m, const uint32_t *dist, size_t N) {
  const int W = m + 1;  // a row of mpd: the distances of defect i to the defects j > i, at [m] to the boundary
  for (int t = lane; t < m * W; t += 64) {
    const int i = t / W, j = t % W;
    if (j <= i) continue;
    st.mpd[t] = dist[(size_t)st.mcl[i] * N + (j < m ? (size_t)st.mcl[j] : 0)];
  }
  if (lane == 0) st.mcost[0] = 0;
}

// One matched cluster, of root r, by the whole wave: the mask of the dynamic program of the docstring over its defects, which
// are the entries of label r in lp[from .. n_list).  The result is in lane 0 (0 in the other lanes).  Gap: *gap = min(*gap, the
// cluster's gap) in every lane, the gap being |g0 - g1| of the class program at the full set, a.gap_cap when one class is infinite.
// (Its first two steps are the functions above, which k_ufw shares: there the winners are walked back to pairs and their paths.)
template <bool Gap = false>
__device__ __forceinline__ uint64_t match_cluster(const Args &a, const State &st, int lane, int from, int n_list, int r, uint32_t *gap = nullptr) {
  const size_t N = (size_t)a.n_nodes;
  const int m = cluster_defects(st, lane, from, n_list, r, a.match_k);
  cluster_distances(st, lane, m, a.mdist, N);
  if constexpr (Gap) {
    const int W = m + 1;
    for (int t = lane; t < m * W; t += 64) {
      const int i = t / W, j = t % W;
      if (j <= i) continue;
      st.gpd[t] = reinterpret_cast<const uint2 *>(a.gdist)[(size_t)st.mcl[i] * N + (j < m ? (size_t)st.mcl[j] : 0)];
    }
    if (lane == 0) st.gcost[0] = make_uint2(0u, kCostInf);
  }
  wsync();
  const int n_sets = 1 << m;
  pair_programs<Gap>(st, lane, m);
  if constexpr (Gap) {  // (one address for the wave: the number is wave-uniform)
    const uint2 g = st.gcost[n_sets - 1];
    const uint32_t mine = g.x != kCostInf && g.y != kCostInf ? (g.x > g.y ? g.x - g.y : g.y - g.x) : a.gap_cap;
    *gap = min(*gap, mine);
  }
  uint64_t mask = 0;
  if (lane == 0)
    for (int S = n_sets - 1; S;) {  // the winners, from the full set down: S loses one or two defects per step
      const int i = __builtin_ctz(S), R = S & (S - 1), via = st.mch[S];
      if (via == kViaNone) break;  // (no pairing: a cluster is connected and holds an even number of defects or node 0)
      const size_t row = (size_t)st.mcl[i] * N;
      if (via == kViaBoundary) mask ^= a.mmask[row], S = R;
      else mask ^= a.mmask[row + st.mcl[via]], S = R ^ (1 << via);  // (via is a defect of R: below m)
    }
  wsync();  // (the next cluster overwrites the arrays)
  return mask;
}

// f(i, r), by the whole wave, for every matched cluster in the order of its smallest defect lp[i]; r is its root
template <class F>
__device__ __forceinline__ void matched_clusters(const State &st, int lane, int n_list, F f) {
  for (int i = 0; i < n_list; ++i) {
    const int r = __builtin_amdgcn_readfirstlane((int)st.label[st.lp[i]]);
    if (__builtin_amdgcn_readfirstlane((int)st.par[r]) != 1) continue;  // (matched before, by an earlier defect of its)
    f(i, r);
    if (lane == 0) st.par[r] = 3;
    wsync();
  }
}

// every matched cluster, in the order of its smallest defect: the XOR of their masks, in lane 0; Gap: *gap as match_cluster
template <bool Gap = false>
__device__ __forceinline__ uint64_t match_clusters(const Args &a, const State &st, int lane, int n_list, uint32_t *gap = nullptr) {
  uint64_t mask = 0;
  matched_clusters(st, lane, n_list, [&](int i, int r) { mask ^= match_cluster<Gap>(a, st, lane, i, n_list, r, gap); });
  return mask;
}

// The steps of cluster matching under heralds, in the place of match_clusters.
// bit 1 of s[v] for every non-boundary end v of an erased edge of the row (bit 0 stays the defect); untag_erased takes it back
// before peel() reads s[]
__device__ __forceinline__ void tag_erased(const Args &a, const State &st, int lane) {
  for (int w = lane; w < a.w32; w += 64)
    for (uint32_t bits = st.ebits[w]; bits; bits &= bits - 1) {
      const uint32_t uv = a.edge_uv[32 * w + __builtin_ctz(bits)];
      const int u = (int)(uv & 0xFFFFu), v = (int)(uv >> 16);
      if (u) atomicOr(&st.s32[u >> 2], 2u << (8 * (u & 3)));
      atomicOr(&st.s32[v >> 2], 2u << (8 * (v & 3)));
    }
  wsync();
}
__device__ __forceinline__ void untag_erased(const Args &a, const State &st, int lane) {
  for (int v = lane; v < a.n_nodes; v += 64) st.s[v] &= 1;
  wsync();
}

// a + b of two distances, kMatchInf when one is (finite ones are below 2^28)
__device__ __forceinline__ uint32_t add_inf(uint32_t x, uint32_t y) { return x == kMatchInf || y == kMatchInf ? kMatchInf : x + y; }
// the two classes of a walk made of one of classes x and one of classes y
__device__ __forceinline__ uint2 join_classes(uint2 x, uint2 y) {
  return make_uint2(min(add_inf(x.x, y.x), add_inf(x.y, y.y)), min(add_inf(x.x, y.y), add_inf(x.y, y.x)));
}

// One cluster of root r with 1 .. K defects (the entries of label r in lp[from .. n_list)), by the whole wave, over its hub graph:
// the mask of the winner program in lane 0 (0 in the other lanes), *gap as match_cluster.  *erased: the cluster has an erased
// edge; *overflow: it has more than H hubs, nothing is matched and the result is 0 (both wave-uniform).
template <bool Gap>
__device__ __forceinline__ uint64_t hub_cluster(const Args &a, const State &st, int lane, int from, int n_list, int r, uint32_t *gap, bool *erased,
                                                bool *overflow) {
  const int K = a.match_k, H = a.max_hubs, N = a.n_nodes;
  int m = 0;
  for (int i0 = from; i0 < n_list; i0 += 64) {
    const int i = i0 + lane;
    const int v = i < n_list ? (int)st.lp[i] : 0;
    const bool flag = i < n_list && st.label[v] == r;
    const int pos = compact(flag, lane, &m);
    if (flag && pos < K) st.hub[pos] = (uint16_t)v;  // (at most K defects: pos < K <= H)
  }
  m = min(m, K);
  int n = m;
  for (int v0 = 0; v0 < N; v0 += 64) {  // the other ends of its erased edges: tagged, no defect (s[0] is never tagged)
    const int v = v0 + lane;
    const bool flag = v < N && st.s[v] == 2 && st.label[v] == r;
    const int pos = compact(flag, lane, &n);
    if (flag && pos < H) st.hub[pos] = (uint16_t)v;
  }
  wsync();
  *overflow = n > H;
  if (*overflow) {
    *erased = true;
    return 0;
  }
  // the static distances of the hubs, and to the boundary
  for (int t = lane; t < n * n; t += 64) {
    const size_t x = st.hub[t / n], y = st.hub[t % n], at = min(x, y) * (size_t)N + max(x, y);
    st.hd[t] = a.mdist[at];
    st.hm[t] = a.mmask[at];
    if constexpr (Gap) st.hd2[t] = reinterpret_cast<const uint2 *>(a.gdist)[at];
  }
  for (int x = lane; x < n; x += 64) {
    const size_t at = (size_t)st.hub[x] * (size_t)N;
    st.hb[x] = a.mdist[at];
    st.hmb[x] = a.mmask[at];
    if constexpr (Gap) st.hb2[x] = reinterpret_cast<const uint2 *>(a.gdist)[at];
  }
  wsync();
  // its erased edges: a pair of nodes has one edge, so an entry has one writer
  bool any = false;
  for (int w = lane; w < a.w32; w += 64)
    for (uint32_t bits = st.ebits[w]; bits; bits &= bits - 1) {
      const int e = 32 * w + __builtin_ctz(bits);
      const uint32_t uv = a.edge_uv[e];
      const int u = (int)(uv & 0xFFFFu), v = (int)(uv >> 16);
      if (st.label[v] != r) continue;
      any = true;
      int i = -1, j = -1;
      for (int x = 0; x < n; ++x) {
        if (st.hub[x] == u) i = x;
        if (st.hub[x] == v) j = x;
      }
      if (j < 0 || (u && i < 0)) continue;  // (never: both ends are tagged nodes of the cluster)
      const uint32_t x = min((uint32_t)a.match_w[e], a.erased_w);
      const unsigned long long obs = a.edge_obs[e];
      const bool odd = (obs >> a.gap_obs) & 1ull;
      if (u) {
        if (x < st.hd[i * n + j]) st.hd[i * n + j] = st.hd[j * n + i] = x, st.hm[i * n + j] = st.hm[j * n + i] = obs;
        if constexpr (Gap) {
          uint2 d = st.hd2[i * n + j];
          if (odd) d.y = min(d.y, x);
          else d.x = min(d.x, x);
          st.hd2[i * n + j] = st.hd2[j * n + i] = d;
        }
      } else {
        if (x < st.hb[j]) st.hb[j] = x, st.hmb[j] = obs;
        if constexpr (Gap) {
          uint2 d = st.hb2[j];
          if (odd) d.y = min(d.y, x);
          else d.x = min(d.x, x);
          st.hb2[j] = d;
        }
      }
    }
  wsync();
  *erased = __builtin_amdgcn_ballot_w64(any) != 0;
  if (*erased) {  // (without an erased edge the static distances obey the triangle inequality: nothing would move)
    for (int k = 0; k < n; ++k) {  // the ordered relaxation: row and column k stand still in step k
      for (int t = lane; t < n * n; t += 64) {
        const int i = t / n, j = t % n;
        if (i == j || i == k || j == k) continue;
        const uint32_t via = add_inf(st.hd[i * n + k], st.hd[k * n + j]);
        if (via < st.hd[t]) st.hd[t] = via, st.hm[t] = st.hm[i * n + k] ^ st.hm[k * n + j];
      }
      wsync();
    }
    if constexpr (Gap)
      for (;;) {  // the classes: in place to the least fixpoint (an entry only ever falls, to the weight of a walk)
        bool moved = false;
        for (int t = lane; t < n * n; t += 64) {
          const int i = t / n, j = t % n;
          const uint2 was = st.hd2[t];
          uint2 d = was;
          for (int k = 0; k < n; ++k) {
            const uint2 via = join_classes(st.hd2[i * n + k], st.hd2[k * n + j]);
            d.x = min(d.x, via.x), d.y = min(d.y, via.y);
          }
          if (d.x != was.x || d.y != was.y) st.hd2[t] = d, moved = true;
        }
        wsync();
        if (!__builtin_amdgcn_ballot_w64(moved)) break;
      }
  }
  // the boundary folds into the defects' rows; the results go where the layered programs read them
  const int W = m + 1;
  for (int t = lane; t < m * W; t += 64) {
    const int i = t / W, j = t % W;
    if (j <= i) continue;
    if (j < m) {
      st.mpd[t] = st.hd[i * n + j];
      if constexpr (Gap) st.gpd[t] = st.hd2[i * n + j];
      continue;
    }
    uint32_t best = st.hb[i];
    unsigned long long mask = st.hmb[i];
    for (int x = 0; x < n; ++x) {  // ascending x; strict < keeps the first of least cost
      if (x == i) continue;
      const uint32_t via = add_inf(st.hd[i * n + x], st.hb[x]);
      if (via < best) best = via, mask = st.hm[i * n + x] ^ st.hmb[x];
    }
    st.mpd[t] = best;
    st.bm[i] = mask;
    if constexpr (Gap) {
      uint2 d = make_uint2(kMatchInf, kMatchInf);
      for (int x = 0; x < n; ++x) {
        const uint2 via = join_classes(st.hd2[i * n + x], st.hb2[x]);
        d.x = min(d.x, via.x), d.y = min(d.y, via.y);
      }
      st.gpd[t] = d;
    }
  }
  if (lane == 0) {
    st.mcost[0] = 0;
    if constexpr (Gap) st.gcost[0] = make_uint2(0u, kCostInf);
  }
  wsync();
  const int n_sets = 1 << m;
  pair_programs<Gap>(st, lane, m);
  if constexpr (Gap) {
    const uint2 g = st.gcost[n_sets - 1];
    const uint32_t mine = g.x != kCostInf && g.y != kCostInf ? (g.x > g.y ? g.x - g.y : g.y - g.x) : a.gap_cap;
    *gap = min(*gap, mine);
  }
  uint64_t mask = 0;
  if (lane == 0)
    for (int S = n_sets - 1; S;) {  // the winners, from the full set down, over the masks in LDS
      const int i = __builtin_ctz(S), R = S & (S - 1), via = st.mch[S];
      if (via == kViaNone) break;
      if (via == kViaBoundary) mask ^= st.bm[i], S = R;
      else mask ^= st.hm[i * n + via], S = R ^ (1 << via);  // (via is a defect of R: below m <= n)
    }
  wsync();  // (the next cluster overwrites the arrays)
  return mask;
}

// every cluster of 1 .. K defects, in the order of its smallest defect: the XOR of the matched ones' masks, in lane 0; *gap as
// match_cluster.  A cluster of more than H hubs becomes a peeled one: counts[0] / counts[1], the matched and the peeled clusters
// of mark_clusters, move by one; counts[2]: the matched clusters with an erased edge, counts[3]: those peeled for their hubs.
template <bool Gap>
__device__ __forceinline__ uint64_t hub_clusters(const Args &a, const State &st, int lane, int n_list, uint32_t *gap, uint32_t *counts) {
  uint64_t mask = 0;
  counts[2] = counts[3] = 0;
  tag_erased(a, st, lane);
  for (int i = 0; i < n_list; ++i) {
    const int r = __builtin_amdgcn_readfirstlane((int)st.label[st.lp[i]]);
    if (__builtin_amdgcn_readfirstlane((int)st.par[r]) != 1) continue;  // (seen before, by an earlier defect of its)
    bool erased, overflow;
    mask ^= hub_cluster<Gap>(a, st, lane, i, n_list, r, gap, &erased, &overflow);
    if (overflow) --counts[0], ++counts[1], ++counts[3];
    else if (erased) ++counts[2];
    if (lane == 0) st.par[r] = overflow ? 2 : 3;
    wsync();
  }
  untag_erased(a, st, lane);
  return mask;
}

// one kept row with a defect, by the whole wave: the prediction (0 for a miss); *missed and *rounds are wave-uniform, and so
// are, with Soft, soft[0 .. 2]: full edges, largest cluster, correction weight; with Match, soft[0 .. 1]: the clusters matched
// and peeled; with Gap, soft[2]: the row's gap, min(a.gap_cap, the least gap of its clusters), 0 with a peeled cluster and for a miss;
// with Erasure (soft has five entries), soft[2 .. 3]: the matched clusters with an erased edge and the clusters peeled for their
// hubs, soft[4]: the row's gap
template <bool Weighted, bool Heralds, bool Soft, bool Match = false, bool Gap = false, bool Erasure = false>
__device__ __forceinline__ uint64_t decode_shot(const Args &a, const State &st, const uint8_t *row, int lane, bool *missed, int *rounds,
                                                uint32_t *soft) {
  load_defects<Heralds>(a, st, row, lane);
  if constexpr (Erasure)
    for (int i = lane; i < a.w32; i += 64) st.ebits[i] = 0;
  clear_edges<Weighted>(a, st, lane);
  if constexpr (Heralds) pregrow_heralds<Erasure>(a, st, row, lane);
  *missed = grow<Weighted>(a, st, lane, rounds);
  if constexpr (Soft) soft_of_growth(a, st, lane, soft), soft[2] = 0;
  if constexpr (Match) soft[0] = soft[1] = 0;
  if constexpr (Gap) soft[2] = 0;
  if constexpr (Erasure) soft[2] = soft[3] = soft[4] = 0;
  if (*missed) return 0;
  if constexpr (Match) {
    int n_list;
    mark_clusters(a, a.match_k, st, lane, &n_list, soft);
    uint32_t gap = a.gap_cap;
    uint64_t flips;
    if constexpr (Erasure) flips = hub_clusters<Gap>(a, st, lane, n_list, &gap, soft);
    else flips = match_clusters<Gap>(a, st, lane, n_list, &gap);
    if constexpr (Gap) soft[Erasure ? 4 : 2] = soft[1] ? 0u : gap;
    if (soft[1]) {  // a flip counts when its edge, and so its child node, lies in a peeled cluster
      forest(a, st, lane);
      flips ^= peel(a, st, lane, [&](int e, int u, int) { return st.par[st.label[u]] == 2 ? a.edge_obs[e] : 0ull; });
    }
    return fold_flips(&st.misc[2], flips);
  }
  forest(a, st, lane);
  uint32_t flipped = 0;  // by this lane
  const uint64_t flips = peel(a, st, lane, [&](int e, int, int) {
    if constexpr (Soft) ++flipped;
    return a.edge_obs[e];
  });
  if constexpr (Soft) soft[2] = wave_sum(flipped);
  return fold_flips(&st.misc[2], flips);
}

template <bool Weighted, bool Heralds, bool Soft = false, bool Match = false, bool Gap = false, bool Erasure = false>
__global__ void __launch_bounds__(64 * kMaxWaves) k_uf(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  uint32_t *stat = reinterpret_cast<uint32_t *>(lds_raw);  // kept, wrong, missed; with Soft or Gap: the kept rows of bin 0
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *base = lds_raw + 16 + (size_t)wave * a.shot_bytes;
  const State st = Erasure ? hub_state_at(a, base) : Gap ? gap_state_at(a, base) : Match ? match_state_at(a, base) : state_at(a, base);
  if (threadIdx.x < 4) stat[threadIdx.x] = 0;
  __syncthreads();
  uint32_t kept_acc = 0, wrong_acc = 0, miss_acc = 0, decoded_acc = 0;  // wave-uniform
  int most_rounds = 0;
  SoftBins bins;                              // (Soft, Gap) the wave's rows of bin 0
  uint32_t matched_acc = 0, peeled_acc = 0;   // (Match) wave-uniform: the clusters matched and peeled
  uint32_t erased_acc = 0, hubs_acc = 0;      // (Erasure) wave-uniform: the matched clusters with an erased edge, those peeled for their hubs
  const int nd = a.n_nodes - 1;
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * a.waves + wave; t < tiles; t += (long long)gridDim.x * a.waves) {
    const long long r = (t << 6) + lane;
    const bool valid = r < a.n;
    const uint8_t *row = a.rows + (valid ? r : 0) * a.rb;
    uint64_t fail, defects;
    scan_row(a, row, valid, Heralds ? a.dmask : nullptr, nd, &fail, &defects);
    const bool kept = valid && fail == 0;
    const uint64_t obs = kept ? row_obs(a, row) : 0;
    uint64_t pred = 0;
    bool missed = false;
    uint32_t mine[4] = {0, 0, 0, 0};  // (Soft) this lane's row: rounds, full edges, largest cluster, correction weight
    uint32_t deficit = 0;             // (Gap) this lane's row: gap_cap - its gap; 0 for a row that is not decoded
    uint64_t work = __builtin_amdgcn_ballot_w64(kept && defects != 0);
    while (work) {
      const int src = __builtin_ctzll(work);
      work &= work - 1;
      bool m;
      int rounds;
      uint32_t soft[Erasure ? 5 : 3];
      const uint64_t p = decode_shot<Weighted, Heralds, Soft, Match, Gap, Erasure>(a, st, a.rows + ((t << 6) + src) * a.rb, lane, &m, &rounds, soft);
      if constexpr (Match) matched_acc += soft[0], peeled_acc += soft[1];
      if constexpr (Erasure) erased_acc += soft[2], hubs_acc += soft[3];
      if (lane == src) pred = p, missed = m;
      if constexpr (Soft)
        if (lane == src) mine[0] = (uint32_t)rounds, mine[1] = soft[0], mine[2] = soft[1], mine[3] = soft[2];
      if constexpr (Gap)
        if (lane == src) deficit = a.gap_cap - soft[Erasure ? 4 : 2];
      most_rounds = max(most_rounds, rounds);
      ++decoded_acc;
    }
    kept_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept));
    wrong_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && pred != obs));
    miss_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && missed));
    if (a.pred && valid) a.pred[r] = pred;  // (0 for a row that is not kept, and for a miss)
    if constexpr (Soft || Gap) {
      uint32_t x;
      if constexpr (Gap) x = deficit / a.gap_step;
      else x = a.metric == 0 ? mine[0] : a.metric == 1 ? mine[1] : a.metric == 2 ? mine[2] : mine[3];
      bins.tile(a, x, kept, kept && pred != obs, lane);
      if constexpr (Gap) {
        if (a.soft && valid) a.soft[r] = deficit;  // (uint32[n] on this call; 0 for a row that is not kept)
      } else {
        if (a.soft && valid) reinterpret_cast<uint4 *>(a.soft)[r] = make_uint4(mine[0], mine[1], mine[2], mine[3]);  // (zeros for a row that is not kept)
      }
    }
  }
  if (lane == 0) {
    if (kept_acc) atomicAdd(&stat[0], kept_acc);
    if (wrong_acc) atomicAdd(&stat[1], wrong_acc);
    if (miss_acc) atomicAdd(&stat[2], miss_acc);
    if (most_rounds) atomicMax(&a.stats[0], (unsigned long long)most_rounds);
    if (decoded_acc) atomicAdd(&a.stats[1], (unsigned long long)decoded_acc);
    if constexpr (Match) {
      if (matched_acc) atomicAdd(&a.stats[2], (unsigned long long)matched_acc);
      if (peeled_acc) atomicAdd(&a.stats[3], (unsigned long long)peeled_acc);
    }
    if constexpr (Erasure) {
      if (erased_acc) atomicAdd(&a.stats[4], (unsigned long long)erased_acc);
      if (hubs_acc) atomicAdd(&a.stats[5], (unsigned long long)hubs_acc);
    }
    if constexpr (Soft || Gap) bins.wave_done(a, stat);
  }
  __syncthreads();
  if (threadIdx.x < 3 && stat[threadIdx.x]) atomicAdd(&a.dec[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
  if constexpr (Soft || Gap) SoftBins::block_done(a, stat);
}

}  // namespace ufk
