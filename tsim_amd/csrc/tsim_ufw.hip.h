// tsim_ufw.hip.h - sliding-window union-find decoding over bit-packed device rows (tsim_ufw_*); the rule is "Sliding-window
// decoding of long runs" in the module docstring of tsim_amd/decode.py, which is also its numpy statement.  Rows, xor and
// test are those of k_uf (the row contract of tsim_bitrows.hip.h), and so are the grid and the passes: one wave owns a tile
// of 64 rows; pass 1 finishes the rows without a defect straight from the row; pass 2 decodes each kept row with a defect by the whole wave in the
// wave's own state in LDS - here window after window, each by the steps of tsim_uf.hip.h (clear_edges, grow, forest, peel) on
// that window's tables.
//
// The windows' tables lie concatenated in global memory (tsim_ufw_create builds and checks them on the host); WinDesc says
// where a window's part of each begins: edge_uv (u | v << 16, LOCAL nodes: 0 the boundary, c - lo + 1 column c), edge_obs,
// cap (weighted growth only), adj_ptr (n_nodes + 1 entries, relative to the window's part of adj_edge), adj_edge, and commit
// (a bitmap over the local edges: the COMMITTED ones).  The global column of a local node v >= 1 is lo + v - 1, so the ends'
// columns need no table of their own.
//
// A wave's state is ufk::layout() of the largest window (the most nodes, the most edge words, taken separately), then
//   carry   uint32[P / 32]  bit (c mod P) = the toggles that committed flips of earlier windows left at column c, P the
//                           smallest power of two >= max(window, 32).  Window k starts from s[v] = row bit ^ xor bit ^ carry
//                           bit of column lo + v - 1; a committed edge that flips in peeling toggles the bits of its
//                           non-boundary ends (32-bit LDS XOR); when the window advances, the slots of its commit region
//                           [lo, lo + commit) are cleared (a lane per word, plain stores: nobody else touches carry then),
//                           and these are the slots the columns [hi, hi + commit) of the next window use, since P >= window
//   pred    uint32[2]       the prediction so far: the XOR of the masks of the committed flips
// Heralded erasures (k_ufw<Weighted, true>, tsim_ufw_create_heralds; "Sliding windows with heralds" in the docstring): herald
// detectors are no nodes and are never windowed.  Pass 1 takes "has a defect" from the columns of dmask (the nodes'), so a row
// with heralds only is finished there.  Local node v >= 1 of a window reads row column node_det[lo + v - 1]; its carry slot
// stays that of the node index lo + v - 1.  After clear_edges and before grow a pre-grow step strides over the window's own
// herald list - win_herald[off_her .. off_her + n_her), the heralds with a local edge in this window, so the cost follows the
// window, not the row: a lane tests the row bit (after xor) at herald_det[i] and, when it is set, ORs the full bit of the
// local edges win_her_edges[win_her_ptr[j] .. win_her_ptr[j + 1]), appending a word of `full` to wlist when it was zero (the
// idiom of ufk::pregrow_heralds; half and the counters stay zero: visits test `full` first).  The three tables are in global
// memory, concatenated over the windows like the others; win_her_ptr is one CSR over the concatenation, absolute.
// Soft outputs (k_ufw<Weighted, Heralds, true>, tsim_ufw_decode_soft_device; "Soft outputs in windows" in the docstring): four
// numbers of a decoded row, in registers only - the state in LDS, its bytes and the shots of a block are those of the plain
// call.  After grow() of every decoded window, miss or not, ufk::soft_of_growth reads the window's full edges and its largest
// cluster off the state (lp[] is dead until forest()); the first are summed and the second is maximised over the row's windows
// in wave-uniform registers.  rounds is the most of a window, as before.  The lane that flips a committed edge counts it in the
// function handed to peel(); the counts are reduced over the wave once per window and summed (0 for a miss).  The row's lane
// keeps the four numbers; a tile's rows are binned by ufk::SoftBins, as k_uf bins its own.
// Cluster matching (k_ufw<Weighted, false, false, true>, tsim_ufw_create_matching; "Cluster matching in windows" in the
// docstring): per DISTINCT window a match table of its graph under its local weights lies in global memory, dist uint32 and
// parent uint16 per pair of nodes (k_match_table of tsim_uf_match.hip.h builds them; no masks), and WinDesc.off_table says where a
// window's begins, in pairs, as a 64-bit number.  After grow() of a decoded window that is no miss, the steps of k_uf run on the
// window: ufk::mark_clusters, then for every matched cluster ufk::cluster_defects, ufk::cluster_distances from the window's dist
// and ufk::pair_programs.  Lane 0 walks the winners back from the full set and writes the pairs (source, target: another defect,
// or 0 for the boundary) to mpair[] in LDS, at most K of them, their number to misc[2] (free in k_ufw: the prediction is in
// pred[]).  Then a lane per pair walks the pair's PATH through `parent`, from the target back to the source, and hands every edge
// to the function peel() is handed: the committed test, the carry toggles, the mask.  The walk is bounded by the window's nodes
// in its loop condition; one that does not end at its source within them, a parent edge that is none or does not hold the node,
// or a cluster without a finite pairing (none of which a table of k_match_table gives) makes the row a miss.  forest() and peel()
// run only when the window has a peeled cluster, and a peeling flip counts only when its edge lies in one (par[] of the root is
// 2), as in k_uf.  The wave-uniform counts of matched and peeled clusters and the longest path go to stats[3 .. 5].
// Every index into LDS and into the tables comes from tables tsim_ufw_create has built and checked; every address is formed
// in 64 bits.
#pragma once
#include "tsim_uf.hip.h"

namespace ufwk {

struct WinDesc {
  int32_t lo, n_nodes, n_edges, w32;                 // the first column; local nodes and edges; words of an edge bitmap
  int32_t w_cnt, off_edge, off_ptr, off_adj;         // words of the 4-bit counters (0: unweighted); where its tables begin
  int32_t off_commit, last, off_her, n_her;          // last: the run's last window (no slots to clear after it); where its
                                                     // heralds begin in win_herald / win_her_ptr, and how many (0 without heralds)
  long long off_table;                               // cluster matching: where its match table begins in mdist / mparent, in pairs
};

// what the steps of tsim_uf.hip.h read of a graph: one window's
struct Win {
  int n_nodes, n_edges, w32, w_cnt;
  const uint32_t *edge_uv;
  const unsigned long long *edge_obs;
  const uint8_t *cap;
  const uint32_t *adj_ptr;
  const uint16_t *adj_edge;
};

struct Args {
  const uint8_t *rows;
  long long n, rb;           // rows, row stride in bytes
  int n_cols, used;          // columns; bytes of a row that hold them
  const uint8_t *xr, *test;  // optional rows of `used` bytes (NULL: none)
  int w8;                    // the row pointer and rb are multiples of 8
  int nd;                    // detector columns: the global graph's nodes but the boundary
  int obs_lo, obs_hi;
  int waves, shot_bytes;     // waves of a block; LDS bytes of one wave's state
  int off_lp, off_s, off_par, off_half, off_full, off_wlist, off_misc, off_carry, off_pred;
  int n_windows, commit, carry_words;  // carry_words * 32 = P
  const WinDesc *desc;
  const uint32_t *edge_uv;
  const unsigned long long *edge_obs;
  const uint8_t *cap;        // NULL: every cap is 2
  const uint32_t *adj_ptr;
  const uint16_t *adj_edge;
  const uint32_t *commit_bits;
  unsigned long long *dec;    // [0] kept [1] wrong [2] missed
  unsigned long long *pred;   // [n] or NULL
  unsigned long long *stats;  // [0] most growth rounds of a window [1] rows decoded in LDS [2] windows decoded; cluster matching:
  //                             [3] clusters matched [4] clusters peeled [5] the longest path walked
  // heralded erasures (NULL on a handle without heralds)
  const int32_t *node_det;    // [nd] the row column of node v at v - 1
  const uint8_t *dmask;       // a row of ceil(n_cols / 8) bytes: the columns of the nodes
  const int32_t *herald_det;  // [n_heralds] the row column of a herald
  const int32_t *win_herald;  // per window (WinDesc.off_her, n_her) the heralds with a local edge there
  const uint32_t *win_her_ptr;     // [entries of win_herald + 1] where the list of entry j begins in win_her_edges
  const uint16_t *win_her_edges;   // LOCAL edges
  // soft outputs (k_ufw<., ., true> only), as ufk::Args has them
  int metric, n_bins;          // 0 rounds 1 full_edges 2 largest_cluster 3 correction_weight; the bin of x is min(x, n_bins - 1)
  unsigned long long *hist;    // [2 * n_bins] kept rows per bin, then the wrong ones among them
  uint32_t *soft;              // [4 * n] the four values of every row (16-byte aligned), or NULL
  // cluster matching (k_ufw<., false, false, true> only; 0 / NULL on other handles)
  int match_k;                 // K in 1 .. 12: a cluster of 1 .. K defects is matched, a larger one peeled
  int off_mcost, off_mch, off_mcl, off_mpd, off_mpair;  // the arrays of ufk::layout(), and mpair uint16[2 K]
  const uint32_t *mdist;       // the distinct windows' match tables, concatenated: distances (kMatchInf: none) ...
  const uint16_t *mparent;     // ... and parent edges, LOCAL (kNoEdge: none)
};

// the bits j of word w of a bitmap whose index 32 w + j lies in [s, e)
__host__ __device__ inline uint32_t bits_between(int w, int s, int e) {
  const int lo = s - 32 * w > 0 ? s - 32 * w : 0, hi = e - 32 * w < 32 ? e - 32 * w : 32;
  if (hi <= lo) return 0;
  return (hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// the local edges of the window's heralds that are set in the row start full
__device__ __forceinline__ void pregrow_window(const Args &a, const WinDesc &d, const ufk::State &st, const uint8_t *row, int lane) {
  for (int j = lane; j < d.n_her; j += 64) {
    const long long at = (long long)d.off_her + j;
    const int c = a.herald_det[a.win_herald[at]];
    uint32_t byte = row[c >> 3];
    if (a.xr) byte ^= a.xr[c >> 3];
    if (!((byte >> (c & 7)) & 1u)) continue;
    for (uint32_t q = a.win_her_ptr[at]; q < a.win_her_ptr[at + 1]; ++q) {
      const int e = a.win_her_edges[q], fw = e >> 5;
      if (atomicOr(&st.full[fw], 1u << (e & 31)) == 0) st.wlist[atomicAdd(&st.misc[0], 1u)] = (uint16_t)fw;  // (each word once)
    }
  }
  bitrows::wsync();
}

// The matched clusters of a window whose defects mark_clusters has listed in lp[0 .. n_list): per cluster the pairs of the dynamic
// program, then `flip(e, u, v)` for every edge of the pairs' paths, by the lane that walks the path; the return value is this
// lane's XOR of what flip returned.  *longest = max(*longest, this lane's longest walk); true in the lanes that met a walk that
// does not end, a broken parent edge or a cluster without a pairing.
template <class F>
__device__ __forceinline__ uint64_t match_window(const Args &a, const WinDesc &d, const Win &w, const ufk::State &st, uint16_t *mpair, int lane,
                                                 int n_list, uint32_t *longest, bool *bad, F flip) {
  using bitrows::wsync;
  const size_t N = (size_t)d.n_nodes;
  const uint32_t *dist = a.mdist + d.off_table;
  const uint16_t *parent = a.mparent + d.off_table;
  uint64_t flips = 0;
  ufk::matched_clusters(st, lane, n_list, [&](int from, int r) {
    const int m = ufk::cluster_defects(st, lane, from, n_list, r, a.match_k);
    ufk::cluster_distances(st, lane, m, dist, N);
    wsync();
    ufk::pair_programs<false>(st, lane, m);
    if (lane == 0) {  // the winners, from the full set down: S loses one or two defects per step, so at most m <= K pairs
      uint32_t n = 0;
      for (int S = (1 << m) - 1; S;) {
        const int i = __builtin_ctz(S), R = S & (S - 1), via = st.mch[S];
        if (via == ufk::kViaNone) {  // (no pairing: a cluster is connected and holds an even number of defects or node 0)
          n = ~0u;
          break;
        }
        mpair[2 * n] = st.mcl[i];
        mpair[2 * n + 1] = via == ufk::kViaBoundary ? (uint16_t)0 : st.mcl[via];  // (via is a defect of R: below m)
        ++n;
        S = via == ufk::kViaBoundary ? R : R ^ (1 << via);
      }
      st.misc[2] = n;
    }
    wsync();
    const uint32_t n_pairs = st.misc[2];
    if (n_pairs == ~0u) *bad = true;
    else
      for (uint32_t p = (uint32_t)lane; p < n_pairs; p += 64) {
        const int src = mpair[2 * p];
        const size_t row = (size_t)src * N;
        int v = mpair[2 * p + 1], steps = 0;
        for (; v != src && steps < d.n_nodes; ++steps) {  // (a parent lies strictly nearer: at most n_nodes - 1 steps)
          const uint32_t e = parent[row + (size_t)v];
          if (e >= (uint32_t)d.n_edges) break;  // (kNoEdge)
          const uint32_t uv = w.edge_uv[e];
          const int eu = (int)(uv & 0xFFFFu), ev = (int)(uv >> 16);
          if (eu != v && ev != v) break;
          flips ^= flip((int)e, eu, ev);
          v = eu == v ? ev : eu;
        }
        if (v != src) *bad = true;
        *longest = max(*longest, (uint32_t)steps);
      }
    wsync();  // (the next cluster overwrites the arrays)
  });
  return flips;
}

// one kept row with a defect, by the whole wave, window after window: the prediction (0 for a miss); *missed, *rounds (the most
// of a window) and *windows (those decoded) are wave-uniform, and so are, with Soft, soft[0 .. 2]: the full edges summed and the
// largest cluster maximised over the decoded windows, a missing one included, and the committed flips (0 for a miss); with
// Match, soft[0 .. 1]: the clusters matched and peeled, summed over the decoded windows (0 for a miss); soft[2], the longest path
// a lane walked, is per lane
template <bool Weighted, bool Heralds, bool Soft = false, bool Match = false>
__device__ __forceinline__ uint64_t decode_row(const Args &a, const ufk::State &st, uint32_t *carry, uint32_t *pred, uint16_t *mpair,
                                               const uint8_t *row, int lane, bool *missed, int *rounds, int *windows, uint32_t *soft = nullptr) {
  using bitrows::wsync;
  for (int i = lane; i < a.carry_words; i += 64) carry[i] = 0;
  if (lane < 2) pred[lane] = 0;
  wsync();
  *missed = false, *rounds = 0, *windows = 0;
  if constexpr (Soft) soft[0] = soft[1] = soft[2] = 0;
  if constexpr (Match) soft[0] = soft[1] = soft[2] = 0;
  const int P = 32 * a.carry_words;
  for (int k = 0; k < a.n_windows; ++k) {
    const WinDesc d = a.desc[k];
    const int N = d.n_nodes;
    bool any = false;
    for (int v = lane; v < N; v += 64) {
      uint32_t bit = 0;
      if (v) {
        int c = d.lo + v - 1;
        const int slot = c & (P - 1);
        if constexpr (Heralds) c = a.node_det[c];
        uint32_t byte = row[c >> 3];
        if (a.xr) byte ^= a.xr[c >> 3];
        bit = ((byte >> (c & 7)) ^ (carry[slot >> 5] >> (slot & 31))) & 1u;
      }
      st.s[v] = (uint8_t)bit;
      st.label[v] = (uint16_t)v;
      any |= bit != 0;
    }
    if (__builtin_amdgcn_ballot_w64(any)) {  // (a window without a defect is skipped)
      Win w;
      w.n_nodes = N, w.n_edges = d.n_edges, w.w32 = d.w32, w.w_cnt = d.w_cnt;
      w.edge_uv = a.edge_uv + d.off_edge;
      w.edge_obs = a.edge_obs + d.off_edge;
      w.cap = Weighted ? a.cap + d.off_edge : nullptr;
      w.adj_ptr = a.adj_ptr + d.off_ptr;
      w.adj_edge = a.adj_edge + d.off_adj;
      const uint32_t *committed = a.commit_bits + d.off_commit;
      ufk::clear_edges<Weighted>(w, st, lane);
      if constexpr (Heralds) pregrow_window(a, d, st, row, lane);
      int r;
      const bool miss = ufk::grow<Weighted>(w, st, lane, &r);
      *rounds = max(*rounds, r);
      ++*windows;
      if constexpr (Soft) {  // (lp[] is free between grow() and forest(); the wsync() this ends on comes before forest() writes it)
        uint32_t grown[2];
        ufk::soft_of_growth(w, st, lane, grown);
        soft[0] += grown[0], soft[1] = max(soft[1], grown[1]);
      }
      if (miss) {
        *missed = true;
        if constexpr (Soft) soft[2] = 0;
        if constexpr (Match) soft[0] = soft[1] = 0;
        return 0;
      }
      uint32_t flipped = 0;  // (Soft) committed, by this lane
      const auto flip = [&](int e, int u, int v) -> uint64_t {  // a local flip: what it does when its edge is committed
        if (!((committed[e >> 5] >> (e & 31)) & 1u)) return 0;
        if constexpr (Soft) ++flipped;
        if (u) {
          const int slot = (d.lo + u - 1) & (P - 1);
          atomicXor(&carry[slot >> 5], 1u << (slot & 31));
        }
        const int slot = (d.lo + v - 1) & (P - 1);
        atomicXor(&carry[slot >> 5], 1u << (slot & 31));
        return w.edge_obs[e];
      };
      uint64_t flips;
      if constexpr (Match) {
        int n_list;
        uint32_t counts[2];
        ufk::mark_clusters(w, a.match_k, st, lane, &n_list, counts);
        bool bad = false;
        flips = match_window(a, d, w, st, mpair, lane, n_list, &soft[2], &bad, flip);
        if (__builtin_amdgcn_ballot_w64(bad)) {
          *missed = true;
          soft[0] = soft[1] = 0;
          return 0;
        }
        soft[0] += counts[0], soft[1] += counts[1];
        if (counts[1]) {  // a flip counts when its edge, and so its child node, lies in a peeled cluster
          ufk::forest(w, st, lane);
          flips ^= ufk::peel(w, st, lane, [&](int e, int u, int v) -> uint64_t { return st.par[st.label[u]] == 2 ? flip(e, u, v) : 0ull; });
        }
      } else {
        ufk::forest(w, st, lane);
        flips = ufk::peel(w, st, lane, flip);
      }
      if constexpr (Soft) soft[2] += ufk::wave_sum(flipped);
      ufk::fold_flips(pred, flips);
    }
    wsync();
    if (!d.last) {  // the window advances: the slots of its commit region are free for the columns that come in
      const int s = d.lo & (P - 1), e = s + a.commit;
      for (int i = lane; i < a.carry_words; i += 64) {
        const uint32_t gone = bits_between(i, s, e) | bits_between(i, 0, e - P);
        if (gone) carry[i] &= ~gone;
      }
      wsync();
    }
  }
  return (uint64_t)pred[0] | (uint64_t)pred[1] << 32;
}

template <bool Weighted, bool Heralds, bool Soft = false, bool Match = false>
__global__ void __launch_bounds__(64 * ufk::kMaxWaves) k_ufw(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  uint32_t *stat = reinterpret_cast<uint32_t *>(lds_raw);  // kept, wrong, missed; with Soft: the kept rows of bin 0
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *base = lds_raw + 16 + (size_t)wave * a.shot_bytes;
  const ufk::State st = Match ? ufk::match_state_at(a, base) : ufk::state_at(a, base);
  uint32_t *carry = reinterpret_cast<uint32_t *>(base + a.off_carry), *predw = reinterpret_cast<uint32_t *>(base + a.off_pred);
  uint16_t *mpair = reinterpret_cast<uint16_t *>(base + a.off_mpair);  // (Match) the pairs a cluster chose
  if (threadIdx.x < 4) stat[threadIdx.x] = 0;
  __syncthreads();
  uint32_t kept_acc = 0, wrong_acc = 0, miss_acc = 0, decoded_acc = 0;  // wave-uniform
  unsigned long long windows_acc = 0;
  int most_rounds = 0;
  ufk::SoftBins bins;  // (Soft) the wave's rows of bin 0
  uint32_t matched_acc = 0, peeled_acc = 0, longest = 0;  // (Match) wave-uniform: the clusters matched and peeled; per lane: its longest path
  const long long tiles = (a.n + 63) >> 6;
  for (long long t = (long long)blockIdx.x * a.waves + wave; t < tiles; t += (long long)gridDim.x * a.waves) {
    const long long r = (t << 6) + lane;
    const bool valid = r < a.n;
    const uint8_t *row = a.rows + (valid ? r : 0) * a.rb;
    uint64_t fail, defects;
    ufk::scan_row(a, row, valid, Heralds ? a.dmask : nullptr, a.nd, &fail, &defects);
    const bool kept = valid && fail == 0;
    const uint64_t obs = kept ? bitrows::row_obs(a, row) : 0;
    uint64_t pred = 0;
    bool missed = false;
    uint32_t mine[4] = {0, 0, 0, 0};  // (Soft) this lane's row: rounds, full edges, largest cluster, correction weight
    uint64_t work = __builtin_amdgcn_ballot_w64(kept && defects != 0);
    while (work) {
      const int src = __builtin_ctzll(work);
      work &= work - 1;
      bool m;
      int rounds, windows;
      uint32_t soft[3];
      const uint64_t p =
          decode_row<Weighted, Heralds, Soft, Match>(a, st, carry, predw, mpair, a.rows + ((t << 6) + src) * a.rb, lane, &m, &rounds, &windows, soft);
      if (lane == src) pred = p, missed = m;
      if constexpr (Match) matched_acc += soft[0], peeled_acc += soft[1], longest = max(longest, soft[2]);
      if constexpr (Soft)
        if (lane == src) mine[0] = (uint32_t)rounds, mine[1] = soft[0], mine[2] = soft[1], mine[3] = soft[2];
      most_rounds = max(most_rounds, rounds);
      windows_acc += (unsigned)windows;
      ++decoded_acc;
    }
    kept_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept));
    wrong_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && pred != obs));
    miss_acc += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(kept && missed));
    if (a.pred && valid) a.pred[r] = pred;  // (0 for a row that is not kept, and for a miss)
    if constexpr (Soft) {
      bins.tile(a, a.metric == 0 ? mine[0] : a.metric == 1 ? mine[1] : a.metric == 2 ? mine[2] : mine[3], kept, kept && pred != obs, lane);
      if (a.soft && valid) reinterpret_cast<uint4 *>(a.soft)[r] = make_uint4(mine[0], mine[1], mine[2], mine[3]);  // (zeros for a row that is not kept)
    }
  }
  if constexpr (Match) longest = ufk::wave_max(longest);
  if (lane == 0) {
    if (kept_acc) atomicAdd(&stat[0], kept_acc);
    if (wrong_acc) atomicAdd(&stat[1], wrong_acc);
    if (miss_acc) atomicAdd(&stat[2], miss_acc);
    if (most_rounds) atomicMax(&a.stats[0], (unsigned long long)most_rounds);
    if (decoded_acc) atomicAdd(&a.stats[1], (unsigned long long)decoded_acc);
    if (windows_acc) atomicAdd(&a.stats[2], windows_acc);
    if constexpr (Match) {
      if (matched_acc) atomicAdd(&a.stats[3], (unsigned long long)matched_acc);
      if (peeled_acc) atomicAdd(&a.stats[4], (unsigned long long)peeled_acc);
      if (longest) atomicMax(&a.stats[5], (unsigned long long)longest);
    }
    if constexpr (Soft) bins.wave_done(a, stat);
  }
  __syncthreads();
  if (threadIdx.x < 3 && stat[threadIdx.x]) atomicAdd(&a.dec[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
  if constexpr (Soft) ufk::SoftBins::block_done(a, stat);
}

}  // namespace ufwk
