// tsim_ufw.hip - sliding-window union-find decoding over bit-packed device rows (tsim_ufw_*): a handle of its own, bound to
// one device.  tsim_ufw_create builds the windows of the global decoding graph on the host, by the rule in the module
// docstring of tsim_amd/decode.py ("Sliding-window decoding of long runs") - a second statement of that construction,
// independent of the numpy one - and holds their tables; the kernel is csrc/tsim_ufw.hip.h.  tsim_ufw_create_heralds takes a
// graph with heralds and builds, with the windows, every window's herald lists ("Sliding windows with heralds" there).
// tsim_ufw_create_matching computes the windows' local match weights beside the caps and builds one match table per DISTINCT
// window on the device ("Cluster matching in windows" there; the table kernel is csrc/tsim_uf_match.hip.h, started through
// ufh::launch_match_table).
#include "tsim_uf_host.hip.h"
#include "tsim_ufw.hip.h"

#include <new>
#include <string>
#include <unordered_map>
#include <utility>

namespace {
constexpr int64_t kMaxTable = 0x7FFFFFFF;  // entries of a concatenated table: int32 offsets
constexpr int64_t kMaxMatchBytes = 1ll << 30;  // of the distinct windows' match tables together, at 6 bytes per pair of nodes

struct Tables {
  std::vector<ufwk::WinDesc> desc;
  std::vector<uint32_t> uv, adj_ptr, commit;
  std::vector<uint64_t> obs;
  std::vector<uint8_t> cap;
  std::vector<uint16_t> adj;
  std::vector<uint16_t> w;  // cluster matching: the local match weights, concatenated like the caps
  int max_nodes = 0, max_edges = 0, max_w32 = 1, max_w_cnt = 0;
  // heralds: per window the heralds with a local edge there, one CSR over the concatenation, the local edges
  std::vector<int32_t> win_herald;
  std::vector<uint32_t> win_her_ptr;
  std::vector<uint16_t> win_her_edges;
};

// the heralds that list a global edge: the transpose of the heralds' CSR (built once, read per window)
struct EdgeHeralds {
  std::vector<int64_t> ptr;  // [n_edges + 1]
  std::vector<int32_t> her;
};
}  // namespace

struct tsim_ufw {
  int device = -1;
  ufwk::Args a{};  // the windows' part of the kernel's arguments
  int grid = 1;
  int n_nodes = 0, n_edges = 0, max_nodes = 0, max_edges = 0, max_cap = 0;
  int64_t launches = 0;
  int n_heralds = 0;
  // cluster matching (a.match_k != 0): the windows' descriptors on the host, the distinct tables and their pairs of nodes
  std::vector<ufwk::WinDesc> desc;
  uint32_t *mdist = nullptr;
  uint16_t *mparent = nullptr;
  int64_t distinct = 0, table_pairs = 0;
  tsimh::Uploads up;  // the tables a points to
};

// The windows of the graph (checked by the caller: u < v inside the nodes, pairs strictly ascending) with `commit` = C and
// `window` = W columns.  0, or an error code after tsim_fail.  `eh` (NULL: a graph without heralds): the heralds of every global
// edge, for the windows' herald lists - per window and herald the distinct local edges loc_k(e) of the herald's edges that are
// present there ("Sliding windows with heralds" in the docstring).  `match_w` (NULL: no cluster matching): the global match
// weights, for the local ones - the least among the global edges that land on a local edge, the rule of the caps.
static int build_windows(const tsim_uf_desc *g, const uint8_t *edge_cap, const uint16_t *match_w, int64_t C, int64_t W, const EdgeHeralds *eh,
                         Tables *t) {
  const int64_t nd = (int64_t)g->n_nodes - 1, E = g->n_edges;
  const int64_t K = nd <= W ? 1 : (nd - W + C - 1) / C + 1;  // the smallest K >= 1 with (K - 1) C + W >= nd
  auto hi_of = [&](int64_t k) { return k == K - 1 ? nd : k * C + W; };
  auto cap_of = [&](int64_t e) { return edge_cap ? edge_cap[e] : (uint8_t)2; };
  auto w_of = [&](int64_t e) { return match_w ? match_w[e] : (uint16_t)1; };
  // validity: the column a of an edge's lower end is committed in window min(a / C, K - 1), which must hold its upper end
  std::vector<int32_t> outer, inner;  // the boundary edges, ascending in their column; the others, ascending in the lower column
  for (int64_t e = 0; e < E; ++e) {
    if (g->edge_u[e] == 0) {
      outer.push_back((int32_t)e);
      continue;
    }
    inner.push_back((int32_t)e);
    const int64_t a = g->edge_u[e] - 1, b = g->edge_v[e] - 1, k = std::min(a / C, K - 1);
    if (b >= hi_of(k))
      return tsim_fail(TSIM_EINVAL,
                       "edge %lld = (%d, %d): column %lld is committed in window %lld, which ends before column %lld (at %lld): the buffer "
                       "window - commit = %lld is too small",
                       (long long)e, g->edge_u[e], g->edge_v[e], (long long)a, (long long)k, (long long)b, (long long)hi_of(k), (long long)(W - C));
  }
  if (std::min(W, nd) + 1 > ufh::kMaxIndex)
    return tsim_fail(TSIM_ENOTSUP, "a window of %lld nodes (at most %d: indices are uint16)", (long long)(std::min(W, nd) + 1), ufh::kMaxIndex);
  const size_t n_max = (size_t)std::min(W, nd) + 1;
  std::vector<uint8_t> b_cap(n_max), b_kind(n_max);  // per local node x the pair (0, x): its cap; 0 none, 1 virtual only, 2 real
  std::vector<int32_t> b_edge(n_max);                // the real boundary edge
  std::vector<uint16_t> b_w(match_w ? n_max : 0);    // (cluster matching) per local node x the weight of the pair (0, x)
  std::vector<int32_t> kept;                         // the window's edges between two of its columns
  std::vector<uint32_t> lu, lv, at;
  std::vector<int32_t> b_index(eh ? n_max : 0);      // (heralds) per local node x the local edge that is the pair (0, x)
  std::vector<std::pair<int32_t, int32_t>> listed;   // (heralds) (herald, local edge) of the window
  size_t po = 0, pi = 0;
  for (int64_t k = 0; k < K; ++k) {
    const int64_t lo = k * C, hi = hi_of(k);
    const int N = (int)(hi - lo + 1);
    const bool last = k == K - 1;
    std::fill(b_kind.begin(), b_kind.begin() + N, 0);
    std::fill(b_cap.begin(), b_cap.begin() + N, 255);
    if (match_w) std::fill(b_w.begin(), b_w.begin() + N, 65535);
    while (po < outer.size() && g->edge_v[outer[po]] - 1 < lo) ++po;
    for (size_t i = po; i < outer.size() && g->edge_v[outer[i]] - 1 < hi; ++i) {
      const int32_t e = outer[i];
      const int x = (int)(g->edge_v[e] - lo);
      b_kind[x] = 2, b_edge[x] = e, b_cap[x] = cap_of(e);
      if (match_w) b_w[x] = w_of(e);
    }
    kept.clear();
    while (pi < inner.size() && g->edge_u[inner[pi]] - 1 < lo) ++pi;
    for (size_t i = pi; i < inner.size() && g->edge_u[inner[i]] - 1 < hi; ++i) {
      const int32_t e = inner[i];
      if (g->edge_v[e] - 1 < hi) {
        kept.push_back(e);
        continue;
      }
      const int x = (int)(g->edge_u[e] - lo);  // to the open future boundary
      b_kind[x] = std::max<uint8_t>(b_kind[x], 1), b_cap[x] = std::min(b_cap[x], cap_of(e));
      if (match_w) b_w[x] = std::min(b_w[x], w_of(e));
    }
    lu.clear(), lv.clear();
    ufwk::WinDesc d{};
    d.lo = (int32_t)lo, d.n_nodes = N, d.last = last;
    d.off_edge = (int32_t)t->uv.size(), d.off_ptr = (int32_t)t->adj_ptr.size(), d.off_adj = (int32_t)t->adj.size();
    d.off_commit = (int32_t)t->commit.size();
    for (int x = 1; x < N; ++x)
      if (b_kind[x]) {
        if (eh) b_index[x] = (int32_t)lu.size();
        lu.push_back(0), lv.push_back((uint32_t)x);
        t->obs.push_back(b_kind[x] == 2 ? g->edge_obs[b_edge[x]] : 0);
        t->cap.push_back(b_cap[x]);
        if (match_w) t->w.push_back(b_w[x]);
      }
    for (int32_t e : kept) {
      lu.push_back((uint32_t)(g->edge_u[e] - lo)), lv.push_back((uint32_t)(g->edge_v[e] - lo));
      t->obs.push_back(g->edge_obs[e]);
      t->cap.push_back(cap_of(e));
      if (match_w) t->w.push_back(w_of(e));
    }
    const size_t n_e = lu.size();
    if (n_e > (size_t)ufh::kMaxIndex)
      return tsim_fail(TSIM_ENOTSUP, "window %lld has %zu edges (at most %d: indices are uint16)", (long long)k, n_e, ufh::kMaxIndex);
    d.n_edges = (int32_t)n_e;
    if (eh) {  // the herald lists: every global edge that is present, under its local edge, for each herald that lists it
      listed.clear();
      auto list = [&](int32_t e, int32_t local) {
        for (int64_t q = eh->ptr[e]; q < eh->ptr[e + 1]; ++q) listed.emplace_back(eh->her[q], local);
      };
      for (size_t i = po; i < outer.size() && g->edge_v[outer[i]] - 1 < hi; ++i) list(outer[i], b_index[g->edge_v[outer[i]] - lo]);
      int32_t next_kept = (int32_t)(n_e - kept.size());  // (the kept edges follow the boundary pairs, in their order)
      for (size_t i = pi; i < inner.size() && g->edge_u[inner[i]] - 1 < hi; ++i) {
        const int32_t e = inner[i];
        if (g->edge_v[e] - 1 < hi) list(e, next_kept++);
        else list(e, b_index[g->edge_u[e] - lo]);  // as the open future boundary of its lower end
      }
      std::sort(listed.begin(), listed.end());
      listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
      d.off_her = (int32_t)t->win_herald.size();
      for (size_t i = 0; i < listed.size(); ++i) {
        if (listed[i].second < 0 || (size_t)listed[i].second >= n_e)
          return tsim_fail(TSIM_EINVAL, "window %lld: a herald's local edge %d leaves its %zu edges", (long long)k, listed[i].second, n_e);
        if (i == 0 || listed[i].first != listed[i - 1].first) {
          t->win_herald.push_back(listed[i].first);
          t->win_her_ptr.push_back((uint32_t)t->win_her_edges.size());
        }
        t->win_her_edges.push_back((uint16_t)listed[i].second);
      }
      d.n_her = (int32_t)(t->win_herald.size() - (size_t)d.off_her);
      if ((int64_t)t->win_herald.size() > kMaxTable || (int64_t)t->win_her_edges.size() > kMaxTable)
        return tsim_fail(TSIM_ENOTSUP, "the windows' herald lists pass 2^31 entries at window %lld of %lld", (long long)k, (long long)K);
    }
    d.w32 = std::max(1, ((int)n_e + 31) / 32);
    d.w_cnt = edge_cap ? std::max(1, ((int)n_e + 7) / 8) : 0;
    t->commit.resize(t->commit.size() + d.w32, 0);
    at.assign((size_t)N + 1, 0);
    for (size_t e = 0; e < n_e; ++e) {
      if (!(lu[e] < lv[e] && lv[e] < (uint32_t)N)) return tsim_fail(TSIM_EINVAL, "window %lld: local edge %zu leaves its nodes", (long long)k, e);
      t->uv.push_back(lu[e] | lv[e] << 16);
      if (last || lv[e] <= C || (lu[e] >= 1 && lu[e] <= C)) t->commit[d.off_commit + (e >> 5)] |= 1u << (e & 31);
      ++at[lu[e] + 1], ++at[lv[e] + 1];
    }
    for (int v = 0; v < N; ++v) at[v + 1] += at[v];
    t->adj_ptr.insert(t->adj_ptr.end(), at.begin(), at.end());
    t->adj.resize(t->adj.size() + 2 * n_e);
    for (size_t e = 0; e < n_e; ++e) {
      t->adj[d.off_adj + at[lu[e]]++] = (uint16_t)e;
      t->adj[d.off_adj + at[lv[e]]++] = (uint16_t)e;
    }
    t->desc.push_back(d);
    t->max_nodes = std::max(t->max_nodes, N), t->max_edges = std::max(t->max_edges, (int)n_e);
    t->max_w32 = std::max(t->max_w32, d.w32), t->max_w_cnt = std::max(t->max_w_cnt, d.w_cnt);
    if ((int64_t)t->adj.size() > kMaxTable || (int64_t)t->adj_ptr.size() > kMaxTable)
      return tsim_fail(TSIM_ENOTSUP, "the windows' tables pass 2^31 entries at window %lld of %lld", (long long)k, (long long)K);
  }
  if (eh) t->win_her_ptr.push_back((uint32_t)t->win_her_edges.size());  // (one CSR over all windows: the end of the last list)
  return TSIM_OK;
}

// every create call; match_w != NULL: tsim_ufw_create_matching, with max_defects
static int ufw_create(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, int32_t commit, int32_t window, const tsim_uf_heralds *her,
                      const uint16_t *match_w, int32_t max_defects, tsim_ufw **out);

extern "C" int tsim_ufw_create(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, int32_t commit, int32_t window,
                               tsim_ufw **out) {
  return ufw_create(device, desc, edge_cap, commit, window, nullptr, nullptr, 0, out);
}

extern "C" int tsim_ufw_create_heralds(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, int32_t commit, int32_t window,
                                       const tsim_uf_heralds *her, tsim_ufw **out) {
  return ufw_create(device, desc, edge_cap, commit, window, her, nullptr, 0, out);
}

extern "C" int tsim_ufw_create_matching(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, const uint16_t *match_w,
                                        int32_t max_defects, int32_t commit, int32_t window, tsim_ufw **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!match_w) return tsim_fail(TSIM_EINVAL, "match_w is NULL");
  if (max_defects < 1 || max_defects > ufk::kMaxMatchDefects)
    return tsim_fail(TSIM_EINVAL, "max_defects = %d (1 .. %d)", max_defects, ufk::kMaxMatchDefects);
  return ufw_create(device, desc, edge_cap, commit, window, nullptr, match_w, max_defects, out);
}

// The distinct windows of t, for their match tables: windows whose local arrays - nodes, edge_uv, edge_obs, weights, adjacency
// and the commit bitmap - are byte-identical share one table.  Sets every window's off_table, in pairs of nodes; first[i]: the
// window that table i is built from; *pairs: the pairs of nodes of all tables together.
static void share_tables(Tables *t, std::vector<int> *first, int64_t *pairs) {
  std::unordered_map<std::string, long long> seen;
  auto bytes = [](std::string *key, const void *p, size_t n) { key->append(static_cast<const char *>(p), n); };
  *pairs = 0;
  for (size_t k = 0; k < t->desc.size(); ++k) {
    ufwk::WinDesc &d = t->desc[k];
    const size_t N = (size_t)d.n_nodes, E = (size_t)d.n_edges;
    std::string key;
    bytes(&key, &d.n_nodes, sizeof d.n_nodes), bytes(&key, &d.n_edges, sizeof d.n_edges);
    bytes(&key, t->uv.data() + d.off_edge, 4 * E), bytes(&key, t->obs.data() + d.off_edge, 8 * E), bytes(&key, t->w.data() + d.off_edge, 2 * E);
    bytes(&key, t->adj_ptr.data() + d.off_ptr, 4 * (N + 1)), bytes(&key, t->adj.data() + d.off_adj, 2 * 2 * E);
    bytes(&key, t->commit.data() + d.off_commit, 4 * (size_t)d.w32);
    const auto at = seen.emplace(std::move(key), (long long)*pairs);
    d.off_table = at.first->second;
    if (at.second) first->push_back((int)k), *pairs += (int64_t)(N * N);
  }
}

static int ufw_create(int32_t device, const tsim_uf_desc *desc, const uint8_t *edge_cap, int32_t commit, int32_t window, const tsim_uf_heralds *her,
                      const uint16_t *match_w, int32_t max_defects, tsim_ufw **out) {
  if (!out) return tsim_fail(TSIM_EINVAL, "out is NULL");
  *out = nullptr;
  if (!desc) return tsim_fail(TSIM_EINVAL, "desc is NULL");
  const int N = desc->n_nodes, E = desc->n_edges;
  if (N < 2) return tsim_fail(TSIM_EINVAL, "n_nodes = %d (the boundary and at least one detector)", N);
  if (E < 0) return tsim_fail(TSIM_EINVAL, "n_edges = %d", E);
  if (commit < 1 || window <= commit) return tsim_fail(TSIM_EINVAL, "commit = %d, window = %d: 1 <= commit < window expected", commit, window);
  long long n_det = 0;
  int max_cap = 0;
  if (const int rc = ufh::check_graph(desc, edge_cap, her, &n_det, &max_cap)) return rc;
  if (match_w)
    for (int e = 0; e < E; ++e)
      if (match_w[e] < 1) return tsim_fail(TSIM_EINVAL, "edge %d has match weight 0 (1 .. 65535)", e);
  const int H = her ? her->n_heralds : 0, mask_bytes = (desc->n_cols + 7) / 8;
  std::vector<uint8_t> dmask;
  EdgeHeralds eh;
  if (her) {
    dmask.assign((size_t)mask_bytes, 0);
    std::vector<uint8_t> hmask((size_t)mask_bytes, 0);
    if (const int rc = ufh::check_heralds(desc, her, n_det, dmask.data(), hmask.data(), nullptr)) return rc;
    const int n_listed = her->herald_ptr[H];
    eh.ptr.assign((size_t)E + 1, 0);
    for (int k = 0; k < n_listed; ++k) ++eh.ptr[her->herald_edges[k] + 1];
    for (int e = 0; e < E; ++e) eh.ptr[e + 1] += eh.ptr[e];
    eh.her.resize((size_t)n_listed);
    std::vector<int64_t> at(eh.ptr.begin(), eh.ptr.end() - 1);
    for (int i = 0; i < H; ++i)
      for (int k = her->herald_ptr[i]; k < her->herald_ptr[i + 1]; ++k) eh.her[at[her->herald_edges[k]]++] = i;
  }
  Tables t;
  if (const int rc = build_windows(desc, edge_cap, match_w, commit, window, her ? &eh : nullptr, &t)) return rc;
  std::vector<int> first;  // cluster matching: the window every distinct table is built from
  int64_t table_pairs = 0;
  if (match_w) {
    if (t.max_nodes > ufk::kMaxMatchNodes)
      return tsim_fail(TSIM_ENOTSUP, "a window of %d nodes (a match table has at most %d: 6 bytes per pair of nodes)", t.max_nodes,
                       ufk::kMaxMatchNodes);
    share_tables(&t, &first, &table_pairs);
    if (6 * table_pairs > kMaxMatchBytes)
      return tsim_fail(TSIM_ENOTSUP, "the match tables of %zu distinct windows take %lld bytes (at most %lld)", first.size(),
                       (long long)(6 * table_pairs), (long long)kMaxMatchBytes);
  }
  // the state of a wave: that of the largest window (with cluster matching: and the dynamic program's), the carry bitmap, the
  // prediction, the pairs a cluster chose
  ufk::Args lay{};
  lay.n_nodes = t.max_nodes, lay.w32 = t.max_w32, lay.w_cnt = t.max_w_cnt;
  lay.match_k = match_w ? max_defects : 0;
  long long shot = ufk::layout(&lay);
  int carry_words = 1;
  while (32ll * carry_words < std::min<long long>(window, N - 1)) carry_words *= 2;
  ufwk::Args a{};
  a.off_lp = lay.off_lp, a.off_s = lay.off_s, a.off_par = lay.off_par, a.off_half = lay.off_half, a.off_full = lay.off_full;
  a.off_wlist = lay.off_wlist, a.off_misc = lay.off_misc;
  a.off_carry = (int)shot, shot += ufk::a16(4ll * carry_words);
  a.off_pred = (int)shot, shot += 16;
  if (match_w) {
    a.match_k = max_defects;
    a.off_mcost = lay.off_mcost, a.off_mch = lay.off_mch, a.off_mcl = lay.off_mcl, a.off_mpd = lay.off_mpd;
    a.off_mpair = (int)shot, shot += ufk::a16(4ll * max_defects);
  }
  if (16 + shot > ufk::kLdsBlock)
    return tsim_fail(TSIM_ENOTSUP, "one shot's state takes %lld bytes of LDS (windows of up to %d nodes, %d edges%s), a block has %d", shot,
                     t.max_nodes, t.max_edges, match_w ? ", the dynamic program of max_defects" : "", ufk::kLdsBlock - 16);
  a.shot_bytes = (int)shot;
  a.carry_words = carry_words;
  a.n_windows = (int)t.desc.size();
  a.commit = commit;
  a.nd = N - 1;
  a.n_cols = desc->n_cols;
  int per_cu = 1;
  ufh::choose_waves(shot, &a.waves, &per_cu);
  if (t.uv.empty()) t.uv.push_back(0), t.obs.push_back(0), t.cap.push_back(1);
  if (t.adj.empty()) t.adj.push_back(0);
  int cus = 0;
  if (const int rc = tsimh::open_device(device, &cus)) return rc;
  tsim_ufw *h = new (std::nothrow) tsim_ufw();
  if (!h) return tsim_fail(TSIM_ENOMEM, "out of host memory");
  h->device = device;
  h->grid = std::max(1, cus) * per_cu;
  h->n_nodes = N, h->n_edges = E, h->max_nodes = t.max_nodes, h->max_edges = t.max_edges, h->max_cap = max_cap;
  tsimh::Uploads &up = h->up;
  a.desc = up.put(t.desc);
  a.edge_uv = up.put(t.uv);
  a.edge_obs = reinterpret_cast<const unsigned long long *>(up.put(t.obs));
  if (edge_cap) a.cap = up.put(t.cap);
  a.adj_ptr = up.put(t.adj_ptr);
  a.adj_edge = up.put(t.adj);
  a.commit_bits = up.put(t.commit);
  if (her) {
    h->n_heralds = H;
    std::vector<int32_t> herald_det(1, 0);  // (never an empty buffer)
    if (H) herald_det.assign(her->herald_det, her->herald_det + H);
    if (t.win_herald.empty()) t.win_herald.push_back(0);
    if (t.win_her_edges.empty()) t.win_her_edges.push_back(0);
    a.node_det = up.put(her->node_det, (size_t)(N - 1));
    a.herald_det = up.put(herald_det);
    a.dmask = up.put(dmask);
    a.win_herald = up.put(t.win_herald);
    a.win_her_ptr = up.put(t.win_her_ptr);
    a.win_her_edges = up.put(t.win_her_edges);
  }
  const uint64_t zero[6] = {0, 0, 0, 0, 0, 0};
  a.stats = reinterpret_cast<unsigned long long *>(up.put(zero, match_w ? 6 : 4));
  if (match_w) {  // the match tables, built here once: one launch per distinct window, on its slices of the concatenated tables
    if (t.w.empty()) t.w.push_back(1);
    const uint16_t *d_w = up.put(t.w);
    const size_t pairs = (size_t)std::max<int64_t>(1, table_pairs);
    h->mdist = static_cast<uint32_t *>(up.room(pairs * sizeof(uint32_t)));
    h->mparent = static_cast<uint16_t *>(up.room(pairs * sizeof(uint16_t)));
    up.bytes += 6 * table_pairs;
    h->distinct = (int64_t)first.size(), h->table_pairs = table_pairs;
    for (size_t i = 0; i < first.size() && up.err == hipSuccess; ++i) {
      const ufwk::WinDesc &d = t.desc[first[i]];
      up.err = ufh::launch_match_table(d.n_nodes, a.edge_uv + d.off_edge, a.edge_obs + d.off_edge, d_w + d.off_edge, a.adj_ptr + d.off_ptr,
                                       a.adj_edge + d.off_adj, h->mdist + d.off_table, nullptr, h->mparent + d.off_table);
    }
    a.mdist = h->mdist, a.mparent = h->mparent;
    h->desc = t.desc;
  }
  if (up.err == hipSuccess) up.err = hipDeviceSynchronize();
  if (up.err != hipSuccess) {
    const hipError_t e = up.err;
    tsim_ufw_destroy(h);
    return tsim_fail(e == hipErrorOutOfMemory ? TSIM_ENOMEM : TSIM_EHIP, "%zu windows of a graph of %d nodes, %d edges: %s", t.desc.size(), N, E,
                     hipGetErrorString(e));
  }
  h->a = a;
  *out = h;
  return TSIM_OK;
}

extern "C" void tsim_ufw_destroy(tsim_ufw *h) {
  if (!h) return;
  h->up.release(h->device);
  delete h;
}

extern "C" int tsim_ufw_info(tsim_ufw *h, int64_t out[16]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());  // (the statistics live on the device: every decode so far is waited for)
  uint64_t st[3];
  HIP_TRY(hipMemcpy(st, h->a.stats, sizeof st, hipMemcpyDeviceToHost));
  std::fill(out, out + 16, 0);
  out[0] = h->n_nodes;
  out[1] = h->n_edges;
  out[2] = h->a.n_windows;
  out[3] = h->max_nodes;
  out[4] = h->max_edges;
  out[5] = h->a.shot_bytes;
  out[6] = h->a.waves;
  out[7] = h->launches;
  out[8] = (int64_t)st[0];
  out[9] = h->up.bytes;
  out[10] = (int64_t)st[1];
  out[11] = (int64_t)st[2];
  out[12] = h->a.n_cols;
  out[13] = h->grid;
  out[14] = h->max_cap;
  out[15] = h->n_heralds;
  return TSIM_OK;
}

extern "C" int tsim_ufw_match_info(tsim_ufw *h, int64_t out[8]) {
  if (!h || !out) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!h->a.match_k) return tsim_fail(TSIM_EINVAL, "the handle matches no clusters (tsim_ufw_create_matching makes one)");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  uint64_t st[3];
  HIP_TRY(hipMemcpy(st, h->a.stats + 3, sizeof st, hipMemcpyDeviceToHost));
  std::fill(out, out + 8, 0);
  out[0] = h->a.match_k;
  out[1] = h->distinct;
  out[2] = 6 * h->table_pairs;
  out[3] = (int64_t)st[0];
  out[4] = (int64_t)st[1];
  out[5] = (int64_t)st[2];
  return TSIM_OK;
}

extern "C" int tsim_ufw_match_table(tsim_ufw *h, int32_t k, uint32_t *dist, uint16_t *parent) {
  if (!h || !dist || !parent) return tsim_fail(TSIM_EINVAL, "NULL argument");
  if (!h->a.match_k) return tsim_fail(TSIM_EINVAL, "the handle has no match tables (tsim_ufw_create_matching makes them)");
  if (k < 0 || k >= h->a.n_windows) return tsim_fail(TSIM_EINVAL, "window %d of %d", k, h->a.n_windows);
  const ufwk::WinDesc &d = h->desc[k];
  const size_t pairs = (size_t)d.n_nodes * (size_t)d.n_nodes;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy(dist, h->mdist + d.off_table, pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(parent, h->mparent + d.off_table, pairs * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return TSIM_OK;
}

namespace {
struct SoftOut {  // what tsim_ufw_decode_soft_device adds to tsim_ufw_decode_device
  int metric, n_bins;
  uint64_t *d_hist;
  uint32_t *d_soft;  // four values per row, or NULL
};

template <bool Soft>
void ufw_launch(const ufwk::Args &a, unsigned blocks, size_t lds, hipStream_t stream) {
  if constexpr (!Soft)
    if (a.match_k) {  // (a handle of tsim_ufw_create_matching: no heralds, no soft outputs)
      if (a.cap) hipLaunchKernelGGL((ufwk::k_ufw<true, false, false, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
      else hipLaunchKernelGGL((ufwk::k_ufw<false, false, false, true>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
      return;
    }
  if (a.node_det) {
    if (a.cap) hipLaunchKernelGGL((ufwk::k_ufw<true, true, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
    else hipLaunchKernelGGL((ufwk::k_ufw<false, true, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  } else if (a.cap) hipLaunchKernelGGL((ufwk::k_ufw<true, false, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
  else hipLaunchKernelGGL((ufwk::k_ufw<false, false, Soft>), dim3(blocks), dim3(64 * a.waves), lds, stream, a);
}
}  // namespace

// the decode entry points; soft == NULL: tsim_ufw_decode_device
static int ufw_decode(tsim_ufw *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor, const uint8_t *d_test,
                      int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred, const SoftOut *soft, void *stream) {
  if (!h) return tsim_fail(TSIM_EINVAL, "decoder is NULL");
  ufwk::Args a = h->a;
  if (const int rc = ufh::check_rows(a, d_rows, n, row_bytes, obs_lo, obs_hi, d_counters, d_pred)) return rc;
  if (soft) {
    if (a.match_k) return tsim_fail(TSIM_EINVAL, "a cluster-matching handle has no soft outputs");
    if (const int rc = ufh::check_soft(a, soft->metric, soft->n_bins, soft->d_hist, soft->d_soft)) return rc;
  }
  if (n == 0) return TSIM_OK;
  HIP_TRY(hipSetDevice(h->device));
  ufh::fill_rows(a, d_rows, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters);
  return ufh::launch_rows(a, d_rows, n, d_pred, h->grid, &h->launches, [&](ufwk::Args &a, int64_t r0, unsigned blocks, size_t lds) {
    if (soft) {
      a.soft = soft->d_soft ? soft->d_soft + 4 * r0 : nullptr;
      ufw_launch<true>(a, blocks, lds, (hipStream_t)stream);
    } else {
      ufw_launch<false>(a, blocks, lds, (hipStream_t)stream);
    }
  });
}

extern "C" int tsim_ufw_decode_device(tsim_ufw *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                      const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                      void *stream) {
  return ufw_decode(h, d_rows, n, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters, d_pred, nullptr, stream);
}

extern "C" int tsim_ufw_decode_soft_device(tsim_ufw *h, const uint8_t *d_rows, int64_t n, int64_t row_bytes, const uint8_t *d_xor,
                                           const uint8_t *d_test, int32_t obs_lo, int32_t obs_hi, uint64_t *d_counters, uint64_t *d_pred,
                                           int32_t metric, int32_t n_bins, uint64_t *d_hist, uint32_t *d_soft, void *stream) {
  const SoftOut soft{metric, n_bins, d_hist, d_soft};
  return ufw_decode(h, d_rows, n, row_bytes, d_xor, d_test, obs_lo, obs_hi, d_counters, d_pred, &soft, stream);
}
