"""The large inputs of the GPU tests of cluster matching, the complementary gap, heralds, soft outputs and heralded windows
(``test_gpu_unionfind_matching_large.py``), and the proof, from the numpy statement alone, that they reach the code the small
graphs never did: tables of 2048 nodes (eight trips of the table kernels' strided loops, distances next to 2^27, 2047 mask
rounds), a shot whose state with both dynamic programs fills a block's LDS to the last 2 KiB and the refusal one step further,
matched clusters of exactly K and of more than K defects with node indices beyond 255 and 1023, heralds on columns beyond 4096
(a lane's second word of the herald sweep), 65535 full edges, every number of waves a block can have, and windows with heralds
late in a long run.  The references of the tables are written here and are not the statement's: a closed form on the chain, a
heap Dijkstra on the sparse graph.  Every builder is seeded and a case is built once and shared with the GPU file."""

import heapq
import types

import numpy as np
import pytest

from test_unionfind import syndrome_of
from test_unionfind_large import LDS_BLOCK, case, shots_per_block_rule, sparse_graph
from test_unionfind_matching import issue_memory

from tsim_amd import circuits, faults
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.decode import (MATCH_INF, MAX_MATCH_NODES, DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder, uf_erasure_shot_bytes,
                             uf_match_shot_bytes, uf_shot_bytes)

W_MAX = 65535

# shots (waves) per block by the rule of tsim_uf_create (shots_per_block_rule), worked out per handle: with every large case
# of the peeling decoder at 1 wave but for these, the matching handles cover 1, 2, 3 and 4
D9_WAVES = {4: 1, 12: 1, "gap": 1}
D9E_HANDLES = [(10, 24, False), (4, 8, False), (4, 8, True), (12, 32, False)]   # (K, max_hubs, with the gap)
D9E_WAVES = {(False, 10, 24, False): 2, (False, 4, 8, False): 1, (False, 4, 8, True): 1, (False, 12, 32, False): 1,
             (True, 10, 24, False): 1, (True, 4, 8, False): 4, (True, 4, 8, True): 3, (True, 12, 32, False): 1}


# ---- the references of the tables --------------------------------------------------------------------------------------------

def chain_tables(edge_obs: np.ndarray, observable: int, w: int = W_MAX):
    """``(dist int64[N, N], mask uint64[N, N], dist2 int64[N, N, 2])`` of the chain 0 - 1 - ... - N - 1 whose every edge weighs
    ``w``, in closed form: between two nodes there is one path, no path continues from node 0, and a walk that repeats an edge
    keeps its class."""
    N = len(edge_obs) + 1
    at = np.arange(N, dtype=np.int64)
    upto = np.zeros(N, np.uint64)   # the XOR of the edges 0 .. v - 1: the path from v to node 0
    upto[1:] = np.bitwise_xor.accumulate(np.asarray(edge_obs, np.uint64))
    dist = np.abs(at[:, None] - at[None, :]) * w
    mask = upto[:, None] ^ upto[None, :]
    dist[0, 1:], mask[0, 1:] = MATCH_INF, 0
    cls = ((mask >> np.uint64(observable)) & np.uint64(1)).astype(np.int64)
    dist2 = np.full((N, N, 2), MATCH_INF, np.int64)
    np.put_along_axis(dist2, cls[:, :, None], dist[:, :, None], axis=2)
    return dist, mask, dist2


def dijkstra_rows(graph: DecodingGraph, w, sources, observable: int = 0):
    """``(dist int64[S, N], mask uint64[S, N], dist2 int64[S, N, 2])`` for the sources listed: a heap Dijkstra over the arcs of the
    docstring's rule (no arc leaves node 0), the parent of a target the first edge in ascending edge index whose other end
    ``x >= 1`` attains the distance, the masks along the parents in order of distance, and the same search over the doubled
    states ``2 * node + class``."""
    N = graph.n_nodes
    ew = [int(x) for x in w]
    obs = [int(x) for x in graph.edge_obs]
    c = [(x >> observable) & 1 for x in obs]
    adj = [[] for _ in range(N)]
    for e, (u, v) in enumerate(zip(graph.edge_u.tolist(), graph.edge_v.tolist())):
        adj[u].append((e, v))
        adj[v].append((e, u))
    dist, mask = np.zeros((len(sources), N), np.int64), np.zeros((len(sources), N), np.uint64)
    dist2 = np.zeros((len(sources), N, 2), np.int64)
    for s, a in enumerate(sources):
        d = [MATCH_INF] * N
        d[a] = 0
        heap = [(0, a)]
        while heap:
            dv, v = heapq.heappop(heap)
            if dv > d[v] or v == 0:
                continue
            for e, x in adj[v]:
                if dv + ew[e] < d[x]:
                    d[x] = dv + ew[e]
                    heapq.heappush(heap, (d[x], x))
        m = [0] * N
        for v in sorted((v for v in range(N) if v != a and d[v] != MATCH_INF), key=d.__getitem__):   # (a parent lies nearer)
            e, x = next((e, x) for e, x in adj[v] if x >= 1 and d[x] != MATCH_INF and d[x] + ew[e] == d[v])
            m[v] = m[x] ^ obs[e]
        d2 = [MATCH_INF] * (2 * N)
        d2[2 * a] = 0
        heap = [(0, 2 * a)]
        while heap:
            dv, state = heapq.heappop(heap)
            if dv > d2[state] or state < 2:
                continue
            for e, x in adj[state >> 1]:
                to = 2 * x + ((state & 1) ^ c[e])
                if dv + ew[e] < d2[to]:
                    d2[to] = dv + ew[e]
                    heapq.heappush(heap, (d2[to], to))
        dist[s], mask[s], dist2[s] = d, np.array(m, np.uint64), np.array(d2, np.int64).reshape(N, 2)
    return dist, mask, dist2


# ---- the rule's growth, restated: the clusters of a row when growth ends --------------------------------------------------------

def grown_clusters(uf: UnionFindDecoder, row: np.ndarray):
    """The defect nodes of every cluster of one row of detector columns when growth ends (step 1 of the rule, with the edges of
    the heralds that are set full from the start); ``None`` for a miss.  Not the statement's code: min-label sweeps from scratch."""
    g = uf.graph
    n, eu, ev = g.n_nodes, g.edge_u.astype(np.int64), g.edge_v.astype(np.int64)
    defect = np.zeros(n, np.bool_)
    defect[np.flatnonzero(row[g.node_det]) + 1] = True
    cap = np.full(g.n_edges, 2, np.int64) if uf.edge_caps is None else uf.edge_caps.astype(np.int64)
    grown = np.zeros(g.n_edges, np.int64)
    for h in np.flatnonzero(row[g.herald_det]) if g.n_heralds else ():
        e = g.herald_edges[g.herald_ptr[h]:g.herald_ptr[h + 1]]
        grown[e] = cap[e]
    label = np.arange(n)
    while True:
        fu, fv = eu[grown == cap], ev[grown == cap]
        while True:   # (labels stay upper bounds from round to round: clusters only merge)
            low = np.minimum(label[fu], label[fv])
            new = label.copy()
            np.minimum.at(new, fu, low)
            np.minimum.at(new, fv, low)
            new = new[new]
            if np.array_equal(new, label):
                break
            label = new
        odd = (np.bincount(label[defect], minlength=n) & 1).astype(np.bool_)
        odd[0] = False
        active = odd[label]
        if not active.any():
            return [np.flatnonzero(defect & (label == r)) for r in np.unique(label[defect])]
        new = np.minimum(cap, grown + active[eu] + active[ev])
        if np.array_equal(new, grown):
            return None
        grown = new


# ---- the cases ---------------------------------------------------------------------------------------------------------------

SPARSE_SOURCES = [0, 1, 2, 255, 256, 257, 511, 512, 1023, 1024, 2045, 2046, 2047]   # (2045 .. 2047: the island)

_CASES: dict = {}


def tiles(bits: np.ndarray, waves: int) -> np.ndarray:
    """``bits`` and ``waves - 1`` more tiles of the same rows in another order each: wave ``t`` of block 0 owns rows
    ``64 t .. 64 t + 63``, so every wave of a block decodes and the host decodes each row once."""
    assert len(bits) % 64 == 0
    return np.concatenate([np.roll(bits, 7 * t, axis=0)[::-1 if t & 1 else 1] for t in range(waves)])


def heralded_memory(d: int, rounds: int, p: float, pe: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, after_clifford_heralded_erasure=pe))


def surface(d: int, p: float, n: int):
    c = issue_memory(d, d, p)
    uf = UnionFindDecoder.from_circuit(c, weights="probability")
    return uf, faults.fault_rows_host(c.compile_faults(), 0, n, (1, 2)).view(np.bool_)


def wrap_base(kind: str, n: int = 1061):
    """The base of a grid-wrap test: ``(decoder with the gap, n seeded rows)`` of d = 3; 1061 is prime and no multiple of 64."""
    if kind == "gap":
        c = issue_memory(3, 3, 1e-2)
        ug = UnionFindDecoder.from_circuit(c, weights="probability").with_cluster_matching(10).with_gap_output(0)
    else:   # K = 2 and 4 hubs at this rate: matched and peeled clusters, erased edges and clusters peeled for their hubs
        c = heralded_memory(3, 3, 3e-3, 5e-2)
        ug = UnionFindDecoder.from_circuit(c, weights="probability", heralds=True).with_erasure_matching(2, max_hubs=4).with_gap_output(0)
    return ug, faults.fault_rows_host(c.compile_faults(), 0, n, (1, 2)).view(np.bool_)


def large(name: str):
    """The case ``name``, built once: a namespace of its graph or decoders and its rows (bool: detector columns, observables)."""
    if name in _CASES:
        return _CASES[name]
    if name == "chain2048":
        rng = np.random.default_rng(2048)
        u = np.arange(2047)
        g = DecodingGraph(2048, u, u + 1, rng.integers(0, 4, size=2047).astype(np.uint64))
        out = types.SimpleNamespace(graph=g, w=np.full(2047, W_MAX, np.int64), tables=[chain_tables(g.edge_obs, k) for k in (0, 1)])
    elif name == "sparse2048":
        rng = np.random.default_rng(2049)
        g = sparse_graph(53, 2048, 7000, 150, island=3)
        w = rng.integers(1, W_MAX + 1, size=g.n_edges)
        w[rng.choice(g.n_edges, size=8, replace=False)] = np.resize([1, W_MAX], 8)
        sources = SPARSE_SOURCES + sorted(rng.choice(np.setdiff1d(np.arange(2048), SPARSE_SOURCES), size=32, replace=False).tolist())
        out = types.SimpleNamespace(graph=g, w=w, sources=sources, rows=dijkstra_rows(g, w, sources, 0))
    elif name == "d9":
        uf, bits = surface(9, 1e-2, 96)
        matching = {K: uf.with_cluster_matching(K) for K in (4, 12)}
        matching[12].match_table()   # (the decoder with the gap shares it)
        out = types.SimpleNamespace(uf=uf, bits=bits, matching=matching, gap=matching[12].with_gap_output(observable=0, bins=64))
    elif name == "d11":
        uf, bits = surface(11, 5e-3, 64)
        out = types.SimpleNamespace(uf=uf, bits=bits, matching={10: uf.with_cluster_matching(10)})
    elif name == "d9e":
        c = heralded_memory(9, 9, 5e-3, 2e-2)
        bits = faults.fault_rows_host(c.compile_faults(), 0, 64, (1, 2)).view(np.bool_)
        peeling = {w: UnionFindDecoder.from_circuit(c, weights="probability" if w else None, heralds=True) for w in (False, True)}
        handles = {}
        for w, uf in peeling.items():
            for K, H, gap in D9E_HANDLES:
                ue = handles[w, K, H, False] if gap else uf.with_erasure_matching(K, max_hubs=H)
                handles[w, K, H, gap] = ue.with_gap_output(0) if gap else ue
        out = types.SimpleNamespace(bits=bits, peeling=peeling, handles=handles)
    elif name == "d3x120e":
        c = heralded_memory(3, 120, 2e-3, 1e-2)
        bits = faults.fault_rows_host(c.compile_faults(), 0, 130, (1, 2)).view(np.bool_)
        out = types.SimpleNamespace(bits=bits, w=WindowedUnionFindDecoder.from_circuit(c, 5 * 8, 10 * 8, weights="probability", heralds=True))
    else:
        raise KeyError(name)
    _CASES[name] = out
    return out


def d9e_quiet():
    """``(the weighted d9e decoder of K = 4 and 8 hubs with the gap, 64 rows of the same columns at a fifth of the rates)``.  Every
    row of ``d9e`` itself has a peeled cluster, so its gap is 0 whatever the class program finds; in most of these every cluster
    is matched and the deficits take many values."""
    if "d9e_quiet" not in _CASES:
        bits = faults.fault_rows_host(heralded_memory(9, 9, 1e-3, 4e-3).compile_faults(), 0, 64, (3, 4)).view(np.bool_)
        _CASES["d9e_quiet"] = (large("d9e").handles[True, 4, 8, True], bits)
    return _CASES["d9e_quiet"]


def dense_erased():
    """The 65535-edge graph with a herald that erases every edge (``test_dense_graph_first_and_last_words``), set in every row."""
    if "dense_erased" not in _CASES:
        base = case("dense").plain.graph
        cols = [0, 100, 200, 300, 403]
        lists = [[0], [32767], [32768], [65534], list(range(65535))]
        g = DecodingGraph(400, base.edge_u, base.edge_v, base.edge_obs, node_det=np.setdiff1d(np.arange(404), cols), herald_det=cols,
                          herald_ptr=np.cumsum([0] + [len(x) for x in lists]), herald_edges=[e for x in lists for e in x])
        rng = np.random.default_rng(65)
        bits = np.zeros((20, 406), np.bool_)
        for r in range(20):
            bits[r, rng.choice(g.node_det, size=int(rng.integers(1, 30)), replace=False)] = True
        bits[:, cols[:4]] = rng.random((20, 4)) < 0.5
        bits[:, 403] = True
        bits[:, 404:] = rng.integers(0, 2, size=(20, 2)).astype(np.bool_)
        _CASES["dense_erased"] = types.SimpleNamespace(uf=UnionFindDecoder(g, 2), bits=bits)
    return _CASES["dense_erased"]


# ---- 1. tables at the node limit -----------------------------------------------------------------------------------------------

def test_chain2048_is_the_worst_case_of_the_table_kernels():
    c = large("chain2048")
    dist, mask, dist2 = c.tables[0]
    assert c.graph.n_nodes == MAX_MATCH_NODES == 2048 and -(-2048 // 256) == 8   # eight trips of `for (v = tid; v < N; v += 256)`
    assert dist[1][2047] == 2046 * W_MAX and abs((1 << 27) - int(dist[1][2047])) < (1 << 27) // 100 and dist.max() == MATCH_INF
    assert dist[2047][0] == 2047 * W_MAX < 1 << 27   # the largest finite entry: 2047 sweeps and 2047 mask rounds behind it
    assert dist[0][0] == 0 and (dist[0, 1:] == MATCH_INF).all() and (dist[1:, 0] == np.arange(1, 2048) * W_MAX).all()
    assert not mask[0].any() and sorted(np.unique(mask).tolist()) == [0, 1, 2, 3]
    for k in (0, 1):
        d2 = c.tables[k][2]
        assert np.array_equal(d2.min(axis=2), dist) and ((d2 == MATCH_INF).sum(axis=2) >= 1).all()   # one class a pair: no W0
        assert (d2[:, :, 1] != MATCH_INF).sum() > 2048 * 2048 // 3


def test_the_closed_form_equals_the_statement_on_a_shorter_chain():
    rng = np.random.default_rng(40)
    u = np.arange(39)
    g = DecodingGraph(40, u, u + 1, rng.integers(0, 4, size=39).astype(np.uint64))
    um = UnionFindDecoder(g, 2).with_cluster_matching(10, np.full(39, W_MAX))
    for k in (0, 1):
        dist, mask, dist2 = chain_tables(g.edge_obs, k)
        assert np.array_equal(um.match_table()[0], dist) and np.array_equal(um.match_table()[1], mask)
        got, w0 = um.with_gap_output(k, cap=5).gap_table()
        assert np.array_equal(got, dist2) and w0 is None


def test_sparse2048_has_the_island_both_extremes_and_the_sources():
    c = large("sparse2048")
    g, (dist, mask, dist2) = c.graph, c.rows
    assert (g.n_nodes, g.n_edges) == (2048, 7152) and c.w.min() == 1 and c.w.max() == W_MAX
    assert c.sources[:13] == SPARSE_SOURCES and len(set(c.sources)) == len(c.sources) == 45
    island = [c.sources.index(v) for v in (2045, 2046, 2047)]
    assert (dist[island][:, 2045:] != MATCH_INF).all() and (dist[island][:, :2045] == MATCH_INF).all()
    others = [s for s, a in enumerate(c.sources) if 1 <= a < 2045]
    assert (dist[others][:, 2045:] == MATCH_INF).all() and (dist[others][:, :2045] != MATCH_INF).mean() > 0.99   # (a few nodes have no edge)
    assert (dist[0] == np.where(np.arange(2048) == 0, 0, MATCH_INF)).all() and not mask[0].any()
    assert np.array_equal(dist2.min(axis=2), dist) and (dist2[others][:, :2045] != MATCH_INF).mean() > 0.99   # both classes: cycles
    assert dist[dist != MATCH_INF].max() < 2047 * W_MAX and not mask[dist == MATCH_INF].any() and mask.max() == 3


def test_the_dijkstra_reference_equals_the_statement_on_d9():
    """Where both are cheap.  Every eighth source, node 0 and the last node."""
    ug = large("d9").gap
    sources = sorted(set(range(0, 721, 8)) | {1, 720})
    dist, mask, dist2 = dijkstra_rows(ug.graph, ug.match_weights, sources, 0)
    want_dist, want_mask = ug.match_table()
    assert np.array_equal(dist, want_dist[sources]) and np.array_equal(mask, want_mask[sources])
    assert np.array_equal(dist2, ug.gap_table()[0][sources])


# ---- 2. cluster matching and the gap on large surface codes --------------------------------------------------------------------

def clusters_of(c):
    """Per decoded row of a case the defect nodes of its clusters (``grown_clusters``), built once."""
    if not hasattr(c, "clusters"):
        nd = c.uf.num_detectors
        c.clusters = [grown_clusters(c.uf, row) if row.any() else [] for row in c.bits[:, :nd]]
    return c.clusters


@pytest.mark.parametrize("name", ["d9", "d11"])
def test_surface_cases_are_what_the_issue_says(name):
    c = large(name)
    g, nd = c.uf.graph, c.uf.num_detectors
    dets = c.bits[:, :nd]
    assert (g.n_nodes, g.n_edges, len(c.bits)) == ((721, 3498, 96) if name == "d9" else (1321, 6663, 64))
    assert c.uf.edge_caps is not None and not c.uf.missed(dets).any()
    want = {("d9", 4): (1590, 267), ("d9", 12): (1756, 101), ("d11", 10): (1784, 50)}
    clusters = clusters_of(c)
    sizes = np.array([len(x) for row in clusters for x in row])
    for K, um in c.matching.items():
        assert um.match_counts(dets) == want[name, K] == (int((sizes <= K).sum()), int((sizes > K).sum()))
        # the two sides of `m <= K`: clusters of exactly K defects, and of the next size there is.  A cluster off the boundary
        # ends growth with an even number of defects and a row has one boundary cluster at most, so with K even the next
        # size is K + 2 (K + 1 only for the boundary cluster)
        assert (sizes == K).any() and sizes[sizes > K].min() <= K + 2, (name, K, np.bincount(sizes).tolist())
        assert any(K in {len(x) for x in row} and max(len(x) for x in row) > K for row in clusters)   # (both in one row)
        assert shots_per_block_rule(uf_match_shot_bytes(g.n_nodes, g.n_edges, True, K)) == 1
    K = max(c.matching)
    top = max(int(x.max()) for row in clusters for x in row if len(x) <= K)
    assert top > (1023 if name == "d11" else 255)   # a matched cluster reads rows of the table beyond these
    assert any(len(x) <= K and x.min() <= 255 < x.max() for row in clusters for x in row)


def test_d9_with_the_gap_nearly_fills_the_block_and_d11_does_not_fit():
    c = large("d9")
    shot = uf_match_shot_bytes(721, 3498, True, 12, gap=True)
    assert shot == 63424 and 0 <= LDS_BLOCK - 16 - shot < 2100 and shots_per_block_rule(shot) == D9_WAVES["gap"] == 1
    assert uf_shot_bytes(721, 3498, True) < 32 * 1024 < shot   # the arrays of the dynamic programs lie beyond 32 KiB of the block
    assert 16 + uf_match_shot_bytes(1321, 6663, True, 12, gap=True) == 16 + 70400 > LDS_BLOCK
    assert 16 + uf_match_shot_bytes(1321, 6663, True, 12) <= LDS_BLOCK   # (the classes are what does not fit)
    D = c.gap.gap_outputs(c.bits[:, :720])
    assert len(np.unique(D)) == 9 and c.gap.soft_bins == 64 and c.gap.gap_cap == c.gap.gap_table()[1]
    assert np.array_equal(c.gap.predictions(c.bits[:, :720]), c.matching[12].predictions(c.bits[:, :720]))


@pytest.mark.parametrize("name", ["d9", "d11", "d9e"])
def test_every_peeled_correction_reproduces_its_syndrome(name):
    """A matching decoder has no ``flipped_edges``; the peeling decoder of the same graph and caps, whose growth it shares, has."""
    c = large(name)
    for uf in ([c.uf] if name != "d9e" else c.peeling.values()):
        g = uf.graph
        dets = c.bits[:, :uf.num_detectors]
        missed, flipped, pred = uf.missed(dets), uf.flipped_edges(dets), uf.predictions(dets)
        assert not missed.any()
        for r in range(len(dets)):
            assert np.array_equal(syndrome_of(g, flipped[r]), dets[r, g.node_det]), (name, r)
            assert int(np.bitwise_xor.reduce(g.edge_obs[flipped[r]], initial=np.uint64(0))) == int(pred[r]), (name, r)


# ---- 3. heralds on wide rows -----------------------------------------------------------------------------------------------------

def test_d9e_reads_a_second_word_of_the_herald_sweep():
    c = large("d9e")
    assert c.bits.shape == (64, 5905) and (5905 + 7) // 8 == 739
    for weighted, uf in c.peeling.items():
        g = uf.graph
        assert (g.n_nodes, g.n_edges, g.n_heralds, uf.num_detectors) == (721, 3498, 5184, 5904)
        decoded = c.bits[:, g.node_det].any(axis=1)
        late = g.herald_det[g.herald_det >= 4096]
        hit = decoded & c.bits[:, late].any(axis=1)
        assert hit.sum() >= 32
        # lane l reads the bytes 8 l .. 8 l + 7 and then 512 + 8 l ..: a set herald there is a col_herald index beyond 4095
        col = int(late[np.flatnonzero(c.bits[np.flatnonzero(hit)[0], late])[0]])
        assert col // 8 // 8 * 8 >= 512 and (uf.num_detectors + 7) // 8 > 512
        assert any(np.diff(g.herald_ptr)[np.flatnonzero(c.bits[r, g.herald_det] & (g.herald_det >= 4096))].sum() > 0 for r in np.flatnonzero(hit))


def test_d9e_handles_cover_the_waves_and_the_counts():
    c = large("d9e")
    for (weighted, K, H, gap), ue in c.handles.items():
        g = ue.graph
        shot = uf_erasure_shot_bytes(g.n_nodes, g.n_edges, weighted, K, H, gap)
        assert shots_per_block_rule(shot) == D9E_WAVES[weighted, K, H, gap], (weighted, K, H, gap, shot)
        assert (ue.match_defects, ue.max_hubs, ue.gap_observable is not None) == (K, H, gap)
    assert 16 + uf_erasure_shot_bytes(721, 3498, True, 12, 32, True) == 16 + 85152 > LDS_BLOCK
    assert 16 + uf_erasure_shot_bytes(721, 3498, False, 12, 32, True) > LDS_BLOCK
    dets = c.bits[:, :5904]
    ue = c.handles[True, 4, 8, False]
    assert ue.match_counts(dets)[1] == 156 and ue.erasure_counts(dets)[1] == 12 and ue.erasure_counts(dets)[0] > 1000
    assert set(D9E_WAVES.values()) | set(D9_WAVES.values()) == {1, 2, 3, 4}   # sections 2 and 3 between them
    assert len(tiles(c.bits, 4)) == 256 and np.array_equal(tiles(c.bits, 4)[:64], c.bits)


def test_d9e_quiet_rows_show_the_class_program():
    ug, bits = d9e_quiet()
    c = large("d9e")
    assert bits.shape == c.bits.shape and (c.handles[True, 4, 8, True].gap_outputs(c.bits[:, :5904]) == ug.gap_cap).all()
    D = ug.gap_outputs(bits[:, :5904])
    assert len(np.unique(D)) >= 16 and ((D > 0) & (D < ug.gap_cap)).sum() >= 20 and (D == ug.gap_cap).sum() >= 20
    assert all(x > 0 for x in ug.match_counts(bits[:, :5904]) + ug.erasure_counts(bits[:, :5904]))
    late = ug.graph.herald_det[ug.graph.herald_det >= 4096]
    assert bits[:, late].any(axis=1).all()


# ---- 4. soft outputs at their bounds ---------------------------------------------------------------------------------------------

def test_soft_outputs_reach_their_bounds():
    c = dense_erased()
    values = c.uf.soft_outputs(c.bits[:, :404])
    assert (values[:, 1] == 65535).all() and (values[:, 2] == 400).all() and not values[:, 0].any()   # full << 16 | most at its top
    chain = case("chain1500")
    values = chain.plain.soft_outputs(chain.bits[:, :1499])
    assert values[0, 3] == 700 and values[:, 3].max() > 1024 and values[:, 0].max() > 1024
    d15 = case("d15")
    assert d15.plain.graph.n_nodes == 3361 and len(d15.bits) == 48


# ---- 5. the bases of the grids that wrap ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["gap", "erasure"])
def test_wrap_bases_count_in_every_accumulator(kind):
    ug, bits = wrap_base(kind)
    nd = ug.num_detectors
    dets = bits[:, :nd]
    assert len(bits) == 1061 and len(bits) % 64 and bits.shape[1] == nd + 1
    D = ug.gap_outputs(dets)
    assert ((D > 0) & (D < ug.gap_cap)).any() and (ug.predictions(dets) != bits[:, nd]).any()
    if kind == "gap":
        assert (ug.graph.n_nodes, ug.match_defects) == (25, 10) and ug.match_counts(dets)[0] > 500
    else:
        assert all(x > 0 for x in ug.match_counts(dets) + ug.erasure_counts(dets))


# ---- 6. windows with heralds on a long run ---------------------------------------------------------------------------------------

def window_trace(w: WindowedUnionFindDecoder, row: np.ndarray, flips: np.ndarray):
    """``(the windows decoded, the windows whose committed flips toggle a column the next window still owns)`` of one row of
    detector columns whose committed flips (global edges) are ``flips``, by "Decoding a row" of the module docstring."""
    g, C, wins = w.graph, w.commit, w.windows()
    low = np.where(g.edge_u > 0, g.edge_u, g.edge_v) - 1
    commit_window = np.minimum(low // C, len(wins) - 1)
    r = row[g.node_det].copy()
    decoded, carries = [], []
    for k, x in enumerate(wins):
        if r[x.lo:x.hi].any():
            decoded.append(k)
        for e in flips[commit_window[flips] == k]:
            for v in (int(g.edge_u[e]), int(g.edge_v[e])):
                if v:
                    r[v - 1] ^= True
                    if k + 1 < len(wins) and v - 1 >= wins[k + 1].lo:
                        carries.append(k)
    assert not r.any()
    return decoded, sorted(set(carries))


def test_d3x120e_has_late_heralds_in_late_windows_and_carries():
    c = large("d3x120e")
    w, g = c.w, c.w.graph
    info = w.info()
    assert c.bits.shape == (130, 6721) and (6721 + 7) // 8 == 841 and w.num_detectors == 6720
    assert (info["n_windows"], w.commit, w.window, g.n_heralds) == (23, 40, 80, 5760) and w.edge_caps is not None
    dets = c.bits[:, :6720]
    assert not w.missed(dets).any()
    late_heralds, most_carries = 0, 0
    for row, flips in zip(dets, w.flipped_edges(dets)):
        if not row[g.node_det].any():
            continue
        decoded, carries = window_trace(w, row, flips)
        most_carries = max(most_carries, len(carries))
        fired = set(np.flatnonzero(row[g.herald_det] & (g.herald_det >= 4096)).tolist())
        late_heralds += any(k >= 1 and fired & set(w.windows()[k].heralds.tolist()) for k in decoded)
    assert late_heralds >= 10   # a decoded window other than the first pre-grows the edges of a herald column beyond 4095
    assert most_carries >= 2    # a row hands defects on at two window advances or more
