"""Cluster matching of the union-find decoder without a device ("Cluster matching" in the module docstring of
``tsim_amd.decode``): the match weights against their formula, the match table against a heap Dijkstra, the dynamic program
against an enumeration of all pairings, the invariants of a decoded row, fewer decoded errors than peeling, and what is refused."""

import heapq

import numpy as np
import pytest

from test_unionfind import chain_graph
from test_unionfind_large import dense_graph, sparse_graph

from tsim_amd import circuits, faults
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.decode import MATCH_INF, MAX_MATCH_NODES, DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder, uf_match_shot_bytes, uf_shot_bytes


def issue_memory(d: int, rounds: int, p: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, before_measure_flip_probability=p))


_SAMPLES: dict = {}


def surface_sample(d: int, rounds: int, p: float, n: int):
    """``(peeling decoder, matching decoder, rows bool [n, detectors + observables])``: weighted growth at resolution 4, cluster
    matching at its defaults, rows of the fault sampler's host statement; built once (the decoders cache syndromes)."""
    if (d, rounds, p, n) not in _SAMPLES:
        c = issue_memory(d, rounds, p)
        uf = UnionFindDecoder.from_circuit(c, weights="probability", resolution=4)
        rows = faults.fault_rows_host(c.compile_faults(), 0, n, (1, 2)).view(np.bool_)
        _SAMPLES[d, rounds, p, n] = (uf, uf.with_cluster_matching(), rows)
    return _SAMPLES[d, rounds, p, n]


def two_boundary_graph() -> DecodingGraph:
    """0 - 1 - 2 - 3 - 4 - 5 - 0: the chain 1 .. 5 with a boundary edge at both ends; edge (2, 3) flips observable 0, (0, 5) observable 1."""
    return DecodingGraph(6, [0, 0, 1, 2, 3, 4], [1, 5, 2, 3, 4, 5], np.array([0, 2, 0, 1, 0, 0], np.uint64))


def table_cases() -> dict:
    """name -> ``(graph, match weights)``: the four graphs of the table tests (70 and 130 nodes are no multiples of 64) and the one
    with two cheap boundary edges around an expensive chain."""
    rng = np.random.default_rng(77)
    g130 = sparse_graph(7, 130, 400, 12)
    island = sparse_graph(9, 70, 150, 6, island=5)
    return {
        "chain70": (chain_graph(70), rng.integers(1, 2000, size=69)),
        "random130": (g130, rng.integers(1, 2000, size=g130.n_edges)),
        "ones130": (g130, np.ones(g130.n_edges, np.int64)),
        "island70": (island, rng.integers(1, 60000, size=island.n_edges)),
        "two_boundary": (two_boundary_graph(), np.array([1, 1, 100, 100, 100, 100])),
    }


def matching_decoder(graph, weights, K: int = 10, caps=None) -> UnionFindDecoder:
    return UnionFindDecoder(graph, edge_caps=caps).with_cluster_matching(K, weights)


def dijkstra_table(graph: DecodingGraph, w):
    """The match table by a heap Dijkstra per source, the parent rule applied to its distances, the masks by descent."""
    N = graph.n_nodes
    adj = [[] for _ in range(N)]
    for e, (u, v) in enumerate(zip(graph.edge_u.tolist(), graph.edge_v.tolist())):
        adj[u].append((e, v))
        adj[v].append((e, u))
    dist = np.full((N, N), MATCH_INF, np.int64)
    mask = np.zeros((N, N), np.uint64)
    dist[0, 0] = 0
    for a in range(1, N):
        d = dist[a]
        d[a] = 0
        heap = [(0, a)]
        while heap:
            dv, v = heapq.heappop(heap)
            if dv > d[v] or v == 0:  # (no path continues from the boundary)
                continue
            for e, x in adj[v]:
                if dv + int(w[e]) < d[x]:
                    d[x] = dv + int(w[e])
                    heapq.heappush(heap, (int(d[x]), x))
        for v in sorted((v for v in range(N) if v != a and d[v] != MATCH_INF), key=lambda v: d[v]):  # (parents lie nearer)
            e, x = next((e, x) for e, x in adj[v] if x != 0 and d[x] != MATCH_INF and d[x] + int(w[e]) == d[v])
            mask[a, v] = mask[a, x] ^ graph.edge_obs[e]
    return dist.astype(np.uint32), mask


# ---- the match weights -------------------------------------------------------------------------------------------------------

def test_match_weights_equal_their_formula():
    g = surface_sample(3, 3, 3e-3, 40000)[0].graph
    for scale in (1000, 1, 65535):
        q = np.clip(g.edge_p, 1e-12, 0.5)
        L = np.log((1 - q) / q)
        want = np.clip(np.rint(scale * L / L.max()), 1, scale)
        got = g.match_weights(scale) if scale != 1000 else g.match_weights()
        assert got.dtype == np.uint16 and np.array_equal(got, want) and got.max() == scale
    assert len(np.unique(g.match_weights())) > 3
    half = DecodingGraph(3, [0, 1], [1, 2], np.zeros(2, np.uint64), [0.5, 0.7])  # L.max() == 0
    assert half.match_weights().tolist() == [1, 1]
    assert chain_graph(5, 2).match_weights(7).tolist() == [7] * 4  # (edge_p = 0 everywhere: every L is the largest)
    for bad in (0, 65536, 2.0, True):
        with pytest.raises(ValueError, match="scale"):
            g.match_weights(bad)


# ---- the match table ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(table_cases()))
def test_match_table_equals_a_heap_dijkstra(name):
    graph, w = table_cases()[name]
    um = matching_decoder(graph, w)
    dist, mask = um.match_table()
    assert um.match_table()[0] is dist  # cached
    want_dist, want_mask = dijkstra_table(graph, w)
    N = graph.n_nodes
    assert dist.dtype == np.uint32 and mask.dtype == np.uint64 and dist.shape == mask.shape == (N, N)
    assert np.array_equal(dist, want_dist)
    assert np.array_equal(mask, want_mask)
    assert (np.diag(dist) == 0).all() and (dist[0, 1:] == MATCH_INF).all() and not mask[dist == MATCH_INF].any()
    if name == "island70":  # the last five nodes have no way to the boundary or to the rest
        assert (dist[65:, :65] == MATCH_INF).all() and (dist[1:65, 65:] == MATCH_INF).all() and (dist[65:, 65:] != MATCH_INF).all()
    elif name == "two_boundary":
        assert dist[1, 5] == 400 and dist[1, 0] == 1 and dist[5, 0] == 1 and dist[3, 0] == 201
        assert mask[1, 5] == 1 and mask[5, 0] == 2 and mask[3, 0] == 1  # (3 - 2 - 1 - 0, not 3 - 4 - 5 - 0: the smaller edge)
    else:
        assert (dist[1:] != MATCH_INF).all()
    if name == "ones130":  # ties everywhere: many nodes have several edges that attain the distance
        ties = sum(1 for v in range(1, N) for a in (1, 64) if v != a and
                   sum(1 for e in np.flatnonzero((graph.edge_u == v) | (graph.edge_v == v))
                       if (x := int(graph.edge_u[e] + graph.edge_v[e] - v)) != 0 and dist[a, x] + 1 == dist[a, v]) > 1)
        assert ties > 20


def test_table_limit():
    n = MAX_MATCH_NODES + 1
    with pytest.raises(NotImplementedError, match="2049 nodes"):
        UnionFindDecoder(chain_graph(n, 3)).with_cluster_matching()


# ---- the dynamic program -----------------------------------------------------------------------------------------------------

def all_pairings(defects):
    """Every way to pair the defects with each other or with the boundary (0)."""
    if not defects:
        yield []
        return
    a, rest = defects[0], defects[1:]
    for tail in all_pairings(rest):
        yield [(a, 0)] + tail
    for k, b in enumerate(rest):
        for tail in all_pairings(rest[:k] + rest[k + 1:]):
            yield [(a, b)] + tail


def rule_top_down(dist, a):
    """The rule of the docstring as a recursion from the full set: ``(cost, pairs)`` of the first candidate of least cost."""
    memo = {0: (0, [])}

    def f(S):
        if S not in memo:
            i = (S & -S).bit_length() - 1
            R = S & (S - 1)
            best = None
            for base, other in [(R, 0)] + [(R ^ (1 << j), a[j]) for j in range(len(a)) if (R >> j) & 1]:
                sub, d = f(base), int(dist[a[i], other])
                if sub is None or d == MATCH_INF:
                    continue
                if best is None or sub[0] + d < best[0]:
                    best = (sub[0] + d, sub[1] + [(a[i], other)])
            memo[S] = best
        return memo[S]

    return f((1 << len(a)) - 1)


@pytest.mark.parametrize("name", ["random130", "ones130", "island70"])
def test_match_cluster_against_all_pairings(name):
    graph, w = table_cases()[name]
    um = matching_decoder(graph, w)
    dist, mask = um.match_table()
    rng = np.random.default_rng(3)
    for trial in range(60):
        m = 1 + trial % 6
        near = int(rng.integers(1, graph.n_nodes - 12))  # (defects that lie close: pairs compete with the boundary)
        a = sorted(rng.choice(np.arange(near, near + 12), size=m, replace=False).tolist())
        cost, got_mask, pairs = um._match_cluster(a)
        costs = [sum(int(dist[p]) for p in pr) for pr in all_pairings(a) if all(dist[p] != MATCH_INF for p in pr)]
        if not costs:
            assert cost is None
            continue
        assert cost == min(costs)
        assert sorted(x for p in pairs for x in p if x) == a and all(p[0] < p[1] or p[1] == 0 for p in pairs)
        assert sum(int(dist[p]) for p in pairs) == cost
        assert int(np.bitwise_xor.reduce([mask[p] for p in pairs])) == got_mask
        want = rule_top_down(dist, a)  # the first minimal candidate wins (on the all-ones graph most costs tie)
        assert want[0] == cost and sorted(want[1]) == sorted(pairs)


def test_first_minimal_candidate_wins_on_a_tie():
    """The ring 0 - 1 - 2 - 3 - 0 with unit weights, where pairings tie: the boundary comes first and strict < replaces."""
    g = DecodingGraph(4, [0, 0, 1, 2], [1, 3, 2, 3], np.array([1, 2, 4, 8], np.uint64))
    um = matching_decoder(g, np.ones(4, np.int64))
    dist, _ = um.match_table()
    assert dist[1, 0] == 1 and dist[3, 0] == 1 and dist[1, 3] == 2 and dist[1, 2] == 1 and dist[2, 0] == 2
    assert um._match_cluster([1, 3]) == (2, 1 ^ 2, [(1, 0), (3, 0)])  # boundary twice (2) comes before the pair (2)
    assert um._match_cluster([1, 2]) == (1, 4, [(1, 2)])               # the pair (1) beats 1 + 2
    cost, m, pairs = um._match_cluster([1, 2, 3])
    assert cost == 2 and sorted(pairs) == [(1, 0), (2, 3)] and m == 1 ^ 8   # (1, 0) + (2, 3) comes before (1, 2) + (3, 0)


# ---- a decoded row -----------------------------------------------------------------------------------------------------------

def test_growth_is_the_plain_decoders():
    uf, um, rows = surface_sample(3, 3, 3e-3, 40000)
    dets = rows[:2000, :uf.num_detectors]
    assert np.array_equal(um.missed(dets), uf.missed(dets))
    assert np.array_equal(um.growth_rounds(dets), uf.growth_rounds(dets))
    assert um._cache is not uf._cache and um.graph is uf.graph and um.edge_caps is uf.edge_caps
    assert um.match_defects == 10 and np.array_equal(um.match_weights, uf.graph.match_weights())
    matched, peeled = um.match_counts(dets)
    assert matched > 500 and peeled == 0
    one = uf.with_cluster_matching(1)
    m1, p1 = one.match_counts(dets)
    assert m1 + p1 == matched and p1 > 0 and m1 > 0


def chain_rows(runs_per_row) -> np.ndarray:
    """Rows over the chain of 70 nodes: per row a list of ``(first node, length)`` runs of consecutive defects."""
    bits = np.zeros((len(runs_per_row), 69), np.bool_)
    for r, runs in enumerate(runs_per_row):
        for first, length in runs:
            bits[r, first - 1:first - 1 + length] = True
    return bits


def test_clusters_larger_than_k_are_peeled_as_before():
    g = chain_graph(70)
    uf = UnionFindDecoder(g)
    um = uf.with_cluster_matching(1, np.arange(1, 70))
    dets = chain_rows([[(10, 2)], [(30, 4)], [(38, 6), (60, 2)], [(29, 1), (49, 1)], [(40, 2), (44, 2), (50, 4)]])
    assert np.array_equal(um.predictions(dets), uf.predictions(dets)) and um.predictions(dets).any()
    assert um.match_counts(dets) == (0, 8)


@pytest.mark.parametrize("K", [1, 2, 3, 10, 12])
def test_k_defects_are_matched_and_k_plus_one_peeled(K):
    g = chain_graph(70)
    um = matching_decoder(g, np.ones(69, np.int64), K)
    exactly, one_more = chain_rows([[(20, K)]]), chain_rows([[(20, K + 1)]])
    assert um.match_counts(exactly) == (1, 0) and um.match_counts(one_more) == (0, 1)
    assert um.match_counts(np.concatenate([exactly, one_more, chain_rows([[(1, 1)]])])) == (2, 1)  # (a boundary cluster of one defect)
    plain = UnionFindDecoder(g)
    both = np.concatenate([exactly, one_more])
    assert np.array_equal(um.predictions(both), plain.predictions(both))  # (on a chain there is one correction)


def test_fewer_decoded_errors_than_peeling():
    uf, um, rows = surface_sample(3, 3, 3e-3, 40000)
    nd = uf.num_detectors
    obs = rows[:, nd].astype(np.uint64)
    peeling, matching = int((uf.predictions(rows[:, :nd]) != obs).sum()), int((um.predictions(rows[:, :nd]) != obs).sum())
    print(f"d = 3, r = 3, p = 3e-3, 40000 rows: peeling {peeling} decoded errors, cluster matching {matching}; "
          f"clusters (matched, peeled) = {um.match_counts(rows[:, :nd])}")
    assert matching < peeling


# ---- what is refused ---------------------------------------------------------------------------------------------------------

def test_refusals():
    g = chain_graph(20, 5)
    uf = UnionFindDecoder(g)
    um = uf.with_cluster_matching()
    dets = chain_rows([[(3, 2)]])[:, :19]
    for bad in (0, 13, 2.0, True):
        with pytest.raises(ValueError, match="max_defects"):
            uf.with_cluster_matching(bad)
    with pytest.raises(ValueError, match="match weight 0"):
        uf.with_cluster_matching(weights=np.zeros(19, np.int64))
    with pytest.raises(ValueError, match="match weight 65536"):
        uf.with_cluster_matching(weights=np.full(19, 65536))
    with pytest.raises(ValueError, match="shape"):
        uf.with_cluster_matching(weights=np.ones(18, np.int64))
    with pytest.raises(ValueError, match="no soft output"):
        um.with_soft_output("rounds")
    with pytest.raises(ValueError, match="takes no cluster matching"):
        uf.with_soft_output("rounds").with_cluster_matching()
    with pytest.raises(ValueError, match="no flipped edges"):
        um.flipped_edges(dets)
    with pytest.raises(ValueError, match="no soft outputs"):
        um.soft_outputs(dets)
    for call in (uf.match_table, lambda: uf._match_cluster([1]), lambda: uf.match_counts(dets)):
        with pytest.raises(ValueError, match="with_cluster_matching"):
            call()
    assert len(uf.flipped_edges(dets)[0]) == 1  # the plain decoder keeps them
    assert not hasattr(WindowedUnionFindDecoder, "with_cluster_matching")


def test_heralds_are_refused():
    g = DecodingGraph(3, [0, 1], [1, 2], np.zeros(2, np.uint64), node_det=[0, 1], herald_det=[2], herald_ptr=[0, 1], herald_edges=[0])
    uf = UnionFindDecoder(g)
    assert uf.graph.n_heralds == 1
    with pytest.raises(NotImplementedError, match="without heralds"):
        uf.with_cluster_matching()


def test_create_matching_checks_every_argument_without_a_device():
    import ctypes as C

    from tsim_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()

    def create(n_nodes, w, K, caps=None, null_w=False):
        u = np.arange(n_nodes - 1, dtype=np.int32)
        v, obs = u + 1, np.zeros(n_nodes - 1, np.uint64)
        w = np.asarray(w, np.uint16)
        desc = _lib.UfDesc(n_nodes, len(u), n_nodes, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        rc = lib.tsim_uf_create_matching(0, C.byref(desc), None if caps is None else np.asarray(caps, np.uint8).ctypes.data_as(C.c_void_p),
                                         None if null_w else w.ctypes.data_as(C.c_void_p), K, C.byref(h))
        return rc, lib.tsim_last_error()

    ones = np.ones(69)
    for K in (0, 13, -1):
        rc, msg = create(70, ones, K)
        assert rc == -22 and b"max_defects" in msg, (rc, msg)
    rc, msg = create(70, np.where(np.arange(69) == 17, 0, 1), 10)
    assert rc == -22 and b"edge 17 has match weight 0" in msg, (rc, msg)
    rc, msg = create(70, ones, 10, null_w=True)
    assert rc == -22 and b"match_w is NULL" in msg
    rc, msg = create(70, ones, 10, caps=np.full(69, 15))
    assert rc == -22 and b"cap" in msg
    rc, msg = create(2049, np.ones(2048), 10)
    assert rc == -95 and b"2049 nodes" in msg, (rc, msg)
    g = dense_graph(31, 2048, 65535)  # within the table's limit; the weighted state (about 61 kB) and 2^12 subsets pass a block's LDS
    desc = _lib.UfDesc(2048, 65535, 2048, g.edge_u.ctypes.data, g.edge_v.ctypes.data, g.edge_obs.ctypes.data)
    caps, w = np.full(65535, 3, np.uint8), np.ones(65535, np.uint16)
    rc = lib.tsim_uf_create_matching(0, C.byref(desc), caps.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 12, C.byref(h))
    assert rc == -95 and b"bytes of LDS" in lib.tsim_last_error() and b"dynamic program" in lib.tsim_last_error()
    assert 16 + uf_shot_bytes(2048, 65535, True) <= 64 * 1024 < 16 + uf_match_shot_bytes(2048, 65535, True, 12)
    assert lib.tsim_uf_match_table(None, None, None) == -22


def test_shot_bytes():
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    for K in (1, 10, 12):
        extra = uf_match_shot_bytes(25, 78, True, K) - uf_shot_bytes(25, 78, True)
        assert extra == a16(4 << K) + a16(1 << K) + a16(2 * K) + a16(4 * K * (K + 1))
    assert 16 + uf_match_shot_bytes(25, 78, True, 12) <= 64 * 1024
