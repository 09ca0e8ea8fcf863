"""Cluster matching in windows without a device (``WindowedUnionFindDecoder.with_cluster_matching``; "Cluster matching in windows"
in the module docstring of ``tsim_amd.decode``): the local weights against a direct loop over the global edges, the windows'
tables, one window against ``UnionFindDecoder.with_cluster_matching``, paths that a window commits in part, a 64-observable
fingerprint of the committed flips against a reference written out here, unit weights, the refusals, the bytes of a shot and
the argument checks of ``tsim_ufw_create_matching`` that need no device."""

import heapq

import numpy as np
import pytest

from test_unionfind_matching import dense_graph
from test_unionfind_windowed import fire, long_memory, time_ladder

from tsim_amd.decode import (MATCH_INF, DecodingGraph, UnionFindDecoder, UnionFindWindow, WindowedUnionFindDecoder, uf_match_shot_bytes,
                             ufw_match_shot_bytes)

_CACHE: dict = {}


def d3():
    """``(circuit, its graph, the 256 syndromes of fire(g, default_rng(7), 256))`` of the d = 3, 12-round memory, built once."""
    if "d3" not in _CACHE:
        c = long_memory()
        g = UnionFindDecoder.from_circuit(c).graph
        _CACHE["d3"] = (c, g, fire(g, np.random.default_rng(7), 256))
    return _CACHE["d3"]


def fingerprint_decoder(K: int = 6) -> WindowedUnionFindDecoder:
    """The d = 3 graph with ``edge_obs`` replaced by random uint64 masks and 64 observables, in windows of 32 columns that commit
    16: a prediction names the set of committed flips."""
    _, g, _ = d3()
    obs = np.random.default_rng(64).integers(0, 1 << 63, size=g.n_edges, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    marked = DecodingGraph(g.n_nodes, g.edge_u, g.edge_v, obs, g.edge_p)
    return WindowedUnionFindDecoder(marked, 16, 32, 64).with_cluster_matching(K)


# ---- the local weights -------------------------------------------------------------------------------------------------------

def local_weights_by_a_loop(g: DecodingGraph, w: np.ndarray, win: UnionFindWindow) -> np.ndarray:
    """Per local edge of ``win`` the least ``w`` among the global edges that land on it, found edge by edge."""
    least = {}
    for e in range(g.n_edges):
        u, v = int(g.edge_u[e]), int(g.edge_v[e])
        if u == 0:
            if not win.lo <= v - 1 < win.hi:
                continue
            pair = (0, v - win.lo)
        else:
            if not win.lo <= u - 1 < win.hi:
                continue
            pair = (u - win.lo, v - win.lo) if v - 1 < win.hi else (0, u - win.lo)
        least[pair] = min(least.get(pair, 1 << 20), int(w[e]))
    pairs = list(zip(win.graph.edge_u.tolist(), win.graph.edge_v.tolist()))
    assert sorted(least) == pairs
    return np.array([least[p] for p in pairs], np.uint16)


def test_local_weights_against_a_loop_over_the_global_edges():
    c, g, _ = d3()
    wm = WindowedUnionFindDecoder.from_circuit(c, 16, 32).with_cluster_matching()
    assert np.array_equal(wm.match_weights, g.match_weights()) and wm.match_defects == 10
    ladder, caps = time_ladder(2, 6, both_ends=False, skip=True)
    lw = WindowedUnionFindDecoder(ladder, 2, 6, edge_caps=caps).with_cluster_matching(4, caps.astype(np.int64) * 100 + 1)
    merged = 0
    for dec in (wm, lw):
        for win in dec.windows():
            want = local_weights_by_a_loop(dec.graph, dec.match_weights, win)
            assert win.weights.dtype == np.uint16 and np.array_equal(win.weights, want)
            real = win.global_edge >= 0
            merged += int((win.weights[real] < dec.match_weights[win.global_edge[real]]).sum())  # a pair (0, x) lighter than its real edge
        assert dec.windows()[0].weights is not None and len(UnionFindWindow(0, 1, dec.graph, None, None, None)) == 10
    assert merged > 0
    assert WindowedUnionFindDecoder.from_circuit(c, 16, 32).windows()[0].weights is None


# ---- the windows' tables -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["d3", "ladder_units"])
def test_window_match_table(which):
    if which == "d3":
        c, g, _ = d3()
        wm = WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights="probability").with_cluster_matching(10)
    else:  # unit weights: every tie rule decides
        g, caps = time_ladder(3, 8)
        wm = WindowedUnionFindDecoder(g, 6, 12, edge_caps=caps).with_cluster_matching(10, np.ones(g.n_edges, np.int64))
    ties = 0
    for k, win in enumerate(wm.windows()):
        dist, parent = wm.window_match_table(k)
        lg, w = win.graph, win.weights.astype(np.int64)
        N = lg.n_nodes
        assert dist.dtype == np.uint32 and parent.dtype == np.uint16 and dist.shape == parent.shape == (N, N)
        whole = UnionFindDecoder(lg, wm.num_observables, None if wm.edge_caps is None else win.caps).with_cluster_matching(10, win.weights)
        assert np.array_equal(dist, whole.match_table()[0])
        d = np.where(dist == MATCH_INF, np.int64(1) << 40, dist.astype(np.int64))
        eu, ev = lg.edge_u.astype(np.int64), lg.edge_v.astype(np.int64)
        none = parent == 0xFFFF
        assert np.array_equal(none, (dist == MATCH_INF) | np.eye(N, dtype=np.bool_))
        for a in range(N):
            # the edges that attain the distance of their end v, arriving from x != 0: towards v = edge_v from edge_u, and back
            down = (eu != 0) & (d[a, eu] + w == d[a, ev]) & (d[a, ev] < 1 << 40)
            up = (d[a, ev] + w == d[a, eu]) & (d[a, eu] < 1 << 40)
            first = np.full(N, 0xFFFF, np.int64)
            for e in np.flatnonzero(down)[::-1]:
                first[ev[e]] = e
            for e in np.flatnonzero(up)[::-1]:
                first[eu[e]] = min(first[eu[e]], e)
            first[a] = 0xFFFF
            attain = np.bincount(np.concatenate([ev[down], eu[up]]), minlength=N)
            attain[a] = 0
            ties += int((attain > 1).sum())   # nodes with several edges that attain their distance: the smallest index is the parent
            assert np.array_equal(parent[a], first), (k, a)
    assert ties > 0 or which == "d3"
    with pytest.raises(IndexError):
        wm.window_match_table(len(wm.windows()))


# ---- one window --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_equals_the_whole_graph_matching_decoder(weights):
    c, g, dets = d3()
    um = UnionFindDecoder.from_circuit(c, weights=weights).with_cluster_matching(3)
    one = WindowedUnionFindDecoder.from_circuit(c, 16, 96, weights=weights).with_cluster_matching(3)
    assert len(one.windows()) == 1
    assert np.array_equal(one.predictions(dets), um.predictions(dets)) and one.predictions(dets).any()
    assert np.array_equal(one.missed(dets), um.missed(dets)) and np.array_equal(one.growth_rounds(dets), um.growth_rounds(dets))
    counts = one.match_counts(dets)
    assert counts.shape == (256, 2) and tuple(counts.sum(0)) == um.match_counts(dets) and counts[:, 1].sum() > 0


# ---- partial commits ---------------------------------------------------------------------------------------------------------

def test_paths_committed_in_part():
    c, g, dets = d3()
    differ = {}
    for weights in (None, "probability"):
        w = WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights=weights)
        wm = w.with_cluster_matching(10)
        pred = wm.predictions(dets)   # (the statement asserts a clean commit region per window and a zero final syndrome)
        assert not wm.missed(dets).any() and np.array_equal(wm.decode(dets)[:, 0], pred.astype(np.bool_))
        assert int((wm.mixed_pairs(dets) > 0).sum()) >= 5
        differ[weights] = int((pred != w.predictions(dets)).sum())
        assert wm.growth_rounds(dets).max() >= 2 and wm.windows()[1].committed.tolist() == w.windows()[1].committed.tolist()
    assert differ[None] >= 10 and differ["probability"] >= 10, differ
    matched, peeled = WindowedUnionFindDecoder.from_circuit(c, 16, 32).with_cluster_matching(2).match_counts(dets).sum(0)
    assert matched > 0 and peeled > 0
    print(f"rows that differ from windowed peeling {differ}, K = 2: {matched} matched / {peeled} peeled")


# ---- a fingerprint of the committed flips against a reference written out here --------------------------------------------------

def grown_clusters(g: DecodingGraph, defects):
    """The labels (smallest node of the cluster) when unweighted growth ends, ``None`` for a miss: the rule of the docstring, an edge
    at a time."""
    n, E = g.n_nodes, g.n_edges
    eu, ev = g.edge_u.tolist(), g.edge_v.tolist()
    grown = [0] * E
    while True:
        label = list(range(n))
        moved = True
        while moved:
            moved = False
            for e in range(E):
                if grown[e] == 2 and label[eu[e]] != label[ev[e]]:
                    label[eu[e]] = label[ev[e]] = min(label[eu[e]], label[ev[e]])
                    moved = True
        odd = [0] * n
        for v in defects:
            odd[label[v]] ^= 1
        odd[0] = 0
        if not any(odd):
            return label
        new = [min(2, grown[e] + odd[label[eu[e]]] + odd[label[ev[e]]]) for e in range(E)]
        if new == grown:
            return None
        grown = new


def dijkstra(g: DecodingGraph, w, a: int):
    """``(dist, parent edge)`` from source ``a`` by a heap; no path continues from node 0; the parent is the smallest-index edge
    ``(x, v)``, ``x != 0``, with ``dist[x] + w == dist[v]``."""
    n = g.n_nodes
    at = [[] for _ in range(n)]
    for e, (u, v) in enumerate(zip(g.edge_u.tolist(), g.edge_v.tolist())):
        at[u].append((e, v))
        at[v].append((e, u))
    dist = [None] * n
    dist[a] = 0
    heap = [(0, a)]
    while heap:
        d, v = heapq.heappop(heap)
        if d != dist[v] or v == 0:
            continue
        for e, x in at[v]:
            if dist[x] is None or d + int(w[e]) < dist[x]:
                dist[x] = d + int(w[e])
                heapq.heappush(heap, (dist[x], x))
    parent = [None] * n
    for v in range(n):
        if v != a and dist[v] is not None:
            parent[v] = min(e for e, x in at[v] if x != 0 and dist[x] is not None and dist[x] + int(w[e]) == dist[v])
    return dist, parent


def pairings(nodes):
    """Every pairing of ``nodes`` (ascending), the lowest node's partner first: the boundary (0), then the others ascending."""
    if not nodes:
        yield []
        return
    a, rest = nodes[0], nodes[1:]
    for tail in pairings(rest):
        yield [(a, 0)] + tail
    for j, b in enumerate(rest):
        for tail in pairings(rest[:j] + rest[j + 1:]):
            yield [(a, b)] + tail


def reference_row(wm: WindowedUnionFindDecoder, bits: np.ndarray, tables: dict) -> int:
    g = wm.graph
    r = bits.copy()
    pred = 0
    for k, win in enumerate(wm.windows()):
        if not r[win.lo:win.hi].any():
            continue
        lg = win.graph
        defects = (np.flatnonzero(r[win.lo:win.hi]) + 1).tolist()
        label = grown_clusters(lg, defects)
        assert label is not None
        flips = []   # a plain edge list
        peeling = None
        for root in sorted({label[v] for v in defects}):
            ds = [v for v in defects if label[v] == root]
            if len(ds) > wm.match_defects:
                if peeling is None:
                    peeling = UnionFindDecoder(lg, 64)._decode_one(np.array(defects))[2].tolist()
                flips += [e for e in peeling if label[lg.edge_v[e]] == root]
                continue
            for a in ds:
                if (k, a) not in tables:
                    tables[k, a] = dijkstra(lg, win.weights, a)
            best, cost = None, None
            for pairing in pairings(ds):   # the first of least cost
                terms = [tables[k, a][0][b] for a, b in pairing]
                if None not in terms and (cost is None or sum(terms) < cost):
                    best, cost = pairing, sum(terms)
            for a, v in best:
                while v != a:
                    e = tables[k, a][1][v]
                    flips.append(e)
                    v = int(lg.edge_u[e]) if int(lg.edge_v[e]) == v else int(lg.edge_v[e])
        for e in flips:
            if win.committed[e]:
                ge = win.global_edge[e]
                pred ^= int(g.edge_obs[ge])
                if g.edge_u[ge]:
                    r[g.edge_u[ge] - 1] ^= True
                r[g.edge_v[ge] - 1] ^= True
    assert not r.any()
    return pred


def test_a_fingerprint_of_the_committed_flips_against_an_independent_reference():
    _, _, dets = d3()
    wm = fingerprint_decoder(6)
    assert wm.num_observables == 64 and not wm.missed(dets).any()
    tables: dict = {}
    want = np.array([reference_row(wm, row, tables) for row in dets], np.uint64)
    got = wm.predictions(dets)
    assert np.array_equal(got, want)
    counts = wm.match_counts(dets).sum(0)
    assert counts[0] > 1000 and counts[1] > 0 and len(set(got.tolist())) > 200   # (the masks tell the sets of flips apart)


def test_unit_weights_where_every_tie_rule_decides():
    """With ``weights = 1`` everywhere the distances tie all the time: parents, pairs and the reference must break every tie alike."""
    _, g, dets = d3()
    fp = fingerprint_decoder(6)
    wm = WindowedUnionFindDecoder(fp.graph, 16, 32, 64).with_cluster_matching(6, np.ones(g.n_edges, np.int64))
    tables: dict = {}
    want = np.array([reference_row(wm, row, tables) for row in dets[:96]], np.uint64)
    assert np.array_equal(wm.predictions(dets[:96]), want)
    assert (wm.predictions(dets[:96]) != fp.predictions(dets[:96])).any()


# ---- the refusals, the bytes of a shot, the create call's checks ----------------------------------------------------------------

def test_refusals():
    c, g, dets = d3()
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32)
    wm = w.with_cluster_matching()
    assert not hasattr(WindowedUnionFindDecoder, "with_cluster_matching") and w.match_defects is None and w.match_weights is None
    for bad in (0, 13, 2.0, True):
        with pytest.raises(ValueError, match="max_defects"):
            w.with_cluster_matching(bad)
    with pytest.raises(ValueError, match="match weight 0"):
        w.with_cluster_matching(weights=np.zeros(g.n_edges, np.int64))
    with pytest.raises(ValueError, match="match weight 65536"):
        w.with_cluster_matching(weights=np.full(g.n_edges, 65536))
    with pytest.raises(ValueError, match="shape"):
        w.with_cluster_matching(weights=np.ones(g.n_edges - 1, np.int64))
    with pytest.raises(ValueError, match="takes no cluster matching"):
        w.with_soft_output("rounds").with_cluster_matching()
    with pytest.raises(ValueError, match="no soft output"):
        wm.with_soft_output("rounds")
    with pytest.raises(ValueError, match="no soft outputs"):
        wm.soft_outputs(dets)
    with pytest.raises(ValueError, match="no flipped edges"):
        wm.flipped_edges(dets)
    for call in (lambda: w.window_match_table(0), lambda: w.match_counts(dets)):
        with pytest.raises(ValueError, match="with_cluster_matching"):
            call()
    assert len(w.flipped_edges(dets)) == 256 and w.soft_outputs(dets).shape == (256, 4)   # the plain decoder keeps them
    hg = DecodingGraph(3, [0, 1], [1, 2], np.zeros(2, np.uint64), node_det=[0, 1], herald_det=[2], herald_ptr=[0, 1], herald_edges=[0])
    with pytest.raises(NotImplementedError, match="without heralds"):
        WindowedUnionFindDecoder(hg, 1, 2, heralds=True).with_cluster_matching()
    chain = DecodingGraph(5001, np.arange(5000), np.arange(5000) + 1, np.zeros(5000, np.uint64), limit=None)
    with pytest.raises(NotImplementedError, match="a window of 2101 nodes"):
        WindowedUnionFindDecoder(chain, 2000, 2100).with_cluster_matching()


def test_shot_bytes():
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    for K, window, words in ((1, 20, 1), (10, 32, 1), (12, 33, 2), (10, 1000, 32)):
        extra = ufw_match_shot_bytes(65, 300, True, K, window) - uf_match_shot_bytes(65, 300, True, K)
        assert extra == a16(4 * K) + a16(4 * words) + 16
    shot = ufw_match_shot_bytes(65, 459, True, 12, 64)   # K = 12: the 2^12 subsets leave two shots to a block, K = 10 four
    assert 16 + 2 * shot <= 64 * 1024 < 16 + 3 * shot and 16 + 4 * ufw_match_shot_bytes(65, 459, True, 10, 64) <= 64 * 1024


def test_create_matching_checks_every_argument_without_a_device():
    import ctypes as C

    from tsim_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()

    def create(n_nodes, w, K, commit, window, caps=None, null_w=False):
        u = np.arange(n_nodes - 1, dtype=np.int32)
        v, obs = u + 1, np.zeros(n_nodes - 1, np.uint64)
        w = np.asarray(w, np.uint16)
        desc = _lib.UfDesc(n_nodes, len(u), n_nodes, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        rc = lib.tsim_ufw_create_matching(0, C.byref(desc), None if caps is None else np.asarray(caps, np.uint8).ctypes.data_as(C.c_void_p),
                                          None if null_w else w.ctypes.data_as(C.c_void_p), K, commit, window, C.byref(h))
        return rc, lib.tsim_last_error()

    ones = np.ones(69)
    for K in (0, 13, -1):
        rc, msg = create(70, ones, K, 8, 16)
        assert rc == -22 and b"max_defects" in msg, (rc, msg)
    rc, msg = create(70, np.where(np.arange(69) == 17, 0, 1), 10, 8, 16)
    assert rc == -22 and b"edge 17 has match weight 0" in msg, (rc, msg)
    rc, msg = create(70, ones, 10, 8, 16, null_w=True)
    assert rc == -22 and b"match_w is NULL" in msg
    rc, msg = create(70, ones, 10, 8, 16, caps=np.full(69, 15))
    assert rc == -22 and b"cap" in msg
    rc, msg = create(70, ones, 10, 16, 16)
    assert rc == -22 and b"commit" in msg
    rc, msg = create(5001, np.ones(5000), 10, 2000, 2100)
    assert rc == -95 and b"a window of 2101 nodes" in msg, (rc, msg)
    # 51 windows of 2048 nodes whose weights differ: 51 * 2048^2 * 6 bytes pass 1 GiB; with equal weights the bulk windows share one table
    n = 2000 * 50 + 2047 + 1
    rc, msg = create(n, np.arange(n - 1) % 65521 + 1, 10, 2000, 2047)
    assert rc == -95 and b"distinct windows" in msg, (rc, msg)
    g = dense_graph(31, 2048, 65535)  # one window within the table's limit whose weighted state and 2^12 subsets pass a block's LDS
    desc = _lib.UfDesc(2048, 65535, 2048, g.edge_u.ctypes.data, g.edge_v.ctypes.data, g.edge_obs.ctypes.data)
    caps, w = np.full(65535, 3, np.uint8), np.ones(65535, np.uint16)
    rc = lib.tsim_ufw_create_matching(0, C.byref(desc), caps.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 12, 1, 4096, C.byref(h))
    assert rc == -95 and b"bytes of LDS" in lib.tsim_last_error() and b"dynamic program" in lib.tsim_last_error()
    assert lib.tsim_ufw_match_table(None, 0, None, None) == -22 and lib.tsim_ufw_match_info(None, None) == -22
