"""Cluster matching and the complementary gap under heralded erasures, without a device ("Cluster matching under heralds" in
the module docstring of ``tsim_amd.decode``): hand-made chains, the hub graph against a Dijkstra over the whole graph under the
lowered weights, the two programs against an enumeration of all pairings, the reduction to ``with_cluster_matching`` where no
herald is set, growth and misses against the plain herald decoder, the two limits K and H, the cost invariants on decoded rows,
the decoded errors against peeling, the gap against ``largest_cluster`` as a rejection signal, and what is refused."""

import ctypes as C
import heapq

import numpy as np
import pytest

from test_unionfind_erasure import erasure_memory
from test_unionfind_large import sparse_graph

from tsim_amd import _lib
from tsim_amd.backend import HipProgram
from tsim_amd.decode import (MATCH_INF, MAX_MATCH_NODES, DecodingGraph, UnionFindDecoder, uf_erasure_shot_bytes, uf_match_shot_bytes)


def with_heralds(g: DecodingGraph, lists, edge_p=None) -> DecodingGraph:
    """``g`` with one herald per entry of ``lists`` (the edges it lists), the herald columns after the nodes' columns."""
    n = g.n_nodes - 1
    return DecodingGraph(g.n_nodes, g.edge_u, g.edge_v, g.edge_obs, g.edge_p if edge_p is None else edge_p, node_det=np.arange(n),
                         herald_det=n + np.arange(len(lists)), herald_ptr=np.cumsum([0] + [len(x) for x in lists]),
                         herald_edges=np.array([e for x in lists for e in sorted(x)], np.int64))


def without_heralds(g: DecodingGraph) -> DecodingGraph:
    return DecodingGraph(g.n_nodes, g.edge_u, g.edge_v, g.edge_obs, g.edge_p)


def inner_chain(obs_far: int = 1) -> DecodingGraph:
    """boundary - 1 - 2 - 3 - 4 - boundary; the boundary edges (0, 1) and (0, 4) flip observable 0 (``obs_far``: whether (0, 4)
    does); one herald lists the three inner edges.  Edges: (0, 1), (0, 4), (1, 2), (2, 3), (3, 4)."""
    g = DecodingGraph(5, [0, 0, 1, 2, 3], [1, 4, 2, 3, 4], np.array([1, obs_far, 0, 0, 0], np.uint64))
    return with_heralds(g, [[2, 3, 4]])


INNER_W = np.array([10, 10, 100, 100, 100])   # cheap boundary edges, expensive inner edges


def long_chain(n_nodes: int = 10) -> DecodingGraph:
    """0 - 1 - ... - 9 with the boundary at one end only; edge (0, 1) flips observable 0; one herald lists every inner edge."""
    u = np.arange(n_nodes - 1)
    obs = np.zeros(n_nodes - 1, np.uint64)
    obs[0] = 1
    return with_heralds(DecodingGraph(n_nodes, u, u + 1, obs), [list(range(1, n_nodes - 1))])


def row_of(g: DecodingGraph, defects=(), heralds=()) -> np.ndarray:
    """One detector row bool ``[1, num_detectors]`` with the defect NODES and the heralds set."""
    row = np.zeros((1, g.num_detectors), np.bool_)
    row[0, g.node_det[np.asarray(defects, np.int64) - 1]] = True
    row[0, g.herald_det[np.asarray(heralds, np.int64)]] = True
    return row


_CASES: dict = {}


def d3_case(p: float = 3e-3, pe: float = 1e-2, n: int = 40000):
    """``(circuit, peeling decoder, erasure-matching decoder, the same with the gap of observable 0, rows bool [n, 169])`` of the
    issue's settings: d = 3, 3 rounds, weighted growth at resolution 4, K = 10, erased weight 1, rows of ``method="faults"`` under
    seed 5.  Built once: the decoders cache the rows they have decoded."""
    if (p, pe, n) not in _CASES:
        c = erasure_memory(3, 3, p, pe)
        uf = UnionFindDecoder.from_circuit(c, weights="probability", resolution=4, heralds=True)
        ue = uf.with_erasure_matching(max_defects=10, erased_weight=1)
        rows = c.compile_detector_sampler(seed=5, method="faults").sample(n, append_observables=True).astype(np.bool_)
        rows.setflags(write=False)
        _CASES[p, pe, n] = (c, uf, ue, ue.with_gap_output(0), rows)
    return _CASES[p, pe, n]


def wrong_rows(dec, rows) -> np.ndarray:
    nd = dec.num_detectors
    return (dec.decode(rows[:, :nd]) != rows[:, nd:]).any(axis=1)


# ---- hand graphs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("obs_far", [1, 0])
def test_erased_inner_path_beats_two_cheap_boundary_edges(obs_far):
    g = inner_chain(obs_far)
    uf = UnionFindDecoder(g)
    ue = uf.with_erasure_matching(weights=INNER_W)
    ug = ue.with_gap_output(0, cap=1000)
    static = UnionFindDecoder(without_heralds(g)).with_cluster_matching(weights=INNER_W)
    assert static._match_cluster([1, 4])[:2] == (20, 1 ^ obs_far)   # the static tables send both defects to the boundary
    set_row, clear_row = row_of(g, [1, 4], [0]), row_of(g, [1, 4])
    hub = ue.hub_graph([1, 4], [2, 3, 4])
    assert hub["hubs"].tolist() == [1, 4, 2, 3] and hub["D"][0, 1] == 3 and hub["M"][0, 1] == 0 and hub["b"].tolist() == [10, 10]
    assert ue._hub_cluster([1, 4], [2, 3, 4])[:2] == (3, 0)
    assert ue.predictions(set_row).tolist() == [0]   # the inner path: no observable flip
    assert ue.match_counts(set_row) == (1, 0) and ue.erasure_counts(set_row) == (1, 0)
    assert ug.predictions(set_row).tolist() == [0]
    if obs_far == 0:   # the other class: both defects to the boundary, 20 against 3
        assert ug.gap_outputs(set_row).tolist() == [1000 - 17]
    # with the herald clear every number is with_cluster_matching's on the same arrays
    ugs = static.with_gap_output(0, cap=1000)
    for defects in ([1, 4], [1], [2, 3], [1, 2, 3, 4], [3]):
        row = row_of(g, defects)
        assert ue.predictions(row).tolist() == static.predictions(row[:, :4]).tolist()
        assert ug.gap_outputs(row).tolist() == ugs.gap_outputs(row[:, :4]).tolist()
        assert ue.match_counts(row) == static.match_counts(row[:, :4]) and ue.erasure_counts(row) == (0, 0)
    assert ue.predictions(clear_row).tolist() == [1 ^ obs_far]


def test_erased_weight_is_a_ceiling_not_a_floor():
    """``min(w[e], w_h)``: an erased edge never gets heavier, and ``w_h = 65535`` leaves every weight what it is."""
    g = inner_chain(0)
    ue = UnionFindDecoder(g).with_erasure_matching(weights=INNER_W, erased_weight=65535)
    assert ue._hub_cluster([1, 4], [2, 3, 4])[:2] == (20, 1)
    light = UnionFindDecoder(g).with_erasure_matching(weights=np.array([10, 10, 1, 1, 1]), erased_weight=5)
    assert light.hub_graph([1, 4], [2, 3, 4])["D"][0, 1] == 3
    mid = UnionFindDecoder(g).with_erasure_matching(weights=INNER_W, erased_weight=7)   # 21 > 20: the boundary wins again
    assert mid._hub_cluster([1, 4], [2, 3, 4])[:2] == (20, 1)
    # an erased boundary edge: (0, 1) erased at weight 1 shortens defect 4's way out only through the hubs
    both = with_heralds(without_heralds(g), [[0, 2, 3, 4]])
    ub = UnionFindDecoder(both).with_erasure_matching(weights=INNER_W)
    h = ub.hub_graph([4], [0, 2, 3, 4])
    assert h["hubs"].tolist() == [4, 1, 2, 3] and h["B"].tolist() == [10, 1, 110, 110] and h["b"].tolist() == [4] and h["mb"].tolist() == [1]


# ---- the hub graph against a Dijkstra over the whole graph -------------------------------------------------------------------

def dijkstra_classes(g: DecodingGraph, w, k: int, source: int) -> np.ndarray:
    """int64 ``[N, 2]``: the least weight of a walk from ``source`` to every node per class of observable ``k``, never continuing
    from node 0 (``MATCH_INF``: none), by a heap over the states (node, class)."""
    adj = [[] for _ in range(g.n_nodes)]
    for e, (u, v) in enumerate(zip(g.edge_u.tolist(), g.edge_v.tolist())):
        c = int(g.edge_obs[e] >> np.uint64(k)) & 1
        adj[u].append((v, int(w[e]), c))
        adj[v].append((u, int(w[e]), c))
    d = np.full((g.n_nodes, 2), MATCH_INF, np.int64)
    d[source, 0] = 0
    heap = [(0, source, 0)]
    while heap:
        dv, v, b = heapq.heappop(heap)
        if dv > d[v, b] or v == 0:
            continue
        for x, wx, c in adj[v]:
            if dv + wx < d[x, b ^ c]:
                d[x, b ^ c] = dv + wx
                heapq.heappush(heap, (dv + wx, x, b ^ c))
    return d


@pytest.mark.parametrize("seed", range(6))
def test_hub_graph_equals_dijkstra_under_the_lowered_weights(seed):
    rng = np.random.default_rng(100 + seed)
    base = sparse_graph(20 + seed, 60, 110, 5)
    lists = [rng.choice(base.n_edges, size=rng.integers(1, 4), replace=False).tolist() for _ in range(30)]
    g = with_heralds(base, lists)
    w = rng.integers(1, 50 if seed % 2 else 3000, size=g.n_edges)
    w_h = int(rng.integers(1, 40))
    ug = UnionFindDecoder(g).with_erasure_matching(12, w, erased_weight=w_h, max_hubs=32).with_gap_output(seed % 2, cap=77)
    checked = lowered = odd = 0
    for _ in range(25):
        erased = np.unique(np.concatenate([lists[h] for h in rng.choice(30, size=rng.integers(1, 6), replace=False)]))
        ends = np.union1d(g.edge_u[erased], g.edge_v[erased])
        ends = ends[ends >= 1]
        some = rng.choice(np.arange(1, g.n_nodes), size=rng.integers(1, 5), replace=False)
        defects = np.unique(np.concatenate([some, rng.choice(ends, size=min(len(ends), 2), replace=False)]))
        if len(np.union1d(defects, ends)) > 32:
            continue
        hub = ug.hub_graph(defects, erased)
        hubs = hub["hubs"]
        assert hubs[:len(defects)].tolist() == defects.tolist() and hubs[len(defects):].tolist() == np.setdiff1d(ends, defects).tolist()
        w2 = w.copy()
        w2[erased] = np.minimum(w2[erased], w_h)
        for i, a in enumerate(hubs):
            d2 = dijkstra_classes(g, w2, ug.gap_observable, int(a))
            assert np.array_equal(hub["D2"][i], d2[hubs]), (seed, i)
            assert np.array_equal(hub["D"][i], d2[hubs].min(axis=1))
            if i < len(defects):
                assert np.array_equal(hub["b2"][i], d2[0]) and hub["b"][i] == d2[0].min()
        static = ug.match_table()[0]
        lowered += int((hub["D"] < static[np.minimum.outer(hubs, hubs), np.maximum.outer(hubs, hubs)]).sum())
        odd += int(((hub["D2"] != MATCH_INF).all(axis=2) & (hub["D2"][:, :, 0] != hub["D2"][:, :, 1])).sum())
        checked += 1
    assert checked >= 20 and lowered > 50 and odd > 50


# ---- the two programs against every pairing ----------------------------------------------------------------------------------

def all_pairings(items):
    """Every way to pair the items off, an item alone standing for a match to the boundary: lists of ``(i, j)`` / ``(i, None)``."""
    if not items:
        yield []
        return
    i, rest = items[0], items[1:]
    for tail in all_pairings(rest):
        yield [(i, None)] + tail
    for k, j in enumerate(rest):
        for tail in all_pairings(rest[:k] + rest[k + 1:]):
            yield [(i, j)] + tail


@pytest.mark.parametrize("seed", range(4))
def test_programs_equal_an_enumeration_of_all_pairings(seed):
    rng = np.random.default_rng(seed)
    base = sparse_graph(50 + seed, 60, 160, 8)
    lists = [rng.choice(base.n_edges, size=2, replace=False).tolist() for _ in range(20)]
    g = with_heralds(base, lists)
    ug = UnionFindDecoder(g).with_erasure_matching(6, rng.integers(1, 9, size=g.n_edges), 2, 32).with_gap_output(0, cap=50)
    sizes = set()
    for m in (1, 2, 3, 4, 5, 6, 6, 5):
        erased = np.unique(np.concatenate([lists[h] for h in rng.choice(20, size=3, replace=False)]))
        defects = np.sort(rng.choice(np.arange(1, 56), size=m, replace=False))
        hub = ug.hub_graph(defects, erased)
        D, b, D2, b2 = hub["D"], hub["b"], hub["D2"], hub["b2"]
        cost, mask, pairs = ug._pair_program(m, lambda i, j: (int(b[i]), int(hub["mb"][i])) if j is None else (int(D[i, j]), int(hub["M"][i, j])))
        classes = ug._class_program(m, lambda i, j: b2[i] if j is None else D2[i, j])
        best, best_class = None, [None, None]
        for pairing in all_pairings(list(range(m))):
            terms = [b[i] if j is None else D[i, j] for i, j in pairing]
            if all(t != MATCH_INF for t in terms) and (best is None or sum(terms) < best):
                best = int(sum(terms))
            terms2 = [b2[i] if j is None else D2[i, j] for i, j in pairing]
            for pick in range(1 << len(pairing)):   # the class of every path of the pairing
                t = [int(terms2[x][(pick >> x) & 1]) for x in range(len(pairing))]
                cl = bin(pick).count("1") & 1
                if all(x != MATCH_INF for x in t) and (best_class[cl] is None or sum(t) < best_class[cl]):
                    best_class[cl] = sum(t)
        assert cost == best and tuple(classes) == tuple(best_class)
        if cost is not None:   # (a sparse random graph may leave a defect without a partner or a way out)
            assert sum((b[i] if j is None else D[i, j]) for i, j in pairs) == cost
            sizes.add(m)
    assert sizes >= {2, 4, 6}


# ---- the reduction, growth and misses ----------------------------------------------------------------------------------------

def test_rows_without_a_herald_equal_cluster_matching_on_the_herald_free_graph():
    _, uf, ue, ug, rows = d3_case()
    g = ue.graph
    dets = rows[:3000, :ue.num_detectors].copy()
    dets[:, g.herald_det] = False
    plain = UnionFindDecoder(without_heralds(g), ue.num_observables, ue.edge_caps)
    um = plain.with_cluster_matching(10, ue.match_weights)
    um_g = um.with_gap_output(0)
    nodes = dets[:, g.node_det]
    assert np.array_equal(ue.predictions(dets), um.predictions(nodes)) and ue.predictions(dets).any()
    assert np.array_equal(ug.predictions(dets), um_g.predictions(nodes))
    assert (ug.gap_cap, ug.gap_step) == (um_g.gap_cap, um_g.gap_step)
    assert np.array_equal(ug.gap_outputs(dets), um_g.gap_outputs(nodes)) and len(np.unique(ug.gap_outputs(dets))) > 5
    assert ue.match_counts(dets) == um.match_counts(nodes) and ue.erasure_counts(dets) == (0, 0)
    assert np.array_equal(ue.match_table()[0], um.match_table()[0]) and np.array_equal(ug.gap_table()[0], um_g.gap_table()[0])


def test_growth_and_misses_are_the_plain_herald_decoders():
    _, uf, ue, ug, rows = d3_case()
    dets = rows[:3000, :ue.num_detectors]
    assert np.array_equal(ue.growth_rounds(dets), uf.growth_rounds(dets)) and not ue.missed(dets).any()
    # an island without a boundary edge: a single defect there is a miss, predicts 0 and has gap 0, herald or not
    island = DecodingGraph(6, [0, 1, 3, 4], [1, 2, 4, 5], np.array([1, 1, 2, 0], np.uint64), node_det=np.arange(5), herald_det=[5, 6],
                           herald_ptr=[0, 1, 3], herald_edges=[2, 0, 1])
    uf2 = UnionFindDecoder(island)
    ue2 = uf2.with_erasure_matching(weights=np.array([3, 4, 5, 6]))
    ug2 = ue2.with_gap_output(0, cap=9)
    for defects, heralds in (([3], [0]), ([5], []), ([1, 4], [0, 1]), ([3, 4], [0]), ([2], [1])):
        row = row_of(island, defects, heralds)
        assert ue2.missed(row).tolist() == uf2.missed(row).tolist() and ue2.growth_rounds(row).tolist() == uf2.growth_rounds(row).tolist()
        if uf2.missed(row)[0]:
            assert ue2.predictions(row).tolist() == [0] and ug2.gap_outputs(row).tolist() == [9] and ue2.match_counts(row) == (0, 0)
    assert uf2.missed(row_of(island, [3], [0]))[0] and not uf2.missed(row_of(island, [3, 4], [0]))[0]
    assert ue2.predictions(row_of(island, [3, 4], [0])).tolist() == [2]   # the erased edge (3, 4), inside the island


# ---- the limits K and H ------------------------------------------------------------------------------------------------------

def test_max_hubs_and_max_defects_are_sharp():
    g = long_chain()   # the herald joins 1 .. 9 into one cluster: defects 1 and 9 make 9 hubs
    uf = UnionFindDecoder(g)
    row = row_of(g, [1, 9], [0])
    w = np.full(9, 100)
    fits, over = uf.with_erasure_matching(2, w, 1, max_hubs=9), uf.with_erasure_matching(2, w, 1, max_hubs=8)
    assert fits.match_counts(row) == (1, 0) and fits.erasure_counts(row) == (1, 0)
    assert over.match_counts(row) == (0, 1) and over.erasure_counts(row) == (0, 1)   # n = H + 1: peeled, and counted
    assert fits.hub_graph([1, 9], range(1, 9))["D"][0, 1] == 8
    assert fits.predictions(row).tolist() == [0] and over.predictions(row).tolist() == uf.predictions(row).tolist()
    assert over.with_gap_output(0, cap=50).gap_outputs(row).tolist() == [50] and fits.with_gap_output(0, cap=50).gap_outputs(row).tolist() == [50 - 50]
    three = row_of(g, [2, 5, 9], [0])
    k3, k2 = uf.with_erasure_matching(3, w, 1, 9), uf.with_erasure_matching(2, w, 1, 9)
    assert k3.match_counts(three) == (1, 0) and k2.match_counts(three) == (0, 1) and k2.erasure_counts(three) == (0, 0)
    assert k3.predictions(three).tolist() == [1]   # 5 - 9 over four erased edges, 2 out over the erased (1, 2) and the real (0, 1): 105
    assert k2.predictions(three).tolist() == uf.predictions(three).tolist()


# ---- decoded rows ------------------------------------------------------------------------------------------------------------

def test_cost_invariants_hold_on_every_cluster_of_decoded_rows():
    """``min(g)`` is the winner's cost and the cheaper class the winner's: asserted by the statement on every matched cluster;
    here they are counted, and the reduction's assertion with them."""
    _, uf, ue, ug, rows = d3_case()
    fresh = ue.with_gap_output(0, bins=32)   # (a cache of its own: every cluster runs here)
    seen = []
    inner = fresh._gap_of_classes
    fresh._gap_of_classes = lambda classes, cost, mask: seen.append((classes, cost, mask)) or inner(classes, cost, mask)
    dets = rows[:4000, :ue.num_detectors]
    fresh.predictions(dets)
    matched, peeled = fresh.match_counts(dets)
    erased, overflowed = fresh.erasure_counts(dets)
    print(f"4000 rows: {len(seen)} programs run, {matched} clusters matched, {erased} of them with an erased edge, {peeled} peeled")
    assert len(seen) >= 1000 and erased > 300 and overflowed == 0
    assert all(min(x for x in g if x is not None) == cost for g, cost, _ in seen)
    assert sum(1 for g, _, _ in seen if None not in g and g[0] != g[1]) > 500


def test_decoded_errors_are_at_most_peelings():
    _, uf, ue, ug, rows = d3_case()
    peeling, hub = int(wrong_rows(uf, rows).sum()), int(wrong_rows(ue, rows).sum())
    print(f"d = 3, p = 3e-3, pe = 1e-2, {len(rows)} rows: peeling {peeling} decoded errors, the hub rule {hub}")
    assert peeling == 399   # the rows of the issue's table
    assert hub <= peeling
    assert np.array_equal(ug.predictions(rows[:, :ue.num_detectors]), ue.predictions(rows[:, :ue.num_detectors]))


def test_gap_rejects_better_than_largest_cluster():
    """Errors left among the kept rows, at 90 % or more kept: rows are accepted in the order of their soft value, a whole value
    at a time, up to the first value at which at least 90 % are in."""
    _, uf, ue, ug, rows = d3_case(n=20000)
    dets = rows[:, :ue.num_detectors]

    def left(values, wrong):
        for t in np.unique(values):
            if (values <= t).sum() >= 0.9 * len(values):
                return int(wrong[values <= t].sum()), int((values <= t).sum())

    by_gap = left(ug.gap_outputs(dets), wrong_rows(ug, rows))
    by_cluster = left(uf.soft_outputs(dets)[:, 2], wrong_rows(uf, rows))
    print(f"{len(rows)} rows: by the gap {by_gap[0]} errors among {by_gap[1]} kept, by largest_cluster {by_cluster[0]} among {by_cluster[1]}")
    assert by_gap[0] <= by_cluster[0]


# ---- what is refused ---------------------------------------------------------------------------------------------------------

def test_refusals():
    g = inner_chain()
    uf = UnionFindDecoder(g)
    for bad in (0, 13, 2.0, True):
        with pytest.raises(ValueError, match="max_defects"):
            uf.with_erasure_matching(bad)
    for bad in (0, 65536, 1.0, False):
        with pytest.raises(ValueError, match="erased_weight"):
            uf.with_erasure_matching(erased_weight=bad)
    for K, H in ((10, 9), (10, 33), (1, 0), (2, 2.0)):
        with pytest.raises(ValueError, match="max_hubs"):
            uf.with_erasure_matching(K, max_hubs=H)
    with pytest.raises(ValueError, match="with_cluster_matching"):
        UnionFindDecoder(without_heralds(g)).with_erasure_matching()
    with pytest.raises(ValueError, match="match weight 0"):
        uf.with_erasure_matching(weights=np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="shape"):
        uf.with_erasure_matching(weights=np.ones(4, np.int64))
    with pytest.raises(ValueError, match="takes no cluster matching"):
        uf.with_soft_output("rounds").with_erasure_matching()
    big = with_heralds(DecodingGraph(MAX_MATCH_NODES + 1, np.arange(MAX_MATCH_NODES), np.arange(MAX_MATCH_NODES) + 1,
                                     np.zeros(MAX_MATCH_NODES, np.uint64)), [[0]])
    with pytest.raises(NotImplementedError, match="2049 nodes"):
        UnionFindDecoder(big).with_erasure_matching()
    ue = uf.with_erasure_matching()
    assert (ue.match_defects, ue.erased_weight, ue.max_hubs) == (10, 1, 24) and ue.gap_observable is None
    with pytest.raises(ValueError, match="no soft output"):
        ue.with_soft_output("rounds")
    with pytest.raises(ValueError, match="no flipped edges"):
        ue.flipped_edges(row_of(g, [1]))
    with pytest.raises(NotImplementedError, match="without heralds"):
        uf.with_cluster_matching()   # (unchanged: the static decoder keeps refusing a herald graph)
    for call in (lambda: uf.hub_graph([1], []), lambda: uf.erasure_counts(row_of(g, [1]))):
        with pytest.raises(ValueError, match="with_erasure_matching"):
            call()
    with pytest.raises(ValueError, match="observable"):
        ue.with_gap_output(1)
    ug = UnionFindDecoder(inner_chain(0)).with_erasure_matching().with_gap_output(0, bins=8)   # (one odd boundary edge: a W0 exists)
    assert (ug.soft_output, ug.soft_bins, ug.erased_weight, ug.max_hubs) == ("gap", 8, 1, 24) and ug.gap_cap == ug.gap_table()[1]


def test_create_matching_heralds_checks_every_argument_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    g = inner_chain()

    def create(graph=g, w=(1, 1, 1, 1, 1), K=10, w_h=1, H=24, observable=-1, her=True, null_w=False, caps=None):
        desc, d_caps, heralds, keep = HipProgram._uf_graph_args(graph, graph.num_detectors + 1, caps)
        w = np.asarray(w, np.uint16)
        rc = lib.tsim_uf_create_matching_heralds(0, C.byref(desc), d_caps, C.byref(heralds) if her and heralds is not None else None,
                                                 None if null_w else w.ctypes.data_as(C.c_void_p), K, w_h, H, observable, C.byref(h))
        return rc, lib.tsim_last_error()

    for kw, code, what in ((dict(K=0), -22, b"max_defects"), (dict(K=13), -22, b"max_defects"), (dict(w_h=0), -22, b"erased_w"),
                           (dict(w_h=65536), -22, b"erased_w"), (dict(K=10, H=9), -22, b"max_hubs"), (dict(H=33), -22, b"max_hubs"),
                           (dict(observable=-2), -22, b"observable"), (dict(observable=64), -22, b"observable"),
                           (dict(her=False), -22, b"her is NULL"), (dict(null_w=True), -22, b"match_w is NULL"),
                           (dict(w=(1, 1, 0, 1, 1)), -22, b"edge 2 has match weight 0"), (dict(caps=np.full(5, 15)), -22, b"cap"),
                           (dict(graph=without_heralds(g)), -22, b"her is NULL"),
                           # both programs at K = 12 and 32 hubs with their classes: 52 kB and 20 kB
                           (dict(K=12, H=32, observable=0), -95, b"hub graph of max_hubs")):
        rc, msg = create(**kw)
        assert rc == code and what in msg, (kw, rc, msg)
        assert h.value is None
    bad = DecodingGraph(5, g.edge_u, g.edge_v, g.edge_obs, node_det=np.arange(4), herald_det=[4], herald_ptr=[0, 3], herald_edges=[2, 3, 4])
    bad.herald_edges = np.array([2, 3, 5], np.int32)
    rc, msg = create(graph=bad)
    assert rc == -22 and b"herald_edges[2] = 5" in msg
    n = MAX_MATCH_NODES + 1
    big = with_heralds(DecodingGraph(n, np.arange(n - 1), np.arange(n - 1) + 1, np.zeros(n - 1, np.uint64)), [[0]])
    rc, msg = create(graph=big, w=np.ones(n - 1))
    assert rc == -95 and b"2049 nodes" in msg
    out = (C.c_int64 * 4)()
    assert lib.tsim_uf_erasure_info(None, out) == -22 and lib.tsim_uf_erasure_info(None, None) == -22


def test_shot_bytes():
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    for K, H, gap in ((1, 1, False), (10, 24, False), (10, 24, True), (12, 32, False), (4, 12, True)):
        extra = uf_erasure_shot_bytes(25, 78, True, K, H, gap) - uf_match_shot_bytes(25, 78, True, K, gap)
        assert extra == a16(4 * 3) + a16(2 * H) + a16(4 * H * H) + a16(8 * H * H) + a16(4 * H) + a16(8 * H) + a16(8 * K) + (a16(8 * H * H) + a16(8 * H) if gap else 0)
    assert 16 + uf_erasure_shot_bytes(25, 78, True, 12, 32) <= 64 * 1024 < 16 + uf_erasure_shot_bytes(25, 78, True, 12, 32, True)
    assert 16 + uf_erasure_shot_bytes(1321, 10000, True, 10, 24, True) <= 64 * 1024   # d = 11, 11 rounds, at the defaults
