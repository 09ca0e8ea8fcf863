"""The complementary gap of the cluster-matching union-find decoder without a device ("Complementary gap" in the module docstring
of ``tsim_amd.decode``): the class table against a heap Dijkstra over the doubled graph, ``W0``, the class program against an
enumeration of every pairing and class choice, its two cost invariants on decoded rows, the rules of a row, the counts of
``soft_bin_counts`` and ``tally_rows``, that the gap removes errors at least as well as ``largest_cluster`` did, and what is
refused."""

import ctypes as C
import heapq
import itertools

import numpy as np
import pytest

from test_unionfind import chain_graph
from test_unionfind_matching import all_pairings, chain_rows, matching_decoder, surface_sample, table_cases, two_boundary_graph

from tsim_amd import _lib
from tsim_amd.counts import tally_rows
from tsim_amd.decode import MATCH_INF, SOFT_OUTPUTS, UnionFindDecoder, WindowedUnionFindDecoder, uf_match_shot_bytes, uf_shot_bytes


def gap_decoder(graph, weights, K: int = 10, observable: int = 0, **kw) -> UnionFindDecoder:
    return matching_decoder(graph, weights, K).with_gap_output(observable, **kw)


def doubled_dijkstra(graph, w, k: int) -> np.ndarray:
    """``dist2`` by a heap Dijkstra per source over the states ``(node, class)``; no state of node 0 is expanded."""
    N = graph.n_nodes
    adj = [[] for _ in range(N)]
    for e, (u, v) in enumerate(zip(graph.edge_u.tolist(), graph.edge_v.tolist())):
        c = (int(graph.edge_obs[e]) >> k) & 1
        adj[u].append((v, int(w[e]), c))
        adj[v].append((u, int(w[e]), c))
    out = np.full((N, N, 2), MATCH_INF, np.int64)
    for a in range(N):
        d = out[a]
        d[a, 0] = 0
        heap = [(0, a, 0)]
        while heap:
            dv, v, b = heapq.heappop(heap)
            if dv > d[v, b] or v == 0:
                continue
            for x, we, c in adj[v]:
                if dv + we < d[x, b ^ c]:
                    d[x, b ^ c] = dv + we
                    heapq.heappush(heap, (dv + we, x, b ^ c))
    return out.astype(np.uint32)


# ---- the class table ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(table_cases()))
def test_gap_table_equals_a_heap_dijkstra_over_the_doubled_graph(name):
    graph, w = table_cases()[name]
    um = matching_decoder(graph, w)
    n_obs = um.num_observables
    assert n_obs == 2 or name == "chain70"
    for k in range(n_obs):
        if name == "chain70" and k == 0:
            ug = um.with_gap_output(0, cap=1000)  # (a chain has no W0)
        else:
            ug = um.with_gap_output(k)
        dist2, w0 = ug.gap_table()
        assert ug.gap_table()[0] is dist2  # cached
        assert dist2.dtype == np.uint32 and dist2.shape == (graph.n_nodes, graph.n_nodes, 2)
        assert np.array_equal(dist2, doubled_dijkstra(graph, w, k))
        assert np.array_equal(dist2.min(axis=2), um.match_table()[0])  # the cheaper class is the match table's distance
        assert dist2[0, 0, 0] == 0 and (dist2[0].reshape(-1)[1:] == MATCH_INF).all()
        finite = dist2[dist2 != MATCH_INF]
        assert finite.max() < (2 * graph.n_nodes - 1) * 65535
        col = dist2[1:, 0].astype(np.int64)
        both = (col != MATCH_INF).all(axis=1)
        assert w0 == (int(col[both].sum(axis=1).min()) if both.any() else None)


def test_w0_by_hand():
    """0 - 1 - 2 - 3 - 4 - 5 - 0 with the weights 1, 100 x 4, 1: a walk from any node to the boundary takes one way round in one
    class and the other way in the other, 402 together, for observable 0 (edge (2, 3)) and observable 1 (edge (0, 5)) alike."""
    g = two_boundary_graph()
    w = np.array([1, 1, 100, 100, 100, 100])
    for k in (0, 1):
        ug = gap_decoder(g, w, observable=k)
        dist2, w0 = ug.gap_table()
        assert w0 == 402 and ug.gap_cap == 402 and ug.gap_step == 402 // 64 + 1 and ug.soft_bins == 64
    dist2 = gap_decoder(g, w).gap_table()[0]
    assert dist2[1, 0].tolist() == [1, 401] and dist2[3, 0].tolist() == [201, 201] and dist2[2, 0].tolist() == [101, 301]
    assert dist2[1, 5].tolist() == [MATCH_INF, 400]  # (no walk continues from node 0: 1 - 2 - 3 - 4 - 5 is the only way, class 1)


def test_a_graph_without_w0():
    g = chain_graph(20, 5)  # a tree: every walk to the boundary has one class
    um = matching_decoder(g, np.ones(19, np.int64))
    with pytest.raises(ValueError, match="observable 0 has no W0"):
        um.with_gap_output()
    ug = um.with_gap_output(cap=77, bins=8)
    assert ug.gap_table()[1] is None and (ug.gap_cap, ug.gap_step, ug.soft_bins) == (77, 77 // 8 + 1, 8)
    assert um.with_gap_output(cap=77, step=5).gap_step == 5


# ---- the class program -------------------------------------------------------------------------------------------------------

def test_gap_cluster_against_every_pairing_and_class_choice():
    graph, w = table_cases()["random130"]
    rng = np.random.default_rng(3)
    some_differ = 0
    for k in (0, 1):
        ug = gap_decoder(graph, w, observable=k)
        dist2 = ug.gap_table()[0]
        for trial in range(36):
            m = 1 + trial % 6
            near = int(rng.integers(1, graph.n_nodes - 12))
            a = sorted(rng.choice(np.arange(near, near + 12), size=m, replace=False).tolist())
            want = [None, None]
            for pairing in all_pairings(a):
                for classes in itertools.product((0, 1), repeat=len(pairing)):
                    terms = [int(dist2[p[0], p[1], cb]) for p, cb in zip(pairing, classes)]
                    if MATCH_INF in terms:
                        continue
                    b = sum(classes) & 1
                    if want[b] is None or sum(terms) < want[b]:
                        want[b] = sum(terms)
            got = ug._gap_cluster(a)
            assert list(got) == want
            cost, mask, _ = ug._match_cluster(a)
            assert cost == min(x for x in got if x is not None)
            if None not in got and got[0] != got[1]:
                some_differ += 1
                assert (mask >> k) & 1 == int(got[1] < got[0])
    assert some_differ > 20


def test_cost_invariants_on_every_cluster_of_decoded_rows():
    uf, um, rows = surface_sample(3, 3, 3e-3, 4000)
    ug = um.with_gap_output()
    seen = []
    inner = ug._cluster_gap
    ug._cluster_gap = lambda ds, cost, mask: seen.append((ds.tolist(), cost, mask)) or inner(ds, cost, mask)
    ug.gap_outputs(rows[:, :uf.num_detectors])
    assert len(seen) > 300
    for ds, cost, mask in seen:
        g0, g1 = ug._gap_cluster(ds)
        assert (cost, mask) == um._match_cluster(ds)[:2]
        assert min(x for x in (g0, g1) if x is not None) == cost
        if g0 is not None and g1 is not None and g0 != g1:
            assert mask & 1 == int(g1 < g0)


# ---- a row -------------------------------------------------------------------------------------------------------------------

def test_a_row_without_a_defect_gives_zero():
    uf, um, rows = surface_sample(3, 3, 3e-3, 4000)
    ug = um.with_gap_output()
    dets = rows[:, :uf.num_detectors]
    D = ug.gap_outputs(dets)
    assert D.dtype == np.int64 and (D[~dets.any(axis=1)] == 0).all() and D.min() >= 0 and D.max() <= ug.gap_cap and (D > 0).sum() > 100


def test_a_miss_gives_the_cap():
    graph, w = table_cases()["island70"]
    ug = gap_decoder(graph, w)
    dets = np.zeros((2, 69), np.bool_)
    dets[0, 66] = True  # node 67: on the island, which has no way to the boundary
    dets[1, 66:68] = True
    assert ug.missed(dets).tolist() == [True, False]
    D = ug.gap_outputs(dets)
    assert D[0] == ug.gap_cap and D[1] < ug.gap_cap


@pytest.mark.parametrize("K", [1, 2, 3, 10, 12])
def test_k_defects_are_matched_and_k_plus_one_peeled(K):
    """On a chain a matched cluster has one finite class (gap = G, deficit 0); a peeled cluster has gap 0 (deficit G)."""
    ug = gap_decoder(chain_graph(70), np.ones(69, np.int64), K, cap=50)
    rows = chain_rows([[(20, K)], [(20, K + 1)], [(10, K), (40, K + 1)], [(1, 1)]])
    assert ug.gap_outputs(rows).tolist() == [0, 50, 50, 0]
    assert ug.match_counts(rows[:2]) == (1, 1) and ug.match_counts(rows[2:3])[1] >= 1 and ug.match_counts(rows[3:]) == (1, 0)
    if K == 2:
        assert ug.gap_outputs(chain_rows([[(30, 3)]])).tolist() == [50]  # three defects in one cluster


def test_the_gap_is_clamped_at_the_cap():
    uf, um, rows = surface_sample(3, 3, 3e-3, 4000)
    dets = rows[:, :uf.num_detectors]
    wide, narrow = um.with_gap_output(), um.with_gap_output(cap=300, step=7)
    Dw, Dn = wide.gap_outputs(dets), narrow.gap_outputs(dets)
    raw = wide.gap_cap - Dw  # min(W0, gap): exact wherever it is below 300 < W0
    assert wide.gap_cap > 300 and np.array_equal(Dn, 300 - np.minimum(300, raw))
    assert (Dn == 0).sum() > (Dw == 0).sum() and 0 < ((Dn > 0) & (Dn < 300)).sum()


def test_counts_of_soft_bin_counts_and_tally_rows():
    uf, um, rows = surface_sample(3, 3, 3e-3, 4000)
    nd = uf.num_detectors
    dets, obs = rows[:, :nd], rows[:, nd].astype(np.uint64)
    for kw in ({}, {"bins": 16}, {"bins": 5, "step": 100}, {"cap": 900, "step": 1, "bins": 1024}):
        ug = um.with_gap_output(**kw)
        wrong = ug.predictions(dets) != obs
        kept, errors = ug.soft_bin_counts(dets, wrong)
        assert kept.shape == errors.shape == (ug.soft_bins,) and kept.sum() == len(rows) and errors.sum() == wrong.sum() > 0
        bins = np.minimum(ug.gap_outputs(dets) // ug.gap_step, ug.soft_bins - 1)
        assert np.array_equal(kept, np.bincount(bins, minlength=ug.soft_bins))
        assert kept[0] >= (~dets.any(axis=1)).sum()
        for corrected in (False, True):
            got = tally_rows(rows, num_detectors=nd, decoder=ug, corrected=corrected)
            assert got.soft_output == "gap" and np.array_equal(got.soft_kept, kept) and np.array_equal(got.soft_errors, errors)
            assert got.decoded_errors == wrong.sum() and got.kept == len(rows)
            k, e = got.rejection_curve()
            assert (k[-1], e[-1]) == (len(rows), wrong.sum())
    mask = np.zeros(nd, np.bool_)
    mask[[1, 7]] = True
    got = tally_rows(rows, num_detectors=nd, decoder=ug, postselection_mask=mask)
    assert got.soft_kept.sum() == got.kept < len(rows) and got.soft_errors.sum() == got.decoded_errors


def test_everything_else_is_the_matching_decoders():
    uf, um, rows = surface_sample(3, 3, 3e-3, 4000)
    dets = rows[:, :uf.num_detectors]
    ug = um.with_gap_output()
    assert np.array_equal(ug.predictions(dets), um.predictions(dets)) and np.array_equal(ug.decode(dets), um.decode(dets))
    assert np.array_equal(ug.missed(dets), um.missed(dets)) and np.array_equal(ug.growth_rounds(dets), um.growth_rounds(dets))
    assert ug.match_counts(dets) == um.match_counts(dets)
    assert ug.graph is um.graph and ug.edge_caps is um.edge_caps and ug.match_weights is um.match_weights and ug.match_defects == um.match_defects
    assert (ug.soft_output, ug.gap_observable) == ("gap", 0) and um.soft_output is None and um.gap_observable is None
    graph, w = table_cases()["island70"]  # misses, and two observables
    bits = np.random.default_rng(8).random((300, 69)) < 0.04
    for k in (0, 1):
        a, b = matching_decoder(graph, w, 3), gap_decoder(graph, w, 3, observable=k)
        assert np.array_equal(a.predictions(bits), b.predictions(bits)) and np.array_equal(a.missed(bits), b.missed(bits))
        assert a.match_counts(bits) == b.match_counts(bits) and a.missed(bits).any() and a.match_counts(bits)[1] > 0
        assert (b.gap_outputs(bits)[a.missed(bits)] == b.gap_cap).all()


def test_the_gap_removes_errors_no_worse_than_the_largest_cluster():
    """A condition, not a measurement: among the rows with ``D <= t`` there are never more errors than among all rows, and at the
    ``t`` that keeps at least 90 % of the rows at most 41 are left, which is what ``largest_cluster`` of the same growth leaves
    there (the numpy prototype of the gap left 9)."""
    uf, um, rows = surface_sample(3, 3, 3e-3, 40000)
    nd = uf.num_detectors
    dets, obs = rows[:, :nd], rows[:, nd].astype(np.uint64)
    ug = um.with_gap_output()
    D = ug.gap_outputs(dets)
    wrong = ug.predictions(dets) != obs
    total = int(wrong.sum())
    left = {}
    for t in np.unique(D):
        keep = D <= t
        left[int(t)] = (float(keep.mean()), int(wrong[keep].sum()))
        assert left[int(t)][1] <= total
    t90 = min(t for t, (frac, _) in left.items() if frac >= 0.9)
    print(f"d = 3, p = 3e-3, 40000 rows, {total} errors: W0 = {ug.gap_cap}; D <= {t90} keeps {left[t90][0]:.4f} with {left[t90][1]} errors")
    assert left[t90][1] <= 41


# ---- what is refused ---------------------------------------------------------------------------------------------------------

def test_refusals():
    g = chain_graph(20, 5)
    uf = UnionFindDecoder(g)
    um = uf.with_cluster_matching()
    ug = um.with_gap_output(cap=10)
    dets = chain_rows([[(3, 2)]])[:, :19]
    with pytest.raises(ValueError, match="no soft output"):
        um.with_soft_output("rounds")
    with pytest.raises(ValueError, match="no soft outputs"):
        um.soft_outputs(dets)
    with pytest.raises(ValueError, match="metric = 'gap'"):
        uf.with_soft_output("gap")
    assert SOFT_OUTPUTS == ("rounds", "full_edges", "largest_cluster", "correction_weight")
    with pytest.raises(ValueError, match="no soft output"):
        ug.with_soft_output("rounds")
    with pytest.raises(ValueError, match="no soft outputs"):
        ug.soft_outputs(dets)
    with pytest.raises(ValueError, match="no flipped edges"):
        ug.flipped_edges(dets)
    with pytest.raises(ValueError, match="with_cluster_matching"):
        uf.with_gap_output(cap=10)
    with pytest.raises(ValueError, match="with_cluster_matching"):
        uf.with_soft_output("rounds").with_gap_output(cap=10)
    for call in (um.gap_table, lambda: um.gap_outputs(dets), lambda: um._gap_cluster([1])):
        with pytest.raises(ValueError, match="with_gap_output"):
            call()
    for bad in (-1, 1, 64, 0.0, True):
        with pytest.raises(ValueError, match="observable"):
            um.with_gap_output(bad, cap=10)
    for bad in (1, 1025, 8.0, True):
        with pytest.raises(ValueError, match="bins"):
            um.with_gap_output(bins=bad, cap=10)
    for bad in (0, -3, 1.5, 1 << 31):
        with pytest.raises(ValueError, match="step"):
            um.with_gap_output(cap=10, step=bad)
    for bad in (0, -1, (1 << 31) - 1, 2.0):
        with pytest.raises(ValueError, match="cap"):
            um.with_gap_output(cap=bad)
    assert um.with_gap_output(cap=(1 << 31) - 2).gap_cap == (1 << 31) - 2
    with pytest.raises(ValueError, match="the decoder has no soft output"):
        um.soft_bin_counts(dets, np.zeros(1, np.bool_))
    assert not hasattr(WindowedUnionFindDecoder, "with_gap_output")


def test_the_new_calls_check_every_argument_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()

    def create(n_nodes, w, K, observable, null_w=False):
        u = np.arange(n_nodes - 1, dtype=np.int32)
        v, obs = u + 1, np.zeros(n_nodes - 1, np.uint64)
        w = np.asarray(w, np.uint16)
        desc = _lib.UfDesc(n_nodes, len(u), n_nodes, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        rc = lib.tsim_uf_create_matching_gap(0, C.byref(desc), None, None if null_w else w.ctypes.data_as(C.c_void_p), K, observable, C.byref(h))
        return rc, lib.tsim_last_error()

    ones = np.ones(69)
    for observable in (-1, 64, 1000):
        rc, msg = create(70, ones, 10, observable)
        assert rc == -22 and b"observable" in msg, (rc, msg)
    for K in (0, 13):
        rc, msg = create(70, ones, K, 0)
        assert rc == -22 and b"max_defects" in msg, (rc, msg)
    rc, msg = create(70, ones, 10, 0, null_w=True)
    assert rc == -22 and b"match_w is NULL" in msg
    rc, msg = create(70, np.where(np.arange(69) == 17, 0, 1), 10, 63)
    assert rc == -22 and b"edge 17 has match weight 0" in msg, (rc, msg)
    rc, msg = create(2049, np.ones(2048), 10, 0)
    assert rc == -95 and b"2049 nodes" in msg, (rc, msg)
    # 1500 nodes: the matching state of K = 12 fits a block's LDS, the two dynamic programs together do not
    assert 16 + uf_match_shot_bytes(1500, 1499, False, 12) <= 64 * 1024 < 16 + uf_match_shot_bytes(1500, 1499, False, 12, gap=True)
    rc, msg = create(1500, np.ones(1499), 12, 0)
    assert rc == -95 and b"bytes of LDS" in msg and b"the winners and the classes" in msg, (rc, msg)
    assert lib.tsim_uf_create_matching_gap(0, None, None, ones.astype(np.uint16).ctypes.data_as(C.c_void_p), 10, 0, C.byref(h)) == -22
    assert lib.tsim_uf_create_matching_gap(0, None, None, None, 10, 0, None) == -22
    w0 = C.c_int64(7)
    assert lib.tsim_uf_gap_table(None, None, C.byref(w0)) == -22

    def decode(cap, step, bins, hist=8):
        return lib.tsim_uf_decode_gap_device(None, None, 1, 16, None, None, 0, 1, None, None, cap, step, bins, hist, None, None), lib.tsim_last_error()

    for cap in (0, -1, (1 << 31) - 1, 1 << 40):
        rc, msg = decode(cap, 1, 8)
        assert rc == -22 and b"gap_cap" in msg, (rc, msg)
    for step in (0, -5, 1 << 31):
        rc, msg = decode(100, step, 8)
        assert rc == -22 and b"gap_step" in msg, (rc, msg)
    for bins in (1, 1025, -1):
        rc, msg = decode(100, 1, bins)
        assert rc == -22 and b"n_bins" in msg, (rc, msg)
    rc, msg = decode(100, 1, 8, hist=None)
    assert rc == -22 and b"d_hist" in msg
    rc, msg = decode(100, 1, 8)
    assert rc == -22 and b"decoder is NULL" in msg


def test_shot_bytes():
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    for K in (1, 4, 10, 12):
        base = uf_match_shot_bytes(25, 78, True, K)
        assert base == uf_match_shot_bytes(25, 78, True, K, gap=False)
        assert uf_match_shot_bytes(25, 78, True, K, gap=True) - base == a16(8 << K) + a16(8 * K * (K + 1))
    assert uf_match_shot_bytes(25, 78, True, 10) - uf_shot_bytes(25, 78, True) == a16(4 << 10) + a16(1 << 10) + a16(20) + a16(440)
    assert 16 + uf_match_shot_bytes(25, 78, True, 12, gap=True) <= 64 * 1024
