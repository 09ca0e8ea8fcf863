"""Sliding-window union-find decoding with heralded erasures, without a device
(``tsim_amd.decode.WindowedUnionFindDecoder(..., heralds=True)``): the windows' herald lists against lists written out by hand,
one window against ``UnionFindDecoder`` with heralds, the invariants of the numpy statement and its known answers on the
heralded d = 3 memory, a graph without heralds, what is refused (``tsim_ufw_create_heralds`` included) and ``count(decoder=wuf)``
on the host path."""

import ctypes as C

import numpy as np
import pytest

from test_unionfind_windowed import d3 as plain_d3
from test_unionfind_windowed import syndrome_of, time_ladder

from tsim_amd import _lib, circuits, faults
from tsim_amd import sampler as sampler_module
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder


def erasure_memory(d: int = 3, rounds: int = 12, p: float = 1e-3, pe: float = 1e-2) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, before_measure_flip_probability=p,
                                                                after_clifford_heralded_erasure=pe))


# ---- the hand-made ladder ----------------------------------------------------------------------------------------------------

LADDER_HERALD_COLS = [2, 5, 9, 10, 16, 17]
LADDER_HERALD_LISTS = [[],          # an empty list
                       [21],        # (8, 10): a time edge across hi_0 = 8
                       [3, 19],     # (0, 7) and (7, 9): the real boundary edge of column 6 and its time edge to the future, one pair in window 0
                       [10, 11],    # (3, 4), (3, 5)
                       [11, 12],    # (3, 5), (3, 6): edge 11 is shared with the herald before; neither herald has an edge in window 1
                       [25]]        # (10, 12): no edge in window 0


def herald_ladder():
    """``(graph, caps)``: ``time_ladder(2, 6, both_ends=False)`` (its 27 edges are written out in ``test_unionfind_windowed``) with six
    heralds whose columns lie among the nodes': 18 detector columns."""
    base, caps = time_ladder(2, 6, both_ends=False)
    g = DecodingGraph(base.n_nodes, base.edge_u, base.edge_v, base.edge_obs, node_det=np.setdiff1d(np.arange(18), LADDER_HERALD_COLS),
                      herald_det=LADDER_HERALD_COLS, herald_ptr=np.cumsum([0] + [len(x) for x in LADDER_HERALD_LISTS]),
                      herald_edges=[e for x in LADDER_HERALD_LISTS for e in x])
    return g, caps


def lists_of(w) -> dict:
    return {int(i): w.herald_edges[w.herald_ptr[j]:w.herald_ptr[j + 1]].tolist() for j, i in enumerate(w.heralds)}


def test_herald_lists_of_a_hand_made_ladder():
    """commit = 4, window = 8: the windows [0, 8) and [4, 12) of ``test_windows_of_a_hand_made_ladder``.  Window 0 numbers its
    edges (0, 1), (0, 3), (0, 5), (0, 7), (0, 8), then the global edges 6 .. 18 as 5 .. 17; window 1 the global edges 2 .. 5 as
    0 .. 3 and 14 .. 26 as 4 .. 16."""
    g, caps = herald_ladder()
    assert (g.n_nodes, g.n_heralds, g.num_detectors) == (13, 6, 18)
    for edge_caps in (None, caps):
        w = WindowedUnionFindDecoder(g, 4, 8, edge_caps=edge_caps, heralds=True)
        assert w.heralds is True and w.num_detectors == 18
        w0, w1 = w.windows()
        assert (w0.lo, w0.hi, w1.lo, w1.hi) == (0, 8, 4, 12)
        # herald 0 has an empty list; herald 1's edge (8, 10) is the virtual pair (0, 8) = local 4 in window 0 and itself, local
        # 11, in window 1; herald 2's two edges are the one pair (0, 7) = local 3 in window 0, and (0, 3) = 1 and (3, 5) = 9 in
        # window 1; heralds 3 and 4 share local 10 and have nothing in window 1; herald 5 has nothing in window 0
        assert lists_of(w0) == {1: [4], 2: [3], 3: [9, 10], 4: [10, 11]}
        assert lists_of(w1) == {1: [11], 2: [1, 9], 5: [15]}
        assert w0.heralds.tolist() == [1, 2, 3, 4] and w0.herald_ptr.tolist() == [0, 1, 2, 4, 6] and w0.herald_edges.tolist() == [4, 3, 9, 10, 10, 11]
        assert w1.heralds.tolist() == [1, 2, 5] and w1.herald_ptr.tolist() == [0, 1, 3, 4] and w1.herald_edges.tolist() == [11, 1, 9, 15]
        assert w0.global_edge[[4, 3]].tolist() == [-1, 3] and w1.global_edge[[11, 1, 9, 15]].tolist() == [21, 3, 19, 25]
    # the pre-grown edges are there before the first round: defects at the nodes 8 and 10 with herald 1 take no growth round,
    # in window 0 (node 8 is joined to the future boundary, nothing is committed) or in window 1 (the edge (8, 10) joins them)
    w = WindowedUnionFindDecoder(g, 4, 8, heralds=True)
    row = np.zeros((2, 18), np.bool_)
    row[:, g.node_det[[7, 9]]] = True
    row[1, LADDER_HERALD_COLS[1]] = True
    flips = w.flipped_edges(row)
    assert flips[1].tolist() == [21] and not w.missed(row).any()
    assert np.array_equal(syndrome_of(g, flips[0]), row[0, g.node_det])
    assert w.growth_rounds(row)[0] >= 1 and w.growth_rounds(row)[1] == 0


# ---- the heralded d = 3 memory of 12 rounds ----------------------------------------------------------------------------------

_CACHE: dict = {}


def d3(weights=None):
    """``(circuit, rows, whole-graph decoder with heralds, windowed decoder with heralds commit = 16, window = 32)``; the rows
    are 3000 seeded rows of ``fault_rows_host`` (673 columns), the same for both weightings."""
    if "c" not in _CACHE:
        c = erasure_memory()
        _CACHE["c"] = (c, faults.fault_rows_host(c.compile_faults(), 0, 3000, (1, 2)).view(np.bool_))
    if weights not in _CACHE:
        c = _CACHE["c"][0]
        _CACHE[weights] = (UnionFindDecoder.from_circuit(c, weights=weights, heralds=True),
                           WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights=weights, heralds=True))
    return _CACHE["c"] + _CACHE[weights]


def test_the_graph_and_its_windows():
    _, rows, uf, w = d3()
    g = w.graph
    assert (g.n_nodes, g.n_edges, g.n_heralds, w.num_detectors, rows.shape) == (97, 363, 576, 672, (3000, 673))
    assert int(rows[:, 672].sum()) == 1030
    assert all(np.array_equal(getattr(g, k), getattr(uf.graph, k)) for k in ("edge_u", "edge_v", "edge_obs", "node_det", "herald_det", "herald_edges"))
    assert [(x.lo, x.hi) for x in w.windows()] == [(0, 32), (16, 48), (32, 64), (48, 80), (64, 96)]
    assert w.info()["n_windows"] == 5 and w.info()["n_heralds"] == 576
    # every herald with an edge has a list somewhere, and every listed local edge is an edge of its window
    seen = np.unique(np.concatenate([x.heralds for x in w.windows()]))
    assert np.array_equal(seen, np.flatnonzero(np.diff(g.herald_ptr) > 0))
    for x in w.windows():
        assert len(x.heralds) > 64 and x.herald_edges.max() < x.graph.n_edges and (np.diff(x.herald_ptr) > 0).all()


@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_is_the_whole_graph_decoder_with_heralds(weights):
    c, rows, uf, _ = d3(weights)
    dets = rows[:600, :672]
    for window in (96, 1000):
        w = WindowedUnionFindDecoder.from_circuit(c, 16, window, weights=weights, resolution=4, heralds=True)
        assert w.info()["n_windows"] == 1
        assert np.array_equal(w.predictions(dets), uf.predictions(dets)) and np.array_equal(w.missed(dets), uf.missed(dets))
        assert np.array_equal(w.growth_rounds(dets), uf.growth_rounds(dets)) and np.array_equal(w.decode(dets), uf.decode(dets))
        assert all(np.array_equal(a, b) for a, b in zip(w.flipped_edges(dets), uf.flipped_edges(dets)))
    assert uf.predictions(dets).any() and uf.growth_rounds(dets).max() >= 1


@pytest.mark.parametrize("weights", [None, "probability"])
def test_invariants_on_seeded_rows(weights):
    """The statement's own asserts (the commit region is clean after its window, the syndrome is reproduced at the end) hold on
    3000 rows - they run inside ``_decode_row`` - and the committed flips reproduce the node columns."""
    _, rows, _, w = d3(weights)
    g = w.graph
    dets = rows[:, :672]
    assert not w.missed(dets).any()
    pred = w.predictions(dets)
    for row, flips, p in zip(dets, w.flipped_edges(dets), pred):
        assert np.array_equal(syndrome_of(g, flips), row[g.node_det])
        assert int(np.bitwise_xor.reduce(g.edge_obs[flips])) == int(p) if len(flips) else p == 0


def test_a_row_with_heralds_only_is_not_decoded():
    _, rows, _, w = d3()
    g = w.graph
    dets = rows[:200, :672].copy()
    dets[:, g.node_det] = False
    dets[0, g.herald_det] = True
    assert dets.any(axis=1).sum() > 150
    assert not w.predictions(dets).any() and not w.missed(dets).any() and not w.growth_rounds(dets).any()
    assert all(len(f) == 0 for f in w.flipped_edges(dets))


def wrong_rows(weights):
    """The wrong rows of the 3000 by: the whole graph with heralds, windows with heralds, the same windows with heralds ignored."""
    _, rows, uf, w = d3(weights)
    g = w.graph
    dets, obs = rows[:, :672], rows[:, 672].astype(np.uint64)
    blind = WindowedUnionFindDecoder(DecodingGraph(g.n_nodes, g.edge_u, g.edge_v, g.edge_obs, g.edge_p), 16, 32, 1, w.edge_caps)
    nodes = dets[:, g.node_det]
    assert not (uf.missed(dets).any() or w.missed(dets).any() or blind.missed(nodes).any())
    return int((uf.predictions(dets) != obs).sum()), int((w.predictions(dets) != obs).sum()), int((blind.predictions(nodes) != obs).sum())


@pytest.mark.parametrize("weights,known", [(None, (39, 44, 527)), ("probability", (34, 36, 449))])
def test_known_answers(weights, known):
    whole, windowed, blind = wrong_rows(weights)
    print(f"weights = {weights}: wrong rows of 3000: whole graph {whole}, windowed {windowed}, windowed with heralds ignored {blind}")
    assert windowed <= 2 * whole
    assert 4 * windowed <= blind
    assert (whole, windowed, blind) == known


# ---- a graph without heralds -------------------------------------------------------------------------------------------------

def test_heralds_true_on_a_graph_without_heralds_is_todays_decoder():
    c, _, plain, rows = plain_d3()
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32, heralds=True)
    assert w.heralds is True and plain.heralds is False and w.graph.n_heralds == 0 and w.num_detectors == 96
    assert np.array_equal(w.predictions(rows), plain.predictions(rows)) and np.array_equal(w.missed(rows), plain.missed(rows))
    assert np.array_equal(w.growth_rounds(rows), plain.growth_rounds(rows))
    assert all(np.array_equal(a, b) for a, b in zip(w.flipped_edges(rows), plain.flipped_edges(rows)))
    for a, b in zip(w.windows(), plain.windows()):
        assert all(np.array_equal(x, y) for x, y in zip(a[3:6], b[3:6])) and a[:2] == b[:2]
        assert len(a.heralds) == 0 and a.herald_ptr.tolist() == [0] and len(a.herald_edges) == 0 and b.heralds is None
    g = WindowedUnionFindDecoder(plain.graph, 16, 32, heralds=True)
    assert np.array_equal(g.predictions(rows), plain.predictions(rows))


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_constructor():
    c, _, _, w = d3()
    g = w.graph
    with pytest.raises(NotImplementedError, match="heralds"):
        WindowedUnionFindDecoder(g, 16, 32)
    with pytest.raises(NotImplementedError, match="heralds"):
        WindowedUnionFindDecoder(g, 16, 32, heralds=False)
    for bad in (dict(commit=0, window=8), dict(commit=8, window=8), dict(commit=4.0, window=8)):
        with pytest.raises(ValueError, match="commit"):
            WindowedUnionFindDecoder(g, heralds=True, **bad)
    with pytest.raises(ValueError, match="heralds"):
        WindowedUnionFindDecoder(g, 16, 32, heralds=1)
    with pytest.raises(ValueError, match="edge 110 = .6, 17.*too small"):
        WindowedUnionFindDecoder.from_circuit(c, 8, 16, heralds=True)
    with pytest.raises(ValueError, match="dets must be .n, 672."):
        w.predictions(np.zeros((1, 96), np.bool_))


def test_create_heralds_refuses_without_a_device():
    """What ``tsim_ufw_create_heralds`` refuses before any device call: the graph, the caps, commit and window, the buffer, and
    every check of ``tsim_uf_create_heralds`` on the herald struct."""
    lib = _lib.load()
    h = C.c_void_p()

    def create(n_cols=7, n_det_cols=6, commit=2, window=4, caps=None, edges=None, no_heralds=False, **kw):
        a = dict(node_det=[0, 2, 3, 5], herald_det=[1, 4], herald_ptr=[0, 1, 3], herald_edges=[3, 0, 3])
        a.update(kw)
        u, v = (np.arange(4), np.arange(4) + 1) if edges is None else edges
        u, v = np.asarray(u, np.int32), np.asarray(v, np.int32)
        obs = np.zeros(len(u), np.uint64)
        desc = _lib.UfDesc(5, len(u), n_cols, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        arrays = {k: np.array(x + [0], np.int32) for k, x in a.items()}
        her = _lib.UfHeralds(n_det_cols, len(a["herald_det"]), *(arrays[k].ctypes.data for k in ("node_det", "herald_det", "herald_ptr", "herald_edges")))
        caps = None if caps is None else np.asarray(caps, np.uint8)
        rc = lib.tsim_ufw_create_heralds(0, C.byref(desc), None if caps is None else C.c_void_p(caps.ctypes.data), commit, window,
                                         None if no_heralds else C.byref(her), C.byref(h))
        msg = lib.tsim_last_error()
        if rc == 0:  # (a device is there and the arguments are fine: give the handle back)
            lib.tsim_ufw_destroy(h)
            h.value = None
        return rc, msg

    for kw, what in ((dict(herald_det=[1, 3]), b"named twice"), (dict(herald_det=[4, 4]), b"named twice"),
                     (dict(herald_edges=[3, 0, 4]), b"of 4 edges"), (dict(herald_edges=[-1, 0, 3]), b"of 4 edges"),
                     (dict(herald_ptr=[0, 2, 1]), b"must not fall"), (dict(herald_ptr=[1, 1, 3]), b"herald_ptr[0] = 1"),
                     (dict(n_cols=5), b"n_cols = 5"), (dict(n_det_cols=7), b"n_det_cols = 7"), (dict(n_det_cols=4), b"n_det_cols = 4"),
                     (dict(node_det=[0, 3, 2, 5]), b"strictly ascending"), (dict(node_det=[0, 2, 3, 6]), b"leaves the columns"),
                     (dict(herald_det=[1, 6]), b"leaves the columns"), (dict(herald_det=[-1, 4]), b"leaves the columns"),
                     (dict(commit=0), b"commit = 0"), (dict(commit=4, window=4), b"commit = 4, window = 4"),
                     (dict(caps=[1, 2, 3, 15]), b"edge 3 has cap 15"), (dict(caps=[0, 2, 3, 4]), b"edge 0 has cap 0"),
                     (dict(edges=([0, 0], [2, 1])), b"strictly ascending"), (dict(edges=([0, 1], [1, 5])), b"leaves the nodes"),
                     # nodes 1 - 4 joined: column 0 is committed in window 0 = [0, 2), which ends before column 3
                     (dict(commit=1, window=2, edges=([0, 1], [1, 4]), herald_edges=[1, 0, 1]), b"too small"),
                     (dict(commit=1, window=2, edges=([0, 1], [1, 4]), herald_edges=[1, 0, 1], no_heralds=True), b"too small")):
        rc, msg = create(**kw)
        assert rc == -22 and what in msg, (kw, rc, msg)
        assert h.value is None
    assert lib.tsim_ufw_create_heralds(0, None, None, 2, 4, None, C.byref(h)) == -22
    assert lib.tsim_ufw_create_heralds(0, None, None, 2, 4, None, None) == -22
    # arguments that are fine get as far as the device: 0 with one, the HIP error without
    for kw in ({}, dict(caps=[1, 2, 3, 14]), dict(n_cols=6), dict(no_heralds=True, n_cols=4)):
        rc, msg = create(**kw)
        assert rc in (0, -5) or (rc == -22 and b"device 0 of 0" in msg), (kw, rc, msg)


def test_both_handles_refuse_a_graph_its_caps_and_its_heralds_alike():
    """The bad graphs, caps and herald structs of the refusal tests of ``tsim_uf_create`` / ``_weighted`` / ``_heralds``: the
    whole-graph handle and the windowed one (``commit`` 2 < ``window`` 4) give the same code and the same text, before any
    device call - a check of one handle is a check of the other."""
    lib = _lib.load()

    def both(n_nodes, u, v, n_cols=None, caps=None, heralds=None, n_det_cols=None):
        u, v = np.asarray(u, np.int32), np.asarray(v, np.int32)
        obs = np.zeros(len(u), np.uint64)
        desc = _lib.UfDesc(n_nodes, len(u), n_nodes if n_cols is None else n_cols, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        caps = None if caps is None else np.asarray(caps, np.uint8)
        d_caps = None if caps is None else C.c_void_p(caps.ctypes.data)
        her = None
        if heralds is not None:
            arrays = {k: np.array(x + [0], np.int32) for k, x in heralds.items()}
            her = C.byref(_lib.UfHeralds(n_det_cols, len(heralds["herald_det"]),
                                         *(arrays[k].ctypes.data for k in ("node_det", "herald_det", "herald_ptr", "herald_edges"))))
        h = C.c_void_p()
        whole = lib.tsim_uf_create_heralds(99, C.byref(desc), d_caps, her, C.byref(h)), lib.tsim_last_error()
        assert not h.value
        windowed = lib.tsim_ufw_create_heralds(99, C.byref(desc), d_caps, 2, 4, her, C.byref(h)), lib.tsim_last_error()
        assert not h.value
        assert whole == windowed
        assert whole[0] == -22 and b"device" not in whole[1], whole
        return whole[1]

    # the graph (test_unionfind.py)
    for nodes, u, v, what in ((4, [0, 0], [2, 1], b"strictly ascending"), (4, [0, 0], [1, 1], b"strictly ascending"),
                              (4, [2], [1], b"u < v"), (4, [1], [4], b"leaves the nodes"), (4, [-1], [2], b"leaves the nodes"),
                              (1, [], [], b"n_nodes")):
        assert what in both(nodes, u, v)
    assert b"n_cols" in both(4, [0], [1], n_cols=2)
    # the caps (test_unionfind_weighted.py); the graph's own checks come first
    u = np.arange(69)
    for caps, what in (([2] * 68 + [0], b"edge 68 has cap 0"), ([15] + [2] * 68, b"edge 0 has cap 15"), ([2, 2, 255] + [2] * 66, b"edge 2 has cap 255")):
        assert what in both(70, u, u + 1, caps=caps)
    assert b"strictly ascending" in both(4, [0, 0], [2, 1], caps=[2, 0])
    # the herald struct (test_unionfind_erasure.py, and the cases of the test above)
    for kw, what in ((dict(herald_det=[1, 3]), b"named twice"), (dict(herald_det=[4, 4]), b"named twice"),
                     (dict(herald_edges=[3, 0, 4]), b"of 4 edges"), (dict(herald_edges=[3, -1, 0]), b"of 4 edges"),
                     (dict(herald_edges=[-1, 0, 3]), b"of 4 edges"), (dict(herald_ptr=[0, 2, 1]), b"must not fall"),
                     (dict(herald_ptr=[1, 1, 3]), b"herald_ptr[0] = 1"), (dict(n_cols=5), b"n_cols = 5"),
                     (dict(n_det_cols=7), b"n_det_cols = 7"), (dict(n_det_cols=4), b"n_det_cols = 4"),
                     (dict(node_det=[0, 3, 2, 5]), b"strictly ascending"), (dict(node_det=[0, 2, 3, 6]), b"leaves the columns"),
                     (dict(herald_det=[1, -4]), b"leaves the columns"), (dict(herald_det=[1, 6]), b"leaves the columns"),
                     (dict(herald_det=[-1, 4]), b"leaves the columns"), (dict(caps=[1, 2, 15, 1]), b"edge 2 has cap 15")):
        kw = dict(kw)
        scalars = {k: kw.pop(k) for k in ("n_cols", "n_det_cols", "caps") if k in kw}
        heralds = dict(dict(node_det=[0, 2, 3, 5], herald_det=[1, 4], herald_ptr=[0, 1, 3], herald_edges=[3, 0, 3]), **kw)
        assert what in both(5, np.arange(4), np.arange(4) + 1, heralds=heralds, **dict(dict(n_cols=7, n_det_cols=6), **scalars))


# ---- count() on the host path ----------------------------------------------------------------------------------------------

def test_host_count_equals_the_tally_of_sample_and_decode(monkeypatch):
    monkeypatch.setattr(sampler_module, "sample_program", lambda *a, **k: pytest.fail("no program is sampled here"))
    c, _, _, w = d3()
    nd = w.num_detectors
    assert (nd, w.num_observables) == (672, 1)
    rows = c.compile_detector_sampler(seed=4, method="faults").sample(600, append_observables=True)
    got = c.compile_detector_sampler(seed=4, method="faults").count(600, decoder=w)
    dets, obs = rows[:, :nd], rows[:, nd:]
    assert got.kept == 600 and got.decoder_misses == int(w.missed(dets).sum()) == 0
    assert got.decoded_errors == int((w.decode(dets) != obs).any(axis=1).sum())
    assert 0 < got.decoded_errors < got.kept_with_observable_flip
    assert got == tally_rows(rows, num_detectors=nd, decoder=w, histogram_columns=(nd,))
