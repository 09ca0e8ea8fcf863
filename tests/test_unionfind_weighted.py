"""Weighted growth of the union-find decoder without a device: the caps from ``edge_p``, caps of 2 against the unweighted
decoder, the numpy statement's known answers on seeded rows, a hand-made graph where the weights change the correction, a
miss under weights, and what the constructor and ``tsim_uf_create_weighted`` refuse."""

import ctypes as C

import numpy as np
import pytest

from test_unionfind import chain_graph, memory, no_boundary_graph, syndrome_of, wide_observable_graph

from tsim_amd import _lib, faults
from tsim_amd.decode import DecodingGraph, UnionFindDecoder


def fault_rows(c, n):
    form = c.compile_faults()
    rows = faults.fault_rows_host(form, 0, n, (1, 2)).view(np.bool_)
    return rows[:, :form.num_detectors], rows[:, form.num_detectors:]


def detour_graph() -> DecodingGraph:
    """Detectors 1 and 2 joined directly (edge 0, observable 0) and over 1 - 3 - 4 - 2 (edges 1, 3, 2: observables 1, -, 2);
    the boundary has no edge."""
    return DecodingGraph(5, [1, 1, 2, 3], [2, 3, 4, 4], np.array([1, 2, 4, 0], np.uint64))


# ---- the caps --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,p,want", [(3, 1e-3, {5: 8, 6: 27, 7: 22, 8: 21}), (5, 5e-3, {4: 16, 5: 110, 6: 75, 7: 116, 8: 185})])
def test_growth_caps_histograms(d, p, want):
    g = UnionFindDecoder.from_circuit(memory(d, p)).graph
    caps = g.growth_caps(4)
    assert caps.dtype == np.uint8 and caps.shape == (g.n_edges,)
    values, counts = np.unique(caps, return_counts=True)
    assert dict(zip(values.tolist(), counts.tolist())) == want
    assert caps[np.argmin(g.edge_p)] == 8 and caps[np.argmax(g.edge_p)] == caps.min()
    assert np.array_equal(g.growth_caps(), caps)  # the default resolution is 4
    uf = UnionFindDecoder.from_circuit(memory(d, p), weights="probability")
    assert np.array_equal(uf.edge_caps, caps) and uf.edge_caps.dtype == np.uint8
    assert UnionFindDecoder.from_circuit(memory(d, p)).edge_caps is None


def test_growth_caps_range_and_refusals():
    g = UnionFindDecoder.from_circuit(memory(3, 1e-3)).graph
    for r in range(1, 8):
        caps = g.growth_caps(r)
        assert caps.min() >= 1 and caps.max() == 2 * r
    assert set(g.growth_caps(1).tolist()) <= {1, 2}
    for bad in (0, 8, -1, 4.0, "4", None, True):
        with pytest.raises(ValueError, match="resolution"):
            g.growth_caps(bad)
    with pytest.raises(ValueError, match="resolution"):
        UnionFindDecoder.from_circuit(memory(3, 1e-3), weights="probability", resolution=8)
    with pytest.raises(ValueError, match="weights"):
        UnionFindDecoder.from_circuit(memory(3, 1e-3), weights="logp")
    # equal probabilities: 2 * resolution everywhere, also when every L is 0 (p = 0.5) and for unset probabilities
    u = np.arange(5)
    for p in (0.01, 0.5, 0.0):
        flat = DecodingGraph(6, u, u + 1, np.zeros(5, np.uint64), np.full(5, p))
        assert flat.growth_caps(3).tolist() == [6] * 5 and flat.growth_caps(7).tolist() == [14] * 5
    assert DecodingGraph(3, [], [], np.zeros(0, np.uint64)).growth_caps(4).shape == (0,)


# ---- the rule --------------------------------------------------------------------------------------------------------------

def same_answers(a, b, dets):
    assert np.array_equal(a.predictions(dets), b.predictions(dets))
    assert np.array_equal(a.missed(dets), b.missed(dets))
    assert np.array_equal(a.growth_rounds(dets), b.growth_rounds(dets))
    fa, fb = a.flipped_edges(dets), b.flipped_edges(dets)
    assert len(fa) == len(fb) and all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert np.array_equal(a.decode(dets), b.decode(dets))


@pytest.mark.parametrize("name", ["chain", "no_boundary", "wide_observables", "d3"])
def test_caps_of_two_are_the_unweighted_decoder(name):
    rng = np.random.default_rng(3)
    if name == "d3":
        c = memory(3, 5e-3)
        plain = UnionFindDecoder.from_circuit(c)
        dets, _ = fault_rows(c, 4000)
        n_obs = 1
    else:
        g, n_obs = {"chain": (chain_graph(), 1), "no_boundary": (no_boundary_graph(), 2), "wide_observables": (wide_observable_graph(), 64)}[name]
        plain = UnionFindDecoder(g, n_obs)
        dets = rng.random((150, g.n_nodes - 1)) < min(0.5, 3.0 / (g.n_nodes - 1))
        dets[0] = False
    two = UnionFindDecoder(plain.graph, n_obs, edge_caps=np.full(plain.graph.n_edges, 2))
    assert two.edge_caps.dtype == np.uint8
    same_answers(plain, two, dets)
    assert plain.growth_rounds(dets).max() >= 2
    if name == "no_boundary":
        assert plain.missed(dets).any()


@pytest.mark.parametrize("d,p,n,weighted_errors,unweighted_errors", [(3, 1e-3, 20000, 9, 12), (3, 5e-3, 4000, 34, 42), (5, 5e-3, 4000, 23, 37)])
def test_known_answers_at_resolution_4(d, p, n, weighted_errors, unweighted_errors):
    """The numpy statement on the fault statement's rows under the key (1, 2): fewer decoded errors than without weights."""
    c = memory(d, p)
    dets, obs = fault_rows(c, n)
    got = {}
    for weights in (None, "probability"):
        uf = UnionFindDecoder.from_circuit(c, weights=weights)
        assert not uf.missed(dets).any()
        got[weights] = int((uf.decode(dets) != obs).any(axis=1).sum())
        print(f"d = {d}, p = {p}, weights = {weights}: {got[weights]} decoded errors of {n}, at most {int(uf.growth_rounds(dets).max())} growth rounds")
        if weights:  # every correction still reproduces its syndrome
            flipped = uf.flipped_edges(dets[:300])
            assert all(np.array_equal(syndrome_of(uf.graph, f), r) for f, r in zip(flipped, dets[:300]))
    assert got == {None: unweighted_errors, "probability": weighted_errors}
    assert got["probability"] < got[None]


def test_weights_change_the_correction():
    g = detour_graph()
    dets = np.array([[1, 1, 0, 0]], np.bool_)
    plain = UnionFindDecoder(g, 3)
    weighted = UnionFindDecoder(g, 3, edge_caps=[8, 1, 1, 1])
    assert plain.flipped_edges(dets)[0].tolist() == [0] and plain.predictions(dets).tolist() == [1]
    assert weighted.flipped_edges(dets)[0].tolist() == [1, 2, 3] and weighted.predictions(dets).tolist() == [6]
    assert plain.growth_rounds(dets).tolist() == [1] and weighted.growth_rounds(dets).tolist() == [2]
    assert not plain.missed(dets).any() and not weighted.missed(dets).any()
    assert weighted.decode(dets).tolist() == [[False, True, True]]


def test_a_miss_survives_weighting():
    uf = UnionFindDecoder(no_boundary_graph(), edge_caps=[3, 14])
    dets = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 0, 0]], np.bool_)
    assert uf.missed(dets).tolist() == [True, True, False, False, True, False]
    assert uf.predictions(dets).tolist() == [0, 0, 1, 2, 0, 0]
    assert uf.growth_rounds(dets).tolist() == [14, 14, 7, 3, 14, 0]  # (a miss is noticed in the round after the last change)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_the_constructor_refuses_bad_caps():
    g = chain_graph()
    for caps, what in ((np.full(68, 2), "shape"), (np.full(70, 2), "shape"), (np.full((69, 1), 2), "shape"), (np.full(69, 2.0), "integers"),
                       ([2] * 68 + [0], "edge 68 has cap 0"), ([15] + [2] * 68, "edge 0 has cap 15"), ([-1] + [2] * 68, "cap -1"),
                       ([256 + 2] * 69, "cap 258")):
        with pytest.raises(ValueError, match=what):
            UnionFindDecoder(g, edge_caps=caps)
    assert UnionFindDecoder(g, edge_caps=[1, 14] + [2] * 67).edge_caps[:2].tolist() == [1, 14]
    assert UnionFindDecoder(g).edge_caps is None


def test_create_weighted_refuses_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()

    def create(n_nodes, u, v, caps):
        u, v = np.asarray(u, np.int32), np.asarray(v, np.int32)
        obs = np.zeros(len(u), np.uint64)
        desc = _lib.UfDesc(n_nodes, len(u), n_nodes, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        if caps is None:
            rc = lib.tsim_uf_create(0, C.byref(desc), C.byref(h))
        else:
            caps = np.asarray(caps, np.uint8)
            rc = lib.tsim_uf_create_weighted(0, C.byref(desc), C.c_void_p(caps.ctypes.data), C.byref(h))
        msg = lib.tsim_last_error() if rc else b""  # (a call that succeeds leaves the text of the last failure)
        if rc == 0:  # (a device is there and the graph is fine: give the handle back)
            lib.tsim_uf_destroy(h)
            h.value = None
        return rc, msg

    u = np.arange(69)
    for caps, what in (([2] * 68 + [0], b"edge 68 has cap 0"), ([15] + [2] * 68, b"edge 0 has cap 15"), ([2, 2, 255] + [2] * 66, b"edge 2 has cap 255")):
        rc, msg = create(70, u, u + 1, caps)
        assert rc == -22 and what in msg, (rc, msg)
        assert h.value is None
    # the graph's own checks come first, as in tsim_uf_create
    rc, msg = create(4, [0, 0], [2, 1], [2, 0])
    assert rc == -22 and b"strictly ascending" in msg
    assert lib.tsim_uf_create_weighted(0, None, None, C.byref(h)) == -22
    # 6500 nodes and 30000 edges: 61.4 kB of LDS per shot with the two bitmaps, 72.6 kB with the 4-bit counters
    uu = np.repeat(np.arange(1, 6001), 5)
    vv = uu + np.tile(np.arange(1, 6), 6000)
    rc, msg = create(6500, uu, vv, np.full(30000, 3))
    assert rc == -95 and b"bytes of LDS" in msg, (rc, msg)
    rc, msg = create(6500, uu, vv, None)
    assert rc != -95 and b"bytes of LDS" not in msg, (rc, msg)  # (without a device it fails later, at the first device call)
    assert h.value is None
