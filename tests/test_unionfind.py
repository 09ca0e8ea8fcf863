"""The union-find decoder without a device: the decoding graph against ``analyze()``'s masks, the numpy statement of the
decoding rule (single edges, validity of every correction, the logical error rate against the plain tally, hand-made
graphs), what the constructors and ``tsim_uf_create`` refuse, and ``count(decoder=uf)`` on the host path."""

import ctypes as C

import numpy as np
import pytest

from tsim_amd import _lib, circuits, faults
from tsim_amd import sampler as sampler_module
from tsim_amd.clifford import CliffordCircuit, _bits
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodingGraph, LookupDecoder, UnionFindDecoder


def memory(d: int, p: float, rounds: int | None = None) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, d if rounds is None else rounds, after_clifford_depolarization=p,
                                                                before_measure_flip_probability=p, after_reset_flip_probability=p))


_CACHE: dict = {}


def decoder_of(d: int, p: float):
    """``(circuit, decoder)``, built once per module run (the decoder caches the syndromes it has seen)."""
    if (d, p) not in _CACHE:
        c = memory(d, p)
        _CACHE[d, p] = (c, UnionFindDecoder.from_circuit(c))
    return _CACHE[d, p]


def chain_graph(n_nodes: int = 70, obs_edge: int = 40) -> DecodingGraph:
    """0 - 1 - 2 - ... - (n_nodes - 1); the edge ``(obs_edge, obs_edge + 1)`` flips observable 0."""
    u = np.arange(n_nodes - 1)
    obs = np.zeros(n_nodes - 1, np.uint64)
    obs[obs_edge] = 1
    return DecodingGraph(n_nodes, u, u + 1, obs)


def no_boundary_graph() -> DecodingGraph:
    """Nodes 1 - 2 joined to each other and not to the boundary; node 3 hangs on the boundary."""
    return DecodingGraph(4, [0, 1], [3, 2], np.array([2, 1], np.uint64))


def wide_observable_graph() -> DecodingGraph:
    """A ring of 9 detectors with three spokes to the boundary; observables 0, 1 and 63."""
    u = [0, 0, 0] + list(range(1, 9)) + [1]
    v = [1, 4, 7] + list(range(2, 10)) + [9]
    order = np.lexsort((v, u))
    obs = np.zeros(len(u), np.uint64)
    obs[[0, 3, 5]] = [1 << 63, 1, 2]
    obs[7] = (1 << 63) | 2
    return DecodingGraph(10, np.array(u)[order], np.array(v)[order], obs)


def syndrome_of(graph: DecodingGraph, edges) -> np.ndarray:
    """The detector row that the edges, flipped together, produce."""
    s = np.zeros(graph.n_nodes, np.bool_)
    for e in edges:
        s[graph.edge_u[e]] ^= True
        s[graph.edge_v[e]] ^= True
    return s[1:]


# ---- the graph -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,nodes,edges", [(3, 25, 78), (5, 121, 502)])
def test_graph_sizes_and_reconstruction_from_the_masks(d, nodes, edges):
    c, uf = decoder_of(d, 1e-3)
    g = uf.graph
    info = uf.info()
    assert (g.n_nodes, g.n_edges, info["dropped_bits"], info["undetectable_bits"]) == (nodes, edges, 0, 0)
    assert (uf.num_detectors, uf.num_observables) == (nodes - 1, 1)
    assert g.edge_u.dtype == np.int32 and g.edge_v.dtype == np.int32 and g.edge_obs.dtype == np.uint64 and g.edge_p.dtype == np.float64
    assert (g.edge_u < g.edge_v).all() and (np.diff(g.edge_u.astype(np.int64) * nodes + g.edge_v) > 0).all()
    assert ((g.edge_p > 0) & (g.edge_p < 0.5)).all()
    # every error bit's column, rebuilt from analyze()'s masks (not from the form's lists), gives the same edges
    an = c.analyze()
    cols = [[] for _ in range(an.num_e)]
    for j, (m, _) in enumerate(an.detectors):
        for e in _bits(int(m)):
            cols[e].append(j + 1)
    flips_obs = [0] * an.num_e
    for k in sorted(an.observables):
        for e in _bits(int(an.observables[k][0])):
            flips_obs[e] |= 1 << k
    want, e0 = {}, 0
    for probs in an.channel_probs:
        nb = int(np.log2(len(probs)))
        for i in range(nb):
            p = sum(float(probs[o]) for o in range(len(probs)) if (o >> i) & 1)
            col = cols[e0 + i]
            assert len(col) <= 2
            if p > 0 and col:
                want.setdefault((0, col[0]) if len(col) == 1 else tuple(col), set()).add(flips_obs[e0 + i])
        e0 += nb
    assert sorted(want) == list(zip(g.edge_u.tolist(), g.edge_v.tolist()))
    assert all(len(masks) == 1 for masks in want.values())  # no two bits of a pair disagree on the observables
    assert [next(iter(want[k])) for k in sorted(want)] == g.edge_obs.tolist()


def test_merging_of_parallel_bits():
    """Bits of one pair: within a mask p (1 - q) + q (1 - p); the likelier mask is kept, a tie goes to the smaller mask."""
    text = "\n".join(["R 0 1", "X_ERROR(0.1) 0", "X_ERROR(0.2) 0", "M 0", "DETECTOR rec[-1]", "X_ERROR(0.25) 1", "M 1", "DETECTOR rec[-1]",
                      "OBSERVABLE_INCLUDE(0) rec[-1]"])
    g = DecodingGraph.from_form(CliffordCircuit(text).compile_faults())
    assert (g.n_nodes, g.edge_u.tolist(), g.edge_v.tolist(), g.edge_obs.tolist()) == (3, [0, 0], [1, 2], [0, 1])
    assert g.edge_p.tolist() == [0.1 * 0.8 + 0.2 * 0.9, 0.25]
    # two masks on one pair: detector 0 is flipped by a bit that also flips the observable (0.3) and by bits that do not
    base = ["R 0 1", "X_ERROR({a}) 0", "X_ERROR({b}) 1", "M 0 1", "DETECTOR rec[-1] rec[-2]", "OBSERVABLE_INCLUDE(0) rec[-1]"]
    for a, b, mask, p in ((0.3, 0.2, 0, 0.3), (0.2, 0.3, 1, 0.3), (0.25, 0.25, 0, 0.25)):
        g = DecodingGraph.from_form(CliffordCircuit("\n".join(base).format(a=a, b=b)).compile_faults())
        assert (g.edge_u.tolist(), g.edge_v.tolist(), g.edge_obs.tolist(), g.edge_p.tolist()) == ([0], [1], [mask], [p])
    # a bit with no detector and an observable, and a bit with three detectors, are counted and left out
    text = "\n".join(["R 0 1 2 3", "X_ERROR(0.1) 3", "X_ERROR(0.1) 0", "CX 0 1 0 2", "M 0 1 2 3", "DETECTOR rec[-4]", "DETECTOR rec[-3]",
                      "DETECTOR rec[-2]", "OBSERVABLE_INCLUDE(0) rec[-1]"])
    g = DecodingGraph.from_form(CliffordCircuit(text).compile_faults())
    assert g.info()["dropped_bits"] == 1 and g.info()["undetectable_bits"] == 1 and g.n_edges == 0 and g.n_nodes == 4


# ---- the decoding rule -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [3, 5])
def test_every_single_edge_decodes_to_its_own_mask(d):
    _, uf = decoder_of(d, 1e-3)
    g = uf.graph
    dets = np.array([syndrome_of(g, [e]) for e in range(g.n_edges)])
    assert not uf.missed(dets).any()
    assert np.array_equal(uf.predictions(dets), g.edge_obs)
    assert np.array_equal(uf.decode(dets)[:, 0], g.edge_obs.astype(np.bool_))


def test_every_correction_reproduces_its_syndrome():
    c, uf = decoder_of(5, 5e-3)
    form = c.compile_faults()
    rows = faults.fault_rows_host(form, 0, 2000, (1, 2)).view(np.bool_)
    dets = rows[:, :form.num_detectors]
    assert dets.any(axis=1).sum() > 1500 and not uf.missed(dets).any()
    flipped = uf.flipped_edges(dets)
    pred = uf.predictions(dets)
    for r in range(len(dets)):
        assert np.array_equal(syndrome_of(uf.graph, flipped[r]), dets[r]), r
        assert int(np.bitwise_xor.reduce(uf.graph.edge_obs[flipped[r]])) == int(pred[r]) if len(flipped[r]) else pred[r] == 0
    assert uf.growth_rounds(dets).max() >= 3


def test_error_rate_against_the_plain_tally():
    """20000 rows of the fault statement at p = 1e-3 under the key (1, 2).  The rule is deterministic: 12 decoded errors of 322
    rows with an observable flip at d = 3, 3 of 830 at d = 5, no miss."""
    got = {}
    for d in (3, 5):
        c, uf = decoder_of(d, 1e-3)
        form = c.compile_faults()
        rows = faults.fault_rows_host(form, 0, 20000, (1, 2)).view(np.bool_)
        dets, obs = rows[:, :form.num_detectors], rows[:, form.num_detectors:]
        raw = int(obs.any(axis=1).sum())
        errors = int((uf.decode(dets) != obs).any(axis=1).sum())
        print(f"d = {d}: {raw} raw observable flips, {errors} decoded errors, {int(uf.missed(dets).sum())} misses, "
              f"{int(uf.growth_rounds(dets).max())} growth rounds at most")
        assert not uf.missed(dets).any()
        got[d] = (raw, errors)
    assert got[3][1] < got[3][0] / 5
    assert got[5][1] < got[3][1]
    assert got == {3: (322, 12), 5: (830, 3)}


def test_hand_made_graphs():
    # a component without a boundary edge and one defect: a miss, no flip predicted; two defects there are matched
    uf = UnionFindDecoder(no_boundary_graph())
    dets = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 0, 0]], np.bool_)
    assert uf.missed(dets).tolist() == [True, True, False, False, True, False]
    assert uf.predictions(dets).tolist() == [0, 0, 1, 2, 0, 0]
    assert uf.num_observables == 2 and uf.decode(dets).shape == (6, 2)
    # observable bit 63 survives
    g = wide_observable_graph()
    uf = UnionFindDecoder(g, 64)
    dets = np.array([syndrome_of(g, [e]) for e in range(g.n_edges)])
    assert np.array_equal(uf.predictions(dets), g.edge_obs) and (int(g.edge_obs.max()) >> 63) == 1
    assert uf.decode(dets)[:, 63].tolist() == [bool(int(m) >> 63) for m in g.edge_obs]
    # a chain of 70 nodes: two defects far from each other and from the boundary are joined along the chain
    g = chain_graph()
    uf = UnionFindDecoder(g)
    dets = np.zeros((3, 69), np.bool_)
    dets[0, [29, 49]] = True   # nodes 30 and 50: across the observable's edge (40, 41)
    dets[1, [44, 64]] = True   # nodes 45 and 65: beside it
    dets[2, [4, 67]] = True    # node 5 reaches the boundary (10 rounds: a lone cluster gains a node per two rounds) and rests;
    #                            node 68 then grows alone until it meets that cluster at node 10: 10 + 2 * 53 rounds
    assert not uf.missed(dets).any() and uf.predictions(dets).tolist() == [1, 0, 1]
    assert uf.flipped_edges(dets)[0].tolist() == list(range(30, 50)) and uf.flipped_edges(dets)[1].tolist() == list(range(45, 65))
    assert uf.flipped_edges(dets)[2].tolist() == list(range(5, 68))
    assert uf.growth_rounds(dets).tolist() == [20, 20, 116]  # (20 edges between the two defects, each fills 10 of them)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_constructors_refuse():
    with pytest.raises(ValueError, match="strictly ascending"):
        DecodingGraph(4, [0, 0], [2, 1], [0, 0])
    with pytest.raises(ValueError, match="strictly ascending"):
        DecodingGraph(4, [0, 0], [1, 1], [0, 0])
    with pytest.raises(ValueError, match="u < v"):
        DecodingGraph(4, [2], [1], [0])
    with pytest.raises(ValueError, match="u < v"):
        DecodingGraph(4, [1], [1], [0])
    with pytest.raises(ValueError, match="0 .. 3"):
        DecodingGraph(4, [1], [4], [0])
    with pytest.raises(ValueError, match="0 .. 3"):
        DecodingGraph(4, [-1], [2], [0])
    with pytest.raises(ValueError, match="equally long"):
        DecodingGraph(4, [0, 1], [1], [0])
    with pytest.raises(NotImplementedError, match="65535"):
        DecodingGraph(65536, [0], [1], [0])
    u = np.repeat(np.arange(300), 300)[:65536]
    v = 300 + np.tile(np.arange(300), 300)[:65536]
    with pytest.raises(NotImplementedError, match="65536 edges"):
        DecodingGraph(600, u, v, np.zeros(65536, np.uint64))
    DecodingGraph(600, u[:65535], v[:65535], np.zeros(65535, np.uint64))
    with pytest.raises(ValueError, match="at most 64 observables"):
        UnionFindDecoder(chain_graph(), 65)
    with pytest.raises(ValueError, match="observable 1"):
        UnionFindDecoder(no_boundary_graph(), 1)
    text = "R 0\nX_ERROR(0.1) 0\nM 0\nDETECTOR rec[-1]\n" + "\n".join(f"OBSERVABLE_INCLUDE({k}) rec[-1]" for k in range(65))
    with pytest.raises(ValueError, match="at most 64 observables"):
        UnionFindDecoder.from_circuit(CliffordCircuit(text))
    with pytest.raises(ValueError, match="dets must be"):
        UnionFindDecoder(chain_graph()).decode(np.zeros((2, 5), np.bool_))


def test_create_refuses_a_bad_graph_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()

    def create(n_nodes, u, v, n_cols=None):
        u, v = np.asarray(u, np.int32), np.asarray(v, np.int32)
        obs = np.zeros(len(u), np.uint64)
        desc = _lib.UfDesc(n_nodes, len(u), n_nodes if n_cols is None else n_cols, u.ctypes.data, v.ctypes.data, obs.ctypes.data)
        return lib.tsim_uf_create(0, C.byref(desc), C.byref(h)), lib.tsim_last_error()

    assert lib.tsim_uf_create(0, None, C.byref(h)) == -22 and lib.tsim_uf_info(None, (C.c_int64 * 16)()) == -22
    for nodes, u, v, what in ((4, [0, 0], [2, 1], b"strictly ascending"), (4, [0, 0], [1, 1], b"strictly ascending"),
                              (4, [2], [1], b"u < v"), (4, [1], [4], b"leaves the nodes"), (4, [-1], [2], b"leaves the nodes"),
                              (1, [], [], b"n_nodes")):
        rc, msg = create(nodes, u, v)
        assert rc == -22 and what in msg, (rc, msg)
    rc, msg = create(4, [0], [1], n_cols=2)
    assert rc == -22 and b"n_cols" in msg
    u = np.arange(19999)
    rc, msg = create(20000, u, u + 1)  # 8 bytes per node: 160 kB of LDS for one shot
    assert rc == -95 and b"bytes of LDS" in msg
    rc, msg = create(70000, [0], [1])
    assert rc == -95 and b"uint16" in msg
    assert h.value is None


# ---- count() on the host path ----------------------------------------------------------------------------------------------

def test_host_count_equals_the_tally_of_sample_and_decode(monkeypatch):
    monkeypatch.setattr(sampler_module, "sample_program", lambda *a, **k: pytest.fail("no program is sampled here"))
    c, uf = decoder_of(3, 5e-3)
    nd = uf.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[2, 11]] = True
    for method in ("faults", "frame"):
        for kw in ({}, dict(postselection_mask=mask)):
            rows = c.compile_detector_sampler(seed=4, method=method).sample(3000, append_observables=True)
            got = c.compile_detector_sampler(seed=4, method=method).count(3000, decoder=uf, **kw)
            keep = ~(rows[:, :nd] & kw.get("postselection_mask", np.zeros(nd, np.bool_))).any(axis=1)
            dets, obs = rows[keep, :nd], rows[keep, nd:]
            assert got.kept == int(keep.sum()) and got.decoder_misses == 0
            assert got.decoded_errors == int((uf.decode(dets) != obs).any(axis=1).sum())
            assert 0 < got.decoded_errors < got.kept_with_observable_flip
            assert got == tally_rows(rows, num_detectors=nd, decoder=uf, histogram_columns=(nd,), **kw)
    # the lookup decoder beside it: the same interface
    train = c.compile_detector_sampler(seed=9, method="faults").count(3000, pattern_columns="all")
    assert isinstance(LookupDecoder.from_counts(train).missed(rows[:, :nd]), np.ndarray)
