"""Erasure-aware union-find decoding without a device: the heralded surface code generator, the herald criterion on hand-written
circuits, ``heralds=False`` against the decoder as it was, the numpy statement with heralds against a restatement of the rule
on the herald-blind graph, the decoded errors with and without heralds, and what the constructor and
``tsim_uf_create_heralds`` refuse."""

import ctypes as C
import hashlib

import numpy as np
import pytest

from test_unionfind import chain_graph, memory, syndrome_of

from tsim_amd import _lib, circuits, faults
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.decode import DecodingGraph, UnionFindDecoder

GRAPH_ARRAYS = ("edge_u", "edge_v", "edge_obs", "edge_p", "node_det", "herald_det", "herald_ptr", "herald_edges")


def erasure_memory(d: int, rounds: int, p: float = 1e-3, pe: float = 1e-2) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p,
                                                                before_measure_flip_probability=p, after_clifford_heralded_erasure=pe))


_D3: dict = {}


def d3(pe: float = 1e-2):
    """``(circuit, form, herald-blind decoder, herald-aware decoder)`` of d = 3, 3 rounds, built once."""
    if pe not in _D3:
        c = erasure_memory(3, 3, pe=pe)
        _D3[pe] = (c, c.compile_faults(), UnionFindDecoder.from_circuit(c), UnionFindDecoder.from_circuit(c, heralds=True))
    return _D3[pe]


def same_graph(a: DecodingGraph, b: DecodingGraph) -> bool:
    return a.n_nodes == b.n_nodes and a.info() == b.info() and all(
        getattr(a, k).dtype == getattr(b, k).dtype and np.array_equal(getattr(a, k), getattr(b, k)) for k in GRAPH_ARRAYS)


# ---- the generator ---------------------------------------------------------------------------------------------------------

# sha256 of the text the generator gave before it knew heralds, with every noise argument set
TEXT_BEFORE = {(3, 3, "Z"): "ef70ea628dfc1c65815486dab80459a03b7512d4989861797629017127505340",
               (3, 1, "X"): "083372a428277d1bdc33fea7452339b38361aa1e3c060103258307d15d92b326",
               (5, 4, "X"): "466ea127cc53d0f9df49d50e1e3bcda15e058a40a452b11d879974e57a26c21f",
               (7, 2, "Z"): "bac2f4b0690a41db5afd4310477758cd331d501489291e50ed77e81616e5ff4c"}


@pytest.mark.parametrize("d,rounds,basis", sorted(TEXT_BEFORE))
def test_generator_without_erasure_gives_the_text_it_gave(d, rounds, basis):
    kw = dict(basis=basis, after_clifford_depolarization=1e-3, before_round_data_depolarization=2e-3,
              before_measure_flip_probability=3e-3, after_reset_flip_probability=4e-3)
    text = circuits.rotated_surface_code_memory(d, rounds, after_clifford_heralded_erasure=0.0, **kw)
    assert text == circuits.rotated_surface_code_memory(d, rounds, **kw) and "HERALDED" not in text
    assert hashlib.sha256(text.encode()).hexdigest() == TEXT_BEFORE[d, rounds, basis]


@pytest.mark.parametrize("d,rounds,basis", [(3, 3, "Z"), (3, 2, "X"), (5, 1, "Z")])
def test_generator_with_erasure_has_deterministic_detectors(d, rounds, basis):
    """The lookbacks over a cycle's heralds are right iff the noiseless circuit's detectors are all 0."""
    text = circuits.rotated_surface_code_memory(d, rounds, basis=basis, after_clifford_depolarization=1e-3,
                                                after_clifford_heralded_erasure=0.01)
    lines = text.split("\n")
    assert sum(line.startswith("HERALDED_ERASE(0.01)") for line in lines) == 4 * min(rounds, 2)
    at = next(i for i, line in enumerate(lines) if line.startswith("HERALDED_ERASE"))
    assert lines[at - 1].startswith("DEPOLARIZE2") and lines[at - 2].split()[1:] == lines[at].split()[1:]  # the layer's targets
    k = len(lines[at].split()) - 1
    assert lines[at + 1:at + 1 + k] == [f"DETECTOR rec[-{k - i}]" for i in range(k)]
    form = CliffordCircuit(text).compile_faults()
    assert not form.out_const.any()
    rows = faults.fault_rows_host(form, 0, 64, (1, 2)).view(np.bool_)
    quiet = CliffordCircuit(text.replace("(0.001)", "(0)").replace("(0.01)", "(0)")).compile_faults()
    assert not faults.fault_rows_host(quiet, 0, 16, (1, 2)).any() and rows.any()


def test_d3_graph_with_heralds():
    c, form, blind, aware = d3()
    g = aware.graph
    assert (blind.graph.n_nodes, blind.graph.n_heralds, blind.num_detectors) == (169, 0, 168)
    assert (g.n_nodes, g.n_heralds, g.num_detectors, aware.num_detectors, form.num_detectors) == (25, 144, 168, 168, 168)
    assert aware.info()["n_heralds"] == 144 and aware.info()["herald_bits_dropped"] == 0
    lengths = np.diff(g.herald_ptr)
    assert lengths.min() >= 1 and lengths.max() <= 2   # an X and a Z component, to the same edge or to two
    assert np.array_equal(np.sort(np.concatenate([g.node_det, g.herald_det])), np.arange(168))
    assert (np.diff(g.herald_det) > 0).all() and g.edge_p.min() > 0
    for h in range(g.n_heralds):
        own = g.herald_edges[g.herald_ptr[h]:g.herald_ptr[h + 1]]
        assert (np.diff(own) > 0).all()


# ---- the herald criterion --------------------------------------------------------------------------------------------------

BELL = "R 0 1\nH 0\nCX 0 1\n"
CHECKS = "MPP X0*X1\nDETECTOR rec[-1]\nMPP Z0*Z1\nDETECTOR rec[-1]\nOBSERVABLE_INCLUDE(0) rec[-1]"


def graphs(text):
    form = CliffordCircuit(text).compile_faults()
    return DecodingGraph.from_form(form), DecodingGraph.from_form(form, heralds=True)


def test_a_component_of_marginal_zero_is_not_listed():
    """``HERALDED_PAULI_CHANNEL_1(pi, px, 0, 0)``: the Z bit would flip the XX check, but never fires."""
    blind, aware = graphs(BELL + "HERALDED_PAULI_CHANNEL_1(0.1, 0.2, 0, 0) 0\nDETECTOR rec[-1]\n" + CHECKS)
    assert (blind.n_nodes, blind.edge_u.tolist(), blind.edge_v.tolist()) == (4, [0, 0], [1, 3])
    assert (aware.n_nodes, aware.num_detectors, aware.edge_u.tolist(), aware.edge_v.tolist()) == (3, 3, [0], [2])
    assert aware.node_det.tolist() == [1, 2] and aware.herald_det.tolist() == [0]
    assert aware.herald_ptr.tolist() == [0, 1] and aware.herald_edges.tolist() == [0]
    assert aware.edge_obs.tolist() == [1] and aware.edge_p[0] == pytest.approx(0.2)   # the unconditional marginal
    # with a Z component both checks are listed
    _, both = graphs(BELL + "HERALDED_PAULI_CHANNEL_1(0.1, 0.2, 0, 0.05) 0\nDETECTOR rec[-1]\n" + CHECKS)
    assert both.edge_v.tolist() == [1, 2] and both.herald_edges.tolist() == [0, 1]


def test_a_detector_over_two_herald_records_is_no_herald():
    blind, aware = graphs(BELL + "HERALDED_ERASE(0.1) 0 1\nDETECTOR rec[-1] rec[-2]\n" + CHECKS)
    assert aware.n_heralds == 0 and aware.n_nodes == 4 and same_graph(blind, aware)


def test_a_herald_record_without_a_detector_changes_nothing():
    blind, aware = graphs(BELL + "HERALDED_ERASE(0.1) 0\n" + CHECKS)
    assert aware.n_heralds == 0 and aware.n_nodes == 3 and same_graph(blind, aware)


def test_depolarize2_sites_have_no_herald():
    form = memory(3, 1e-3).compile_faults()
    blind, aware = DecodingGraph.from_form(form), DecodingGraph.from_form(form, heralds=True)
    assert aware.n_heralds == 0 and (aware.n_nodes, aware.n_edges) == (25, 78) and same_graph(blind, aware)


def test_a_component_with_three_detectors_is_dropped_and_the_list_is_empty():
    text = "R 0\nHERALDED_PAULI_CHANNEL_1(0, 0.1, 0, 0) 0\nDETECTOR rec[-1]\n" + "M 0\nDETECTOR rec[-1]\n" * 3
    blind, aware = graphs(text)
    assert blind.info()["dropped_bits"] == 1 and blind.info()["herald_bits_dropped"] == 0
    assert (aware.n_nodes, aware.n_edges, aware.n_heralds, aware.num_detectors) == (4, 0, 1, 4)
    assert aware.herald_det.tolist() == [0] and aware.herald_ptr.tolist() == [0, 0] and aware.node_det.tolist() == [1, 2, 3]
    assert aware.info()["herald_bits_dropped"] == 1 and aware.info()["dropped_bits"] == 1


# ---- heralds=False is the decoder as it was --------------------------------------------------------------------------------

def test_heralds_false_is_the_default_and_changes_nothing():
    c, form, blind, _ = d3()
    off = UnionFindDecoder.from_circuit(c, heralds=False)
    assert same_graph(blind.graph, off.graph) and same_graph(blind.graph, DecodingGraph.from_form(form))
    g = blind.graph
    assert (g.n_nodes, g.n_edges, g.n_heralds) == (169, 219, 0) and np.array_equal(g.node_det, np.arange(168))
    assert g.herald_ptr.tolist() == [0] and len(g.herald_edges) == 0 and blind.num_detectors == g.n_nodes - 1
    # the graph of the circuit without erasures is what the earlier tests pin down: 25 nodes, 78 edges
    plain = UnionFindDecoder.from_circuit(memory(3, 1e-3), heralds=False).graph
    assert (plain.n_nodes, plain.n_edges) == (25, 78) and np.array_equal(plain.node_det, np.arange(24))
    rows = faults.fault_rows_host(form, 0, 300, (1, 2)).view(np.bool_)[:, :168]
    assert np.array_equal(blind.predictions(rows), off.predictions(rows)) and np.array_equal(blind.growth_rounds(rows), off.growth_rounds(rows))
    w, w_off = UnionFindDecoder.from_circuit(c, weights="probability"), UnionFindDecoder.from_circuit(c, "probability", 4, False)
    assert np.array_equal(w.edge_caps, w_off.edge_caps) and np.array_equal(w.predictions(rows), w_off.predictions(rows))


# ---- the rule, restated on the herald-blind graph --------------------------------------------------------------------------

def restated(n, eu, ev, eobs, cap, defects, forbidden, prefilled):
    """The decoding rule of the module docstring in plain Python on one syndrome: ``forbidden`` edges never grow,
    ``prefilled`` edges start full.  ``(prediction, missed, growth rounds)``."""
    E = len(eu)
    grown = [0] * E
    for e in prefilled:
        grown[e] = cap[e]
    defect = [False] * n
    for v in defects:
        defect[v] = True
    rounds = 0
    while True:
        root = list(range(n))

        def find(x):
            while root[x] != x:
                x = root[x]
            return x
        for e in range(E):
            if grown[e] == cap[e]:
                a, b = find(eu[e]), find(ev[e])
                root[max(a, b)] = min(a, b)   # (the root of a cluster is its smallest node)
        label = [find(v) for v in range(n)]
        odd = [False] * n
        for v in range(n):
            if defect[v]:
                odd[label[v]] ^= True
        odd[0] = False
        active = [odd[label[v]] for v in range(n)]
        if not any(active):
            break
        new = [grown[e] if forbidden[e] else min(cap[e], grown[e] + active[eu[e]] + active[ev[e]]) for e in range(E)]
        if new == grown:
            return 0, True, rounds
        grown, rounds = new, rounds + 1
    full = [e for e in range(E) if grown[e] == cap[e]]
    level = [0 if label[v] == v else -1 for v in range(n)]
    parent = [-1] * n
    depth = 0
    while True:
        found = {}
        for e in full:   # (ascending: the first edge found is the smallest)
            for a, b in ((eu[e], ev[e]), (ev[e], eu[e])):
                if level[a] == depth and level[b] < 0:
                    found.setdefault(b, e)
        if not found:
            break
        for v, e in found.items():
            level[v], parent[v] = depth + 1, e
        depth += 1
    s = list(defect)
    prediction = 0
    for lv in range(depth, 0, -1):
        for v in range(n):
            if level[v] == lv and s[v]:
                e = parent[v]
                s[eu[e]] ^= True
                s[ev[e]] ^= True
                prediction ^= int(eobs[e])
    assert not any(s[1:])
    return prediction, False, rounds


@pytest.mark.parametrize("weighted", [False, True])
def test_statement_with_heralds_equals_the_rule_on_the_blind_graph(weighted):
    """The herald-blind graph of the d = 3 circuit with (1) the boundary edges of the herald detectors forbidden to grow, (2) the
    herald defects cleared and (3) the edges listed under the heralds that are set pre-filled decodes as ``heralds=True`` does:
    the other edges keep their order, so the comparison is exact."""
    c, form, blind, aware = d3(0.05)
    bg, g = blind.graph, aware.graph
    forbidden = (bg.edge_u == 0) & np.isin(bg.edge_v - 1, g.herald_det)
    assert int(forbidden.sum()) == 144 and bg.n_edges - 144 == g.n_edges
    to_blind = np.flatnonzero(~forbidden)   # aware edge -> blind edge
    node_col = np.concatenate([[-1], g.node_det])
    for e, be in enumerate(to_blind):
        assert (node_col[g.edge_u[e]] + 1, node_col[g.edge_v[e]] + 1, g.edge_obs[e]) == (bg.edge_u[be], bg.edge_v[be], bg.edge_obs[be])
    if weighted:
        aware = UnionFindDecoder(g, 1, g.growth_caps(4))
        cap = np.full(bg.n_edges, 14)
        cap[to_blind] = aware.edge_caps
    else:
        cap = np.full(bg.n_edges, 2)
    rows = np.unique(faults.fault_rows_host(form, 0, 400, (1, 2)).view(np.bool_)[:, :168], axis=0)
    pred, miss, rounds = aware.predictions(rows), aware.missed(rows), aware.growth_rounds(rows)
    is_herald = np.zeros(168, np.bool_)
    is_herald[g.herald_det] = True
    col_herald = {int(col): h for h, col in enumerate(g.herald_det)}
    eu, ev, eobs = bg.edge_u.tolist(), bg.edge_v.tolist(), bg.edge_obs.tolist()
    decoded = several = 0
    for r, row in enumerate(rows):
        if not (row & ~is_herald).any():
            assert pred[r] == 0 and not miss[r] and rounds[r] == 0
            continue
        set_heralds = [col_herald[int(col)] for col in np.flatnonzero(row & is_herald)]
        pre = sorted({int(to_blind[e]) for h in set_heralds for e in g.herald_edges[g.herald_ptr[h]:g.herald_ptr[h + 1]]})
        want = restated(169, eu, ev, eobs, cap.tolist(), (np.flatnonzero(row & ~is_herald) + 1).tolist(), forbidden.tolist(), pre)
        assert (int(pred[r]), bool(miss[r]), int(rounds[r])) == want, r
        decoded += 1
        several += len(set_heralds) > 1
    assert decoded > 200 and several > 150 and rounds.max() >= 2 and pred.any()


# ---- what it buys ----------------------------------------------------------------------------------------------------------

def test_heralds_cut_the_decoded_errors():
    """d = 3, 3 rounds, p = 1e-3, pe = 1e-2, 4000 rows under the key (1, 2), unweighted growth."""
    c, form, blind, aware = d3()
    rows = faults.fault_rows_host(form, 0, 4000, (1, 2)).view(np.bool_)
    dets, obs = rows[:, :168], rows[:, 168].astype(np.uint64)
    errors_blind = int((blind.predictions(dets) != obs).sum())
    errors_aware = int((aware.predictions(dets) != obs).sum())
    no_growth = int(((aware.growth_rounds(dets) == 0) & dets[:, aware.graph.node_det].any(axis=1)).sum())
    print(f"{int(obs.sum())} rows with an observable flip: {errors_blind} decoded errors herald-blind, {errors_aware} herald-aware; "
          f"{no_growth} of {int(dets[:, aware.graph.node_det].any(axis=1).sum())} rows with a defect took no growth round")
    assert not aware.missed(dets).any() and not blind.missed(dets).any()
    assert 2 * errors_aware < errors_blind
    assert np.array_equal(aware.decode(dets)[:, 0], aware.predictions(dets).astype(np.bool_))


def test_every_edge_under_one_herald_takes_no_growth_round():
    """A chain of 70 nodes whose 69 edges all hang under the herald of column 69: peeling alone, and a valid correction."""
    base = chain_graph()
    g = DecodingGraph(70, base.edge_u, base.edge_v, base.edge_obs, node_det=np.arange(69), herald_det=[69], herald_ptr=[0, 69],
                      herald_edges=np.arange(69))
    uf = UnionFindDecoder(g)
    assert uf.num_detectors == 70
    rng = np.random.default_rng(3)
    dets = rng.random((60, 70)) < 0.1
    dets[:, 69] = True
    dets[0, :69] = False    # heralds only: not decoded
    dets[1, :69] = True
    assert (uf.growth_rounds(dets) == 0).all() and not uf.missed(dets).any()
    for row, edges in zip(dets, uf.flipped_edges(dets)):
        assert np.array_equal(syndrome_of(g, edges), row[:69])
    assert len(uf.flipped_edges(dets)[0]) == 0 and uf.predictions(dets)[0] == 0
    # the same rows without the herald grow
    dets[:, 69] = False
    assert uf.growth_rounds(dets)[1:].min() >= 1 and UnionFindDecoder(base).growth_rounds(dets[:, :69]).tolist() == uf.growth_rounds(dets).tolist()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_constructor_refusals():
    u, obs = np.arange(4), np.zeros(4, np.uint64)
    ok = dict(node_det=[0, 2, 3, 5], herald_det=[1, 4], herald_ptr=[0, 1, 3], herald_edges=[3, 0, 3])
    g = DecodingGraph(5, u, u + 1, obs, **ok)
    assert (g.num_detectors, g.n_heralds) == (6, 2) and g.node_det.dtype == g.herald_edges.dtype == np.int32
    for bad, match in ((dict(herald_ptr=[0, 2, 1]), "herald_ptr"), (dict(herald_ptr=[0, 1, 2]), "herald_ptr"),
                       (dict(herald_edges=[3, 0, 4]), "edge 4"), (dict(node_det=[0, 3, 2, 5]), "ascending"),
                       (dict(herald_det=[1, 3]), "named twice"), (dict(herald_det=[1, 1]), "named twice"),
                       (dict(herald_det=[1, 6]), "column 6"), (dict(node_det=[0, 2, 3]), "node_det"),
                       (dict(herald_det=[1.0, 4.0]), "integers")):
        with pytest.raises(ValueError, match=match):
            DecodingGraph(5, u, u + 1, obs, **{**ok, **bad})
    with pytest.raises(NotImplementedError):
        DecodingGraph(65536, u, u + 1, obs, node_det=np.arange(65535))
    many = DecodingGraph(2, [0], [1], obs[:1], node_det=[70000], herald_det=np.arange(70000), herald_ptr=np.zeros(70001, np.int64))
    assert many.num_detectors == 70001   # (no limit on the heralds)
    with pytest.raises(ValueError, match=r"\[n, 6\]"):
        UnionFindDecoder(g).decode(np.zeros((2, 4), np.bool_))


def test_create_heralds_refusals_need_no_device():
    """Every check of ``tsim_uf_create_heralds`` comes before its first device call."""
    lib = _lib.load()
    eu, ev, eo = np.arange(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32), np.zeros(4, np.uint64)

    def create(n_cols=7, n_det_cols=6, caps=None, **kw):
        a = dict(node_det=[0, 2, 3, 5], herald_det=[1, 4], herald_ptr=[0, 1, 3], herald_edges=[3, 0, 3])
        a.update(kw)
        a = {k: np.array(v, np.int32) for k, v in a.items()}
        desc = _lib.UfDesc(5, 4, n_cols, eu.ctypes.data, ev.ctypes.data, eo.ctypes.data)
        her = _lib.UfHeralds(n_det_cols, len(a["herald_det"]), *(a[k].ctypes.data for k in ("node_det", "herald_det", "herald_ptr", "herald_edges")))
        h = C.c_void_p()
        rc = lib.tsim_uf_create_heralds(99, C.byref(desc), None if caps is None else C.c_void_p(caps.ctypes.data), C.byref(her), C.byref(h))
        assert not h.value
        return rc, lib.tsim_last_error().decode()

    for kw, match in ((dict(herald_det=[1, 3]), "named twice"), (dict(herald_det=[4, 4]), "named twice"),
                      (dict(herald_edges=[3, 0, 4]), "of 4 edges"), (dict(herald_edges=[3, -1, 0]), "of 4 edges"),
                      (dict(herald_ptr=[0, 2, 1]), "must not fall"), (dict(herald_ptr=[1, 1, 3]), "herald_ptr"),
                      (dict(n_cols=5), "n_cols = 5"), (dict(n_det_cols=7), "n_det_cols"), (dict(node_det=[0, 3, 2, 5]), "ascending"),
                      (dict(node_det=[0, 2, 3, 6]), "leaves the columns"), (dict(herald_det=[1, -4]), "leaves the columns"),
                      (dict(caps=np.array([1, 2, 15, 1], np.uint8)), "cap 15")):
        rc, msg = create(**kw)
        assert rc == -22 and match in msg, (kw, rc, msg)
    rc, msg = create()   # (everything is in order: the refusal is the device's, which does not exist)
    assert rc != 0 and "device" in msg.lower()
