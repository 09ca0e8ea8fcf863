"""Sliding-window union-find decoding without a device (``tsim_amd.decode.WindowedUnionFindDecoder``): the window construction
against arrays written out by hand, the validity condition, one window against ``UnionFindDecoder``, the invariants of the
numpy statement on sampled syndromes, a graph beyond the uint16 limit, and ``count(decoder=wuf)`` on the host path."""

import time

import numpy as np
import pytest

from tsim_amd import circuits
from tsim_amd import sampler as sampler_module
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.counts import tally_rows
from tsim_amd.decode import MAX_GRAPH, DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder


def long_memory(d: int = 3, rounds: int = 12, p: float = 1e-2) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, before_measure_flip_probability=p))


def time_ladder(checks: int, rounds: int, *, both_ends: bool = True, skip: bool = False, limit=MAX_GRAPH):
    """``(graph, caps)``: ``checks`` detectors a round, column ``t * checks + s``; per node a space edge to ``(t, s + 1)`` (cap 4),
    a time edge to ``(t + 1, s)`` (cap 2) and a diagonal edge to ``(t + 1, s + 1)`` (cap 1); the checks ``s = 0`` have a
    boundary edge that flips observable 0 (cap 3), with ``both_ends`` the checks ``s = checks - 1`` one that flips nothing;
    ``skip``: the checks ``s = 0`` also have an edge to ``(t + 2, 0)`` (cap 2)."""
    t, s = (x.ravel() for x in np.meshgrid(np.arange(rounds), np.arange(checks), indexing="ij"))
    node = lambda t_, s_: 1 + t_ * checks + s_  # noqa: E731
    parts = [(np.zeros(rounds, np.int64), node(np.arange(rounds), 0), 3, 1)]
    if both_ends:
        parts.append((np.zeros(rounds, np.int64), node(np.arange(rounds), checks - 1), 3, 0))
    for m, dt, ds, cap in ((s < checks - 1, 0, 1, 4), (t < rounds - 1, 1, 0, 2), ((t < rounds - 1) & (s < checks - 1), 1, 1, 1),
                           ((t < rounds - 2) & (s == 0) & skip, 2, 0, 2)):
        parts.append((node(t[m], s[m]), node(t[m] + dt, s[m] + ds), cap, 0))
    u = np.concatenate([p[0] for p in parts])
    v = np.concatenate([p[1] for p in parts])
    caps = np.concatenate([np.full(len(p[0]), p[2], np.uint8) for p in parts])
    obs = np.concatenate([np.full(len(p[0]), p[3], np.uint64) for p in parts])
    order = np.lexsort((v, u))
    return DecodingGraph(checks * rounds + 1, u[order], v[order], obs[order], limit=limit), caps[order]


def fire(graph: DecodingGraph, rng, n: int, p=None) -> np.ndarray:
    """bool ``[n, nd]``: the syndromes of ``n`` draws in which every edge fires with its ``edge_p`` (or ``p``)."""
    out = np.zeros((n, graph.n_nodes), np.bool_)
    prob = graph.edge_p if p is None else p
    for r in range(n):
        f = np.flatnonzero(rng.random(graph.n_edges) < prob)
        np.logical_xor.at(out[r], graph.edge_u[f], True)
        np.logical_xor.at(out[r], graph.edge_v[f], True)
    return out[:, 1:]


def syndrome_of(graph: DecodingGraph, edges) -> np.ndarray:
    s = np.zeros(graph.n_nodes, np.bool_)
    np.logical_xor.at(s, graph.edge_u[edges], True)
    np.logical_xor.at(s, graph.edge_v[edges], True)
    return s[1:]


_CACHE: dict = {}


def d3():
    """``(circuit, whole-graph decoder, windowed decoder commit = 16, window = 32, 200 fired syndromes)``, built once."""
    if "d3" not in _CACHE:
        c = long_memory()
        uf = UnionFindDecoder.from_circuit(c)
        _CACHE["d3"] = (c, uf, WindowedUnionFindDecoder.from_circuit(c, 16, 32), fire(uf.graph, np.random.default_rng(1), 200))
    return _CACHE["d3"]


# ---- the construction --------------------------------------------------------------------------------------------------------

def test_windows_of_a_hand_made_ladder():
    """2 checks x 6 rounds, boundary edges at the checks s = 0 only, commit = 4, window = 8: two windows.  In window 0 the pair
    (0, 7) merges the real boundary edge of column 6 (cap 3, mask 1) with its time (cap 2) and diagonal (cap 1) edges to the
    future: cap 1, mask 1, REAL; the pair (0, 8) is the time edge of column 7 alone: purely virtual, cap 2, mask 0."""
    g, caps = time_ladder(2, 6, both_ends=False)
    assert list(zip(g.edge_u.tolist(), g.edge_v.tolist())) == [
        (0, 1), (0, 3), (0, 5), (0, 7), (0, 9), (0, 11), (1, 2), (1, 3), (1, 4), (2, 4), (3, 4), (3, 5), (3, 6), (4, 6), (5, 6), (5, 7), (5, 8),
        (6, 8), (7, 8), (7, 9), (7, 10), (8, 10), (9, 10), (9, 11), (9, 12), (10, 12), (11, 12)]
    w = WindowedUnionFindDecoder(g, 4, 8, edge_caps=caps)
    w0, w1 = w.windows()
    assert (w0.lo, w0.hi, w0.graph.n_nodes, w1.lo, w1.hi, w1.graph.n_nodes) == (0, 8, 9, 4, 12, 9)
    assert list(zip(w0.graph.edge_u.tolist(), w0.graph.edge_v.tolist())) == [
        (0, 1), (0, 3), (0, 5), (0, 7), (0, 8), (1, 2), (1, 3), (1, 4), (2, 4), (3, 4), (3, 5), (3, 6), (4, 6), (5, 6), (5, 7), (5, 8), (6, 8), (7, 8)]
    assert w0.global_edge.tolist() == [0, 1, 2, 3, -1, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18]
    assert w0.caps.tolist() == [3, 3, 3, 1, 2, 4, 2, 1, 2, 4, 2, 1, 2, 4, 2, 1, 2, 4]
    assert w0.graph.edge_obs.tolist() == [1, 1, 1, 1, 0] + [0] * 13
    assert w0.committed.tolist() == [True, True, False, False, False, True, True, True, True, True, True, True, True, False, False, False, False, False]
    assert list(zip(w1.graph.edge_u.tolist(), w1.graph.edge_v.tolist())) == [
        (0, 1), (0, 3), (0, 5), (0, 7), (1, 2), (1, 3), (1, 4), (2, 4), (3, 4), (3, 5), (3, 6), (4, 6), (5, 6), (5, 7), (5, 8), (6, 8), (7, 8)]
    assert w1.global_edge.tolist() == [2, 3, 4, 5] + list(range(14, 27))
    assert w1.caps.tolist() == [3, 3, 3, 3, 4, 2, 1, 2, 4, 2, 1, 2, 4, 2, 1, 2, 4]
    assert w1.graph.edge_obs.tolist() == [1, 1, 1, 1] + [0] * 13
    assert w1.committed.all()
    assert w.info()["n_windows"] == 2 and w.info()["max_window_nodes"] == 9 and w.info()["max_window_edges"] == 18
    # without caps every cap is 2, merged or not
    assert all((x.caps == 2).all() for x in WindowedUnionFindDecoder(g, 4, 8).windows())
    # an error on a committed edge of each window is undone by that edge
    for e in (8, 20, 25):
        row = syndrome_of(g, [e])[None, :]
        assert w.flipped_edges(row)[0].tolist() == [e] and not w.missed(row)[0]


def test_a_buffer_that_is_too_small_is_refused():
    c, _, w, _ = d3()
    with pytest.raises(ValueError, match="edge 110 = .6, 17.*too small"):
        WindowedUnionFindDecoder.from_circuit(c, 8, 16)
    info = w.info()
    assert (info["n_nodes"], info["n_edges"], info["n_windows"], info["max_window_nodes"]) == (97, 363, 5, 33)
    assert [(x.lo, x.hi) for x in w.windows()] == [(0, 32), (16, 48), (32, 64), (48, 80), (64, 96)]
    for bad in (dict(commit=0, window=8), dict(commit=8, window=8), dict(commit=4.0, window=8)):
        with pytest.raises(ValueError, match="commit"):
            WindowedUnionFindDecoder(w.graph, **bad)


def test_heralds_are_refused_and_the_default_limit_stands():
    g = DecodingGraph(4, [0, 1], [1, 2], np.zeros(2, np.uint64), node_det=[0, 1, 3], herald_det=[2], herald_ptr=[0, 1], herald_edges=[1])
    with pytest.raises(NotImplementedError, match="heralds"):
        WindowedUnionFindDecoder(g, 1, 2)
    u = np.arange(MAX_GRAPH)
    with pytest.raises(NotImplementedError, match="at most 65535 each: indices are uint16"):
        DecodingGraph(MAX_GRAPH + 1, u, u + 1, np.zeros(MAX_GRAPH, np.uint64))
    assert DecodingGraph(MAX_GRAPH + 1, u, u + 1, np.zeros(MAX_GRAPH, np.uint64), limit=None).n_nodes == MAX_GRAPH + 1
    with pytest.raises(NotImplementedError, match="at most 100 each"):
        DecodingGraph(102, u[:101], u[:101] + 1, np.zeros(101, np.uint64), limit=100)


# ---- the rule ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_is_the_whole_graph_decoder(weights):
    c, _, _, rows = d3()
    uf = UnionFindDecoder.from_circuit(c, weights=weights)
    for window in (96, 1000):
        w = WindowedUnionFindDecoder.from_circuit(c, 16, window, weights=weights)
        assert w.info()["n_windows"] == 1
        assert np.array_equal(w.predictions(rows), uf.predictions(rows)) and np.array_equal(w.missed(rows), uf.missed(rows))
        assert np.array_equal(w.growth_rounds(rows), uf.growth_rounds(rows)) and np.array_equal(w.decode(rows), uf.decode(rows))
        assert all(np.array_equal(a, b) for a, b in zip(w.flipped_edges(rows), uf.flipped_edges(rows)))
    assert uf.predictions(rows).any() and uf.growth_rounds(rows).max() >= 2


def test_invariants_on_fired_syndromes():
    """Every edge is committed in one window: that of its lowest column.  After window k the syndrome XOR the ends of the
    flips committed so far is zero on k's commit region, and zero everywhere at the end; the prediction is the XOR of the
    flips' masks."""
    _, uf, w, rows = d3()
    g, C, K = w.graph, w.commit, len(w.windows())
    assert not w.missed(rows).any() and rows.any(axis=1).sum() > 150
    low = np.where(g.edge_u > 0, g.edge_u, g.edge_v) - 1
    commit_window = np.minimum(low // C, K - 1)
    pred = w.predictions(rows)
    for row, flips, p in zip(rows, w.flipped_edges(rows), pred):
        assert np.array_equal(syndrome_of(g, flips), row)
        assert int(np.bitwise_xor.reduce(g.edge_obs[flips])) == int(p) if len(flips) else p == 0
        for k in range(K - 1):
            left = row ^ syndrome_of(g, flips[commit_window[flips] <= k])
            assert not left[k * C:(k + 1) * C].any()
    differ = int((pred != uf.predictions(rows)).sum())
    print(f"{differ} of {len(rows)} rows are predicted differently from the whole graph")  # (a figure, not a check)


def test_a_graph_beyond_uint16_builds_and_decodes():
    """8 checks x 8200 rounds: 65601 nodes, 196785 edges, 2049 windows of 65 nodes; built in seconds."""
    t0 = time.perf_counter()
    g, caps = time_ladder(8, 8200, limit=None)
    with pytest.raises(NotImplementedError):
        time_ladder(8, 8200)
    w = WindowedUnionFindDecoder(g, 32, 64, edge_caps=caps)
    built = time.perf_counter() - t0
    info = w.info()
    assert (info["n_nodes"], info["n_edges"], info["n_windows"], info["max_window_nodes"]) == (65601, 196785, 2049, 65)
    rows = fire(g, np.random.default_rng(2), 16, 2e-4)
    rows[0] = False
    assert rows[1:].any(axis=1).all() and not w.missed(rows).any() and w.predictions(rows).any()
    for row, flips in zip(rows, w.flipped_edges(rows)):
        assert np.array_equal(syndrome_of(g, flips), row)
    print(f"built in {built:.2f} s")
    assert built < 20


# ---- count() on the host path ----------------------------------------------------------------------------------------------

def test_host_count_equals_the_tally_of_sample_and_decode(monkeypatch):
    monkeypatch.setattr(sampler_module, "sample_program", lambda *a, **k: pytest.fail("no program is sampled here"))
    c, _, w, _ = d3()
    nd = w.num_detectors
    assert (nd, w.num_observables) == (96, 1)
    rows = c.compile_detector_sampler(seed=4, method="faults").sample(600, append_observables=True)
    got = c.compile_detector_sampler(seed=4, method="faults").count(600, decoder=w)
    dets, obs = rows[:, :nd], rows[:, nd:]
    assert got.kept == 600 and got.decoder_misses == int(w.missed(dets).sum()) == 0
    assert got.decoded_errors == int((w.decode(dets) != obs).any(axis=1).sum())
    assert 0 < got.decoded_errors < got.kept_with_observable_flip
    assert got == tally_rows(rows, num_detectors=nd, decoder=w, histogram_columns=(nd,))
