"""Soft outputs of the sliding-window union-find decoder without a device (``WindowedUnionFindDecoder.soft_outputs`` /
``with_soft_output``; "Soft outputs in windows" in the module docstring of ``tsim_amd.decode``): one window against
``UnionFindDecoder``, the sums and maxima over many windows, rows worked out by hand, a miss, what is refused, and ``count()`` on
the host path."""

import numpy as np
import pytest

from test_unionfind_windowed import d3, fire, syndrome_of, time_ladder
from test_unionfind_windowed_erasure import LADDER_HERALD_COLS, herald_ladder

from tsim_amd import sampler as sampler_module
from tsim_amd.counts import tally_rows
from tsim_amd.decode import SOFT_OUTPUTS, DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder


def d3_fired():
    """256 rows of the d = 3, 12-round graph from edge firing (the rows the issue's figures are of)."""
    c, uf, _, _ = d3()
    return c, fire(uf.graph, np.random.default_rng(7), 256)


def miss_ladder():
    """``time_ladder(2, 6, both_ends=False)`` plus the nodes 13 and 14 joined by one edge and by nothing else: a component without
    a boundary edge in the columns 12 and 13, which only the last window of commit = 4, window = 8 holds."""
    base, _ = time_ladder(2, 6, both_ends=False)
    g = DecodingGraph(15, np.append(base.edge_u, 13), np.append(base.edge_v, 14), np.append(base.edge_obs, np.uint64(0)))
    return g, WindowedUnionFindDecoder(g, 4, 8)


def miss_rows(g) -> np.ndarray:
    """Three rows with a defect on node 13: alone; with the fired edge (1, 2); with a defect on node 1."""
    rows = np.zeros((3, 14), np.bool_)
    rows[:, 12] = True
    rows[1, [0, 1]] = True
    rows[2, 0] = True
    return rows


# what the rule gives for miss_rows, by hand.  The windows are [0, 8), [4, 12) and [8, 14); window 1 never has a defect.  In
# window 2 node 13 is local node 5: round 1 half-grows its one edge, round 2 fills it, round 3 changes nothing: a miss after 2
# rounds with 1 full edge and a cluster of 2.  Window 0 of row 1: the edge (1, 2) gets 2 in round 1 and is full, the cluster of
# both defects is even: 1 round, 1 full edge, a cluster of 2.  Window 0 of row 2: node 1 has the edges (0, 1), (1, 2), (1, 3) and
# (1, 4), full after 2 rounds: 4 full edges, a cluster of 5 with the boundary.  A miss has weight 0.
MISS_ROWS_BY_HAND = [[2, 1, 2, 0], [2, 2, 2, 0], [2, 5, 5, 0]]


@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_is_the_whole_graph_decoder(weights):
    c, rows = d3_fired()
    uf = UnionFindDecoder.from_circuit(c, weights=weights)
    want = uf.soft_outputs(rows)
    for window in (96, 1000):
        w = WindowedUnionFindDecoder.from_circuit(c, 16, window, weights=weights)
        assert w.info()["n_windows"] == 1 and np.array_equal(w.soft_outputs(rows), want)
    assert want.dtype == np.int64 and want.shape == (256, 4) and (want.max(axis=0) >= [2, 20, 10, 5]).all()


@pytest.mark.parametrize("weighted", [False, True])
def test_one_window_with_heralds_is_the_whole_graph_decoder(weighted):
    g, caps = herald_ladder()
    rng = np.random.default_rng(3)
    rows = np.zeros((300, 18), np.bool_)
    rows[:, g.node_det] = fire(g, rng, 300, 0.08)
    rows[:, LADDER_HERALD_COLS] = rng.random((300, 6)) < 0.3
    uf = UnionFindDecoder(g, edge_caps=caps if weighted else None)
    w = WindowedUnionFindDecoder(g, 4, 12, edge_caps=caps if weighted else None, heralds=True)
    assert w.info()["n_windows"] == 1 and np.array_equal(w.soft_outputs(rows), uf.soft_outputs(rows))
    blind = rows.copy()
    blind[:, LADDER_HERALD_COLS] = False
    assert (uf.soft_outputs(rows)[:, 1] != uf.soft_outputs(blind)[:, 1]).any()   # (pre-grown edges are full edges)
    only_heralds = rows[~rows[:, g.node_det].any(axis=1)]
    assert only_heralds[:, LADDER_HERALD_COLS].any() and not w.soft_outputs(only_heralds).any()


@pytest.mark.parametrize("weights", [None, "probability"])
def test_many_windows(weights):
    c, rows = d3_fired()
    rows = rows.copy()
    rows[:8] = False
    rows[8:24, :80] = False   # defects in the columns [80, 96) lie in the last window, [64, 96), and in no other
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights=weights)
    whole = UnionFindDecoder.from_circuit(c, weights=weights)
    soft = w.soft_outputs(rows)
    assert len(w.windows()) == 5 and soft.dtype == np.int64 and soft.shape == (256, 4)
    assert np.array_equal(soft[:, 0], w.growth_rounds(rows))
    assert np.array_equal(soft[:, 3], [len(f) for f in w.flipped_edges(rows)])
    assert not soft[:8].any() and (soft[rows.any(axis=1), 1:3] >= 1).all()
    assert (soft != whole.soft_outputs(rows)).any(axis=0).all()   # (windows are not the whole graph, in any of the four)
    distinct = [len(np.unique(soft[:, k])) for k in range(4)]
    print(f"weights = {weights}: distinct values {distinct}, largest {soft.max(axis=0).tolist()}")
    assert min(distinct) >= 2 and max(distinct) >= 16
    last = w.windows()[-1]
    one = rows[8:24][rows[8:24].any(axis=1)]
    assert len(one) >= 4 and (last.lo, last.hi) == (64, 96)
    alone = UnionFindDecoder(last.graph, 1, None if weights is None else last.caps).soft_outputs(one[:, 64:])
    assert np.array_equal(w.soft_outputs(one)[:, 1:3], alone[:, 1:3]) and np.array_equal(w.soft_outputs(one)[:, 0], alone[:, 0])


def test_a_row_by_hand():
    """2 checks x 6 rounds with skip edges, no caps, commit = 2, window = 6: the windows [0, 6), [2, 8), [4, 10), [6, 12).  The skip
    edge (5, 9) fires: defects at the columns 4 and 8.
    Window 0 sees column 4 alone, local node 5, whose edges are (0, 5) - the real boundary edge merged with the edges to the future
    -, (1, 5), (3, 5) and (5, 6): half after round 1, full after round 2, and the cluster {0, 1, 3, 5, 6} holds the boundary: 2 rounds,
    4 full edges, a cluster of 5.  Peeling flips (0, 5), which is not committed (column 4 is outside [0, 2)).
    Window 1 sees column 4 alone, local node 3, with the edges (0, 3) - the skip edge (5, 9) leaves the window and merges into it -,
    (1, 3), (3, 4), (3, 5) and (3, 6); the skip edge (1, 5) is left out: 2 rounds, 5 full edges, a cluster of 6; nothing is committed.
    Window 2 sees both defects, local nodes 1 and 5, and the skip edge between them grows from both ends: full after round 1, the
    cluster is even: 1 round, 1 full edge, a cluster of 2, and the flip is committed (column 4 is in [4, 6)).  Window 3 is clean.
    So: rounds max(2, 2, 1), full edges 4 + 5 + 1, largest cluster max(5, 6, 2), one committed flip."""
    g, _ = time_ladder(2, 6, both_ends=False, skip=True)
    w = WindowedUnionFindDecoder(g, 2, 6)
    assert [(x.lo, x.hi) for x in w.windows()] == [(0, 6), (2, 8), (4, 10), (6, 12)]
    e = int(np.flatnonzero((g.edge_u == 5) & (g.edge_v == 9))[0])
    row = syndrome_of(g, [e])[None, :]
    assert np.flatnonzero(row[0]).tolist() == [4, 8]
    assert w.soft_outputs(row).tolist() == [[2, 10, 6, 1]]
    assert w.flipped_edges(row)[0].tolist() == [e] and not w.missed(row)[0]
    assert UnionFindDecoder(g).soft_outputs(row).tolist() == [[1, 1, 2, 1]]   # (the whole graph sees the edge at once)


def test_a_miss_keeps_its_growth_and_has_no_weight():
    g, w = miss_ladder()
    assert [(x.lo, x.hi) for x in w.windows()] == [(0, 8), (4, 12), (8, 14)]
    rows = miss_rows(g)
    assert w.missed(rows).all() and not w.predictions(rows).any() and all(len(f) == 0 for f in w.flipped_edges(rows))
    assert w.soft_outputs(rows).tolist() == MISS_ROWS_BY_HAND
    # without the defect on the component the same rows decode, and the earlier window is all there is
    rows[:, 12] = False
    assert not w.missed(rows).any() and w.soft_outputs(rows).tolist() == [[0, 0, 0, 0], [1, 1, 2, 1], [2, 4, 5, 1]]


def test_with_soft_output():
    c, _, w, rows = d3()
    uf = UnionFindDecoder.from_circuit(c)
    assert w.soft_output is None and w.soft_bins is None and hasattr(w, "with_soft_output") and not hasattr(w, "with_gap_output")
    soft = w.with_soft_output("full_edges", 8)
    assert isinstance(soft, WindowedUnionFindDecoder) and (soft.soft_output, soft.soft_bins) == ("full_edges", 8)
    assert w.soft_output is None and w.with_soft_output("rounds").soft_bins == 64
    assert soft.graph is w.graph and soft._windows is w._windows and soft._decoders is w._decoders
    assert soft._cache is w._cache and soft._window_cache is w._window_cache and (soft.commit, soft.window) == (w.commit, w.window)
    assert np.array_equal(soft.predictions(rows), w.predictions(rows))
    for bad, match in (("confidence", "metric = 'confidence': one of rounds, full_edges, largest_cluster, correction_weight"),
                       (2, "metric = 2"), (None, "metric = None")):
        for dec in (w, uf):
            with pytest.raises(ValueError, match=match):
                dec.with_soft_output(bad)
    for bad in (1, 1025, 0, -3, 8.0, True, None):
        for dec in (w, uf):
            with pytest.raises(ValueError, match=r"bins = .*: an int in 2 \.\. 1024"):
                dec.with_soft_output("rounds", bad)
    with pytest.raises(ValueError, match=r"the decoder has no soft output: with_soft_output\(metric, bins\)"):
        w.soft_bin_counts(rows, np.zeros(len(rows), np.bool_))


@pytest.mark.parametrize("metric", SOFT_OUTPUTS)
def test_bin_counts(metric):
    _, _, w, rows = d3()
    soft = w.with_soft_output(metric, 8)
    wrong = np.random.default_rng(2).random(len(rows)) < 0.2
    kept, errors = soft.soft_bin_counts(rows, wrong)
    values = np.minimum(w.soft_outputs(rows)[:, SOFT_OUTPUTS.index(metric)], 7)
    assert kept.dtype == errors.dtype == np.int64 and kept.shape == errors.shape == (8,)
    assert np.array_equal(kept, np.bincount(values, minlength=8)) and np.array_equal(errors, np.bincount(values[wrong], minlength=8))
    assert kept.sum() == len(rows) and errors.sum() == wrong.sum() and (kept > 0).sum() >= 2


def test_host_count_equals_the_tally_of_sample_and_decode(monkeypatch):
    monkeypatch.setattr(sampler_module, "sample_program", lambda *a, **k: pytest.fail("no program is sampled here"))
    c, _, w, _ = d3()
    nd = w.num_detectors
    soft = w.with_soft_output("largest_cluster", 16)
    mask = np.zeros(nd, np.bool_)
    mask[[0, 70]] = True
    rows = c.compile_detector_sampler(seed=4, method="faults").sample(600, append_observables=True)
    got = c.compile_detector_sampler(seed=4, method="faults").count(600, decoder=soft, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, decoder=soft, postselection_mask=mask, histogram_columns=(nd,))
    assert got == want and got.soft_output == "largest_cluster"
    assert int(got.soft_kept.sum()) == got.kept < 600 and int(got.soft_errors.sum()) == got.decoded_errors > 0
    keep = ~(rows[:, :nd] & mask).any(axis=1)
    dets, obs = rows[keep, :nd], rows[keep, nd:]
    kept, errors = soft.soft_bin_counts(dets, (w.decode(dets) != obs).any(axis=1))
    assert np.array_equal(got.soft_kept, kept) and np.array_equal(got.soft_errors, errors) and (kept > 0).sum() >= 4
    accepted, wrong = got.rejection_curve()
    assert (accepted[-1], wrong[-1]) == (got.kept, got.decoded_errors)
    plain = c.compile_detector_sampler(seed=4, method="faults").count(600, decoder=w, postselection_mask=mask)
    assert plain.soft_output is None and plain.soft_kept is None and (plain.kept, plain.decoded_errors) == (got.kept, got.decoded_errors)
