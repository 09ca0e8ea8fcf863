"""Soft outputs of the union-find decoder without a device ("Soft outputs" in the module docstring of ``tsim_amd/decode.py``):
``soft_outputs()`` against a slow per-row restatement of the rule, its columns against ``growth_rounds()`` and
``flipped_edges()``, ``with_soft_output``, the host tally's histograms and ``ShotCounts.rejection_curve()``."""

import numpy as np
import pytest

from test_unionfind import chain_graph, memory, no_boundary_graph
from test_unionfind_erasure import erasure_memory

from tsim_amd import faults
from tsim_amd.counts import ShotCounts, tally_rows
from tsim_amd.decode import UnionFindDecoder, WindowedUnionFindDecoder

METRICS = ("rounds", "full_edges", "largest_cluster", "correction_weight")


def restated(uf: UnionFindDecoder, dets: np.ndarray) -> np.ndarray:
    """int64 ``[n, 4]`` by the docstring, a row and an edge at a time: synchronous growth on plain Python integers, the clusters by
    a union over the full edges, the correction weight from ``flipped_edges``."""
    g = uf.graph
    n, eu, ev = g.n_nodes, g.edge_u.tolist(), g.edge_v.tolist()
    cap = [2] * g.n_edges if uf.edge_caps is None else [int(c) for c in uf.edge_caps]
    out = np.zeros((len(dets), 4), np.int64)
    seen: dict = {}
    weights = [len(x) for x in uf.flipped_edges(dets)]
    for r, row in enumerate(dets):
        key = row.tobytes()
        if key in seen:
            out[r] = out[seen[key]]
            continue
        seen[key] = r
        defect = [False] + [bool(row[c]) for c in g.node_det]
        if not any(defect):
            continue   # (not decoded, whatever its heralds say)
        grown = [0] * g.n_edges
        for h in np.flatnonzero(row[g.herald_det]):
            for e in g.herald_edges[g.herald_ptr[h]:g.herald_ptr[h + 1]]:
                grown[e] = cap[e]
        rounds = 0
        while True:
            root = list(range(n))

            def find(x):
                while root[x] != x:
                    x = root[x]
                return x

            for e in range(g.n_edges):
                if grown[e] == cap[e]:
                    a, b = find(eu[e]), find(ev[e])
                    root[max(a, b)] = min(a, b)
            cluster = [find(v) for v in range(n)]
            odd = [False] * n
            for v in range(n):
                if defect[v]:
                    odd[cluster[v]] = not odd[cluster[v]]
            odd[cluster[0]] = False
            if not any(odd):
                miss = False
                break
            new = [min(cap[e], grown[e] + odd[cluster[eu[e]]] + odd[cluster[ev[e]]]) for e in range(g.n_edges)]
            if new == grown:
                miss = True
                break
            grown, rounds = new, rounds + 1
        sizes = np.bincount(cluster, minlength=n)
        out[r] = rounds, sum(grown[e] == cap[e] for e in range(g.n_edges)), sizes.max(), 0 if miss else weights[r]
    return out


_CASES: dict = {}


def case(name: str):
    """``(decoder, bool rows of detectors and observables)``, built once."""
    if name not in _CASES:
        if name in ("d3", "d3_weighted"):
            c = memory(3, 0.02, 3)
            uf = UnionFindDecoder.from_circuit(c, weights="probability" if name == "d3_weighted" else None)
            bits = faults.fault_rows_host(c.compile_faults(), 0, 4133, (1, 2)).view(np.bool_)
        elif name == "no_boundary":
            uf = UnionFindDecoder(no_boundary_graph())
            bits = np.random.default_rng(11).integers(0, 2, (200, 5)).astype(np.bool_)
        elif name == "chain":
            uf = UnionFindDecoder(chain_graph())
            rng = np.random.default_rng(11)
            bits = np.zeros((120, 70), np.bool_)
            for r in range(3, 120):
                bits[r, rng.choice(69, size=int(rng.integers(0, 5)), replace=False)] = True
            bits[0, [29, 49]] = bits[1, [44, 64]] = bits[2, [4, 67]] = True
            bits[:, 69] = rng.integers(0, 2, size=120).astype(np.bool_)
        else:
            c = erasure_memory(3, 3, pe=0.05)
            uf = UnionFindDecoder.from_circuit(c, heralds=True)
            bits = faults.fault_rows_host(c.compile_faults(), 0, 512, (1, 2)).view(np.bool_).copy()
            bits[:8, uf.graph.node_det] = False   # heralds only
            assert bits[:8, uf.graph.herald_det].any(axis=1).all()
        _CASES[name] = (uf, bits)
    return _CASES[name]


@pytest.mark.parametrize("name", ["d3", "d3_weighted", "no_boundary", "chain", "heralds"])
def test_soft_outputs_against_the_restatement(name):
    uf, bits = case(name)
    nd = uf.num_detectors
    dets = bits[:, :nd]
    got = uf.soft_outputs(dets)
    assert got.dtype == np.int64 and got.shape == (len(bits), 4)
    assert np.array_equal(got, restated(uf, dets))
    assert np.array_equal(got[:, 0], uf.growth_rounds(dets))
    assert np.array_equal(got[:, 3], [len(x) for x in uf.flipped_edges(dets)])
    quiet = ~dets[:, uf.graph.node_det].any(axis=1)
    assert quiet.any() and not got[quiet].any() and (got[~quiet, 2] >= 1).all()
    missed = uf.missed(dets)
    assert not got[missed, 3].any() and (got[~quiet & ~missed, 3] >= 1).all()
    # the margins the inputs are chosen for
    wrong = (uf.decode(dets) != bits[:, nd:nd + uf.num_observables]).any(axis=1)
    if name == "d3":
        assert int(wrong.sum()) == 557 and got.max(axis=0).tolist() == [2, 60, 25, 14]
    if name == "d3_weighted":
        assert int(wrong.sum()) == 498 and got.max(axis=0).tolist() == [7, 28, 19, 11]
    if name == "no_boundary":
        assert int(missed.sum()) == 103 and got[missed, 1:3].min() >= 1   # a miss keeps the state its growth ended in
    if name == "chain":
        assert got[:, 0].max() > 64   # over the default bins
    if name == "heralds":
        only = quiet & dets[:, uf.graph.herald_det].any(axis=1)
        assert only.sum() >= 8 and not got[only].any()
        assert (got[:, 0] == 0)[~quiet].any()   # pre-grown edges alone can end the growth before its first round


def test_the_existing_answers_are_unchanged_by_the_soft_entries():
    uf, bits = case("d3")
    fresh = UnionFindDecoder(uf.graph, uf.num_observables)
    dets = bits[:300, :uf.num_detectors]
    one = fresh._decode_one(np.flatnonzero(dets[5]) + 1)
    assert len(one) == 4 and one[0] == int(uf.predictions(dets[5:6])[0])
    assert np.array_equal(fresh.predictions(dets), uf.predictions(dets)) and np.array_equal(fresh.missed(dets), uf.missed(dets))


def test_small_clusters_are_decoded_better():
    """The confidence the soft output is for: accepting only the shots whose largest cluster has at most 4 nodes leaves a smaller
    error fraction than accepting all of them."""
    uf, bits = case("d3")
    nd = uf.num_detectors
    wrong = (uf.decode(bits[:, :nd]) != bits[:, nd:]).any(axis=1)
    accept = uf.soft_outputs(bits[:, :nd])[:, 2] <= 4
    print(f"accepted {int(accept.sum())} of {len(bits)}: {int(wrong[accept].sum())} errors against {int(wrong.sum())}")
    assert 0 < accept.sum() < len(bits)
    assert wrong[accept].sum() / accept.sum() < wrong.sum() / len(bits)


def test_with_soft_output_arguments():
    uf, _ = case("d3_weighted")
    assert uf.soft_output is None and uf.soft_bins is None
    soft = uf.with_soft_output("largest_cluster")
    assert isinstance(soft, UnionFindDecoder) and soft is not uf and (soft.soft_output, soft.soft_bins) == ("largest_cluster", 64)
    assert soft.graph is uf.graph and soft.edge_caps is uf.edge_caps and soft.num_observables == uf.num_observables
    assert uf.soft_output is None
    for m in METRICS:
        assert uf.with_soft_output(m, bins=2).soft_output == m
    assert uf.with_soft_output("rounds", 1024).soft_bins == 1024 and soft.with_soft_output("rounds", np.int64(7)).soft_bins == 7
    for bad in ("cluster", None, 2, "ROUNDS"):
        with pytest.raises(ValueError, match="metric"):
            uf.with_soft_output(bad)
    for bad in (1, 0, -3, 1025, 64.0, "64", True, None):
        with pytest.raises(ValueError, match="bins"):
            uf.with_soft_output("rounds", bad)
    assert not hasattr(WindowedUnionFindDecoder, "with_soft_output")
    with pytest.raises(ValueError, match="soft output"):
        uf.soft_bin_counts(np.zeros((1, uf.num_detectors), np.bool_), np.zeros(1, np.bool_))


@pytest.mark.parametrize("metric,bins", [("rounds", 64), ("full_edges", 16), ("largest_cluster", 64), ("largest_cluster", 2),
                                         ("correction_weight", 8)])
def test_tally_rows_fills_the_histograms(metric, bins):
    uf, bits = case("d3")
    nd = uf.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[0, 13]] = True
    soft = uf.with_soft_output(metric, bins)
    plain = tally_rows(bits, num_detectors=nd, postselection_mask=mask, decoder=uf)
    got = tally_rows(bits, num_detectors=nd, postselection_mask=mask, decoder=soft)
    assert plain.soft_output is None and plain.soft_kept is None and plain.soft_errors is None
    assert got.soft_output == metric and got.soft_kept.shape == got.soft_errors.shape == (bins,)
    assert got.soft_kept.dtype == got.soft_errors.dtype == np.int64
    assert int(got.soft_kept.sum()) == got.kept < len(bits) and int(got.soft_errors.sum()) == got.decoded_errors == plain.decoded_errors > 0
    assert (got.soft_errors <= got.soft_kept).all()
    # bin by bin against the statement
    keep = ~(bits[:, :nd] & mask).any(axis=1)
    raw = uf.soft_outputs(bits[keep, :nd])[:, METRICS.index(metric)]
    value = np.minimum(raw, bins - 1)
    wrong = (uf.decode(bits[keep, :nd]) != bits[keep, nd:]).any(axis=1)
    assert np.array_equal(got.soft_kept, np.bincount(value, minlength=bins))
    assert np.array_equal(got.soft_errors, np.bincount(value[wrong], minlength=bins))
    assert (raw.max() >= bins) == (bins < 64) and got.soft_kept[min(int(raw.max()), bins - 1)] > 0   # the small bin counts clamp
    # every other field is the plain decoder's
    fields = [f for f in ShotCounts.__dataclass_fields__ if not f.startswith("soft_")]
    assert ShotCounts(*(getattr(got, f) for f in fields)) == plain
    accepted, errors = got.rejection_curve()
    assert accepted.shape == errors.shape == (bins,) and (accepted[-1], errors[-1]) == (got.kept, got.decoded_errors)
    assert (np.diff(accepted) >= 0).all() and (np.diff(errors) >= 0).all()
    assert np.array_equal(accepted, np.cumsum(got.soft_kept)) and np.array_equal(errors, np.cumsum(got.soft_errors))
    with pytest.raises(ValueError, match="soft output"):
        plain.rejection_curve()


def test_tally_in_parts_and_empty():
    from tsim_amd import counts

    uf, bits = case("d3")
    nd = uf.num_detectors
    soft = uf.with_soft_output("correction_weight", 6)
    whole = tally_rows(bits[:900], num_detectors=nd, decoder=soft)
    parts = counts._HostTally(nd + 1, nd, None, (), decoder=soft)
    parts.add(bits[:400])
    parts.add(bits[400:900])
    assert parts.result() == whole
    empty = counts._HostTally(nd + 1, nd, None, (), decoder=soft).result()
    assert empty.soft_output == "correction_weight" and empty.soft_kept.tolist() == [0] * 6 and empty.soft_errors.tolist() == [0] * 6
    assert empty.rejection_curve()[0].tolist() == [0] * 6


def test_shot_counts_equality_with_the_soft_fields():
    base = (10, 4, 1, np.array([1, 2, 3, 0, 1]), 3, (3, 4), np.array([2, 1, 0, 1]), (), None, (), None, None, 0, 2, 0)
    k, e = np.array([3, 1]), np.array([1, 1])
    plain = ShotCounts(*base)
    assert plain == ShotCounts(*base) and plain.soft_output is None and plain.soft_kept is None and plain.soft_errors is None
    a = ShotCounts(*base, "rounds", k, e)
    assert a == ShotCounts(*base, "rounds", k.copy(), e.copy())
    assert a != plain and plain != a
    assert a != ShotCounts(*base, "full_edges", k, e)
    assert a != ShotCounts(*base, "rounds", np.array([2, 2]), e)
    assert a != ShotCounts(*base, "rounds", k, np.array([2, 0]))
    assert a != ShotCounts(*base, "rounds", np.array([3, 1, 0]), np.array([1, 1, 0]))
    assert a != ShotCounts(*base, "rounds", k, None)
    assert a.rejection_curve()[0].tolist() == [3, 4] and a.rejection_curve()[1].tolist() == [1, 2]
