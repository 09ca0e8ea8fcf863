"""Soft outputs of the sliding-window union-find decoder on the GPU (``tsim_ufw_decode_soft_device``, ``k_ufw<Weighted, Heralds,
true>`` of ``csrc/tsim_ufw.hip.h``): every prediction, the three counters, the four values of every row (``d_soft`` as
``uint32[n, 4]``) and both histograms bit for bit against the numpy statement (``WindowedUnionFindDecoder.soft_outputs``), on both
kinds of handle, with masks, on a miss, accumulating, beside the whole-graph handle, through ``count()``, and what the entry
refuses."""

import numpy as np
import pytest

from test_gpu_unionfind import packed
from test_gpu_unionfind_soft import METRICS, same, soft_on_device, soft_statement
from test_gpu_unionfind_windowed import d3_rows, with_observables
from test_gpu_unionfind_windowed_erasure import d3 as heralded_d3
from test_unionfind_windowed import fire, time_ladder
from test_unionfind_windowed_erasure import LADDER_HERALD_COLS, herald_ladder
from test_unionfind_windowed_soft import MISS_ROWS_BY_HAND, miss_ladder, miss_rows

from tsim_amd import synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import ShotCounts, tally_rows
from tsim_amd.decode import UnionFindDecoder, WindowedUnionFindDecoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


_DECODERS: dict = {}


def d3_windowed(weights, window=32):
    """The windowed decoder of the d = 3, 12-round circuit, commit = 16, built once (its caches fill once, too)."""
    if (weights, window) not in _DECODERS:
        _DECODERS[weights, window] = WindowedUnionFindDecoder.from_circuit(d3_rows()[0], 16, window, weights=weights)
    return _DECODERS[weights, window]


@pytest.mark.parametrize("metric,bins,weights", [(m, 8, None) for m in METRICS] + [
    ("full_edges", 8, "probability"), ("largest_cluster", 8, "probability"), ("full_edges", 1024, None), ("correction_weight", 1024, "probability")])
def test_d3_rows_bit_for_bit(hp, metric, bins, weights):
    """5 windows of 32 columns, a carry bitmap of exactly 32 bits that wraps twice; 8 rows without a defect, 16 with defects in the
    last window only; 8 bins clip the top one, 1024 clip nothing."""
    _, bits = d3_rows()
    soft = d3_windowed(weights).with_soft_output(metric, bins)
    assert soft.info()["n_windows"] == 5 and not bits[:8, :96].any() and bits[8:24, 64:96].any(axis=1).all() and not bits[8:24, :64].any()
    want = soft_statement(soft, bits)
    top = int(want[2][:, METRICS.index(metric)].max())
    assert want[1][0] == 256 and 0 < want[1][1] < 256 and not want[2][:8].any() and want[3][0][0] >= 8
    assert (want[3][0] > 0).sum() >= 2 and want[3][0][min(top, bins - 1)] > 0
    if metric != "rounds":
        assert (top >= bins) == (bins == 8)   # the clamp is exercised by 8 bins, and 1024 hold every value
    whole = UnionFindDecoder.from_circuit(d3_rows()[0], weights=weights).soft_outputs(bits[:, :96])
    assert (want[2] != whole).any(axis=0).all()   # (windows are not the whole graph)
    same(soft_on_device(hp, soft, bits, 13, np.random.default_rng(1)), want, f"d = 3, {metric} in {bins} bins, weights = {weights}")


@pytest.mark.parametrize("weighted", [False, True])
def test_the_skip_ladder(hp, weighted):
    """2 checks with edges that skip a round, commit = 2, window = 6: overlapping windows fill the same edges, and count them twice."""
    g, caps = time_ladder(2, 6, both_ends=False, skip=True)
    rng = np.random.default_rng(3)
    w = WindowedUnionFindDecoder(g, 2, 6, edge_caps=caps if weighted else None)
    bits = with_observables(fire(g, rng, 300, 0.08), rng)
    for metric in ("full_edges", "correction_weight"):
        soft = w.with_soft_output(metric, 8)
        want = soft_statement(soft, bits)
        assert want[2][:, 1].max() > g.n_edges // 2 and want[2][:, 3].max() >= 3
        same(soft_on_device(hp, soft, bits, 2, rng), want, f"skip ladder, weighted = {weighted}, {metric}")


def test_masks_and_a_ragged_row_count(hp):
    """``d_xor`` and ``d_test``, 201 rows (no multiple of 64) at an odd address: a row that is not kept has four zeros and is in no bin."""
    _, bits = d3_rows()
    soft = d3_windowed(None).with_soft_output("largest_cluster", 8)
    rng = np.random.default_rng(5)
    xor = rng.random(97) < 0.05
    test = np.zeros(97, np.bool_)
    test[[3, 50, 90]] = True
    want = soft_statement(soft, bits[:201], xor, test)
    keep = ~((bits[:201] ^ xor) & test).any(axis=1)
    assert 0 < want[1][0] == int(keep.sum()) < 201 and want[1][1] > 0 and not want[2][~keep].any() and want[2][keep].any()
    assert int(want[3][0].sum()) == int(keep.sum())
    got = soft_on_device(hp, soft, bits[:201], 16, rng, xor=xor, test=test, offset=3)
    same(got, want, "masks")
    assert not got[2][~keep].any() and int(got[3][0].sum()) == int(keep.sum())


@pytest.mark.parametrize("weighted", [False, True])
def test_the_herald_ladder(hp, weighted):
    """A herald across ``hi_0``, a merged pair, a shared edge, an empty list: the edges a herald pre-grows are full edges."""
    g, caps = herald_ladder()
    w = WindowedUnionFindDecoder(g, 4, 8, edge_caps=caps if weighted else None, heralds=True)
    rng = np.random.default_rng(3)
    bits = np.zeros((300, 19), np.bool_)
    bits[:, g.node_det] = fire(g, rng, 300, 0.08)
    bits[:, LADDER_HERALD_COLS] = rng.random((300, 6)) < 0.3
    bits[:, 18] = rng.integers(0, 2, size=300).astype(np.bool_)
    blind = bits.copy()
    blind[:, LADDER_HERALD_COLS] = False
    assert (w.soft_outputs(bits[:, :18])[:, 1] > w.soft_outputs(blind[:, :18])[:, 1]).any()
    only_heralds = ~bits[:, g.node_det].any(axis=1) & bits[:, LADDER_HERALD_COLS].any(axis=1)
    assert only_heralds.sum() >= 4
    for metric, row_bytes, offset in (("full_edges", 3, 1), ("largest_cluster", 8, 0)):
        soft = w.with_soft_output(metric, 16)
        want = soft_statement(soft, bits)
        assert not want[2][only_heralds].any()
        same(soft_on_device(hp, soft, bits, row_bytes, rng, offset=offset), want, f"herald ladder, weighted = {weighted}, {metric}")


@pytest.mark.parametrize("metric,weights", [("full_edges", None), ("rounds", "probability")])
def test_heralded_d3_rows(hp, metric, weights):
    """The d = 3 erasure memory of 12 rounds: 5 windows, about 208 heralds to a window; rows with heralds and no defect on a node
    column are not decoded, have four zeros and land in bin 0."""
    _, bits, w = heralded_d3(weights)
    soft = w.with_soft_output(metric, 32)
    want = soft_statement(soft, bits)
    assert want[1][0] == 336 and not want[2][320:].any() and want[3][0][0] >= 16 and (want[3][0] > 0).sum() >= 3
    same(soft_on_device(hp, soft, bits, 85, np.random.default_rng(2), offset=3), want, f"heralded d = 3, {metric}, weights = {weights}")


def test_a_miss_on_the_device(hp):
    """A miss in the last window: rounds, full_edges and largest_cluster include it and the windows decoded before it; no weight."""
    g, w = miss_ladder()
    rng = np.random.default_rng(4)
    dets = np.concatenate([miss_rows(g), fire(g, rng, 61, 0.08)])
    dets[3:, 12:] = rng.random((61, 2)) < 0.3
    bits = with_observables(dets, rng)
    soft = w.with_soft_output("full_edges", 8)
    want = soft_statement(soft, bits)
    assert want[2][:3].tolist() == MISS_ROWS_BY_HAND and 3 < want[1][2] < 64
    same(soft_on_device(hp, soft, bits, 2, rng), want, "miss")


@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_equals_the_whole_graph_handle(hp, weights):
    _, bits = d3_rows()
    uf = UnionFindDecoder.from_circuit(d3_rows()[0], weights=weights).with_soft_output("largest_cluster", 16)
    w = d3_windowed(weights, 96).with_soft_output("largest_cluster", 16)
    assert w.info()["n_windows"] == 1
    rows = packed(bits, 16, np.random.default_rng(8))
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        whole = uf.decode_device(hp, d_rows.ptr, len(rows), 16, soft=True)
        windowed = w.decode_device(hp, d_rows.ptr, len(rows), 16, soft=True)
    finally:
        d_rows.free()
    same(windowed, whole, f"one window, weights = {weights}")
    assert whole[2].any() and np.array_equal(whole[2], uf.soft_outputs(bits[:, :96]))


def raw_call(hp, w, bits, row_bytes, calls, start_cnt, start_hist, n_values):
    """``calls`` (each ``(n, metric, n_bins, with d_hist, with d_soft)``) on one handle, one ``d_counters``, one ``d_hist`` and one
    ``d_soft``: ``(errors raised, counters, histogram words, values, launches)``."""
    n, n_cols = bits.shape
    nd = w.num_detectors
    rows = packed(bits, row_bytes, np.random.default_rng(6))
    h = hp.ufw_create(w.graph, n_cols, w.commit, w.window, w.edge_caps, heralds=w.heralds)
    bufs = [hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(8 * len(start_hist) + 16), hp.malloc(16 * n_values + 16)]
    d_rows, d_cnt, d_hist, d_values = bufs
    raised = []
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, start_cnt)
        hp.h2d(d_hist, start_hist)
        hp.h2d(d_values, np.full((n_values, 4), 0xFFFFFFFF, np.uint32))
        for n_rows, metric, n_bins, hist, values in calls:
            try:
                hp.ufw_decode_soft_device(h, d_rows.ptr, n_rows, row_bytes, (nd, n_cols), d_cnt.ptr, metric, n_bins, d_hist.ptr if hist else 0,
                                          d_soft=d_values.ptr if values else 0)
                raised.append(None)
            except ValueError as e:
                raised.append(str(e))
        launches = hp.ufw_info(h)["launches"]   # (waits for the decodes)
        cnt, hist, values = np.zeros(3, np.uint64), np.zeros(len(start_hist), np.uint64), np.zeros((n_values, 4), np.uint32)
        hp.d2h(cnt, d_cnt)
        hp.d2h(hist, d_hist)
        hp.d2h(values, d_values)
    finally:
        hp.ufw_destroy(h)
        for b in bufs:
            b.free()
    return raised, cnt, hist, values, launches


def test_two_calls_accumulate_and_no_rows_are_a_no_op(hp):
    _, bits = d3_rows()
    w = d3_windowed(None)
    want = soft_statement(w.with_soft_output("full_edges", 8), bits)
    start_cnt, start_hist = np.array([5, 6, 7], np.uint64), np.arange(100, 116, dtype=np.uint64)
    calls = [(256, "full_edges", 8, True, True), (256, 1, 8, True, False), (0, "full_edges", 8, True, True)]
    raised, cnt, hist, values, launches = raw_call(hp, w, bits, 13, calls, start_cnt, start_hist, 256)
    assert raised == [None, None, None] and launches == 2
    assert cnt.tolist() == [5 + 2 * want[1][0], 6 + 2 * want[1][1], 7 + 2 * want[1][2]]
    assert hist.tolist() == (start_hist.astype(np.int64) + 2 * np.concatenate(want[3])).tolist()
    assert np.array_equal(values, want[2])


def test_refusals(hp):
    """A bad metric, a bad number of bins and a NULL histogram are ``TSIM_EINVAL`` on the host: nothing is launched or written."""
    _, bits = d3_rows()
    w = d3_windowed(None)
    zeros = np.zeros(2048, np.uint64)
    calls = [(64, 4, 8, True, True), (64, -1, 8, True, True), (64, 2, 1, True, True), (64, 2, 1025, True, True), (64, 2, 8, False, True),
             (0, 4, 8, True, True), (0, 2, 8, False, True)]
    raised, cnt, hist, values, launches = raw_call(hp, w, bits[:64], 13, calls, np.zeros(3, np.uint64), zeros, 64)
    assert all(r is not None for r in raised) and launches == 0
    assert "metric = 4" in raised[0] and "n_bins = 1 " in raised[2] and "n_bins = 1025" in raised[3] and "d_hist is NULL" in raised[4]
    assert not cnt.any() and not hist.any() and (values == 0xFFFFFFFF).all()
    raised, _, _, _, launches = raw_call(hp, w, bits[:64], 13, [(64, "confidence", 8, True, True)], np.zeros(3, np.uint64), zeros, 64)
    assert raised[0] is not None and launches == 0   # (an unknown name never reaches the library)
    with pytest.raises(ValueError, match="the decoder has no soft output"):
        soft_on_device(hp, w, bits[:64], 13, np.random.default_rng(0))


def test_count_equals_the_host_tally_of_the_same_sample(hip):
    c, _ = d3_rows()
    w = d3_windowed(None)
    soft = w.with_soft_output("largest_cluster", 16)
    nd = w.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[0, 70]] = True
    rows = c.compile_detector_sampler(seed=21, method="faults").sample(4096, append_observables=True)
    got = c.compile_detector_sampler(seed=21, method="faults").count(4096, decoder=soft, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=soft, histogram_columns=(nd,))
    print(f"kept per bin {got.soft_kept.tolist()}, wrong per bin {got.soft_errors.tolist()}; host {want.soft_kept.tolist()}, "
          f"{want.soft_errors.tolist()}")
    assert got == want
    assert got.soft_output == "largest_cluster" and np.array_equal(got.soft_kept, want.soft_kept) and np.array_equal(got.soft_errors, want.soft_errors)
    assert int(got.soft_kept.sum()) == got.kept < 4096 and int(got.soft_errors.sum()) == got.decoded_errors > 0 and (got.soft_kept > 0).sum() >= 4
    accepted, errors = got.rejection_curve()
    assert (accepted[-1], errors[-1]) == (got.kept, got.decoded_errors)
    # the same count() without the soft output is what it is today
    plain = c.compile_detector_sampler(seed=21, method="faults").count(4096, decoder=w, postselection_mask=mask)
    assert plain == tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=w, histogram_columns=(nd,))
    assert plain.soft_output is None and plain.soft_kept is None and plain.soft_errors is None and plain != got
    fields = [f for f in ShotCounts.__dataclass_fields__ if not f.startswith("soft_")]
    assert ShotCounts(*(getattr(got, f) for f in fields)) == plain
