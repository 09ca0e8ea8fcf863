"""Soft outputs of the union-find decoder on the GPU (``tsim_uf_decode_soft_device``, ``k_uf<Weighted, Heralds, true>`` of
``csrc/tsim_uf.hip.h``): every prediction, the three counters, the four values of every row and both histograms bit for bit
against the numpy statement (``UnionFindDecoder.soft_outputs``), on every kind of handle, with masks, accumulating, beside
``tsim_uf_decode_device``, through ``count()``, and what the entry refuses."""

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_unionfind import chain_graph, memory, no_boundary_graph
from test_unionfind_erasure import erasure_memory

from tsim_amd import faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import ShotCounts, tally_rows
from tsim_amd.decode import UnionFindDecoder

pytestmark = pytest.mark.gpu

METRICS = ("rounds", "full_edges", "largest_cluster", "correction_weight")


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def soft_statement(uf, bits, xor=None, test=None):
    """``(predictions, (kept, wrong, missed), values uint32[n, 4], (kept per bin, wrong per bin))`` of bool rows (detectors, then
    observables) by the numpy statement, for the metric and the bins ``uf`` carries; a row that is not kept has no values."""
    nd, n_obs = uf.num_detectors, uf.num_observables
    pred, cnt = host_statement(uf, bits, xor, test)
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    values = np.where(keep[:, None], uf.soft_outputs(b[:, :nd]), 0)
    obs = (b[:, nd:nd + n_obs].astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    which = np.minimum(values[:, METRICS.index(uf.soft_output)], uf.soft_bins - 1)
    hist = (np.bincount(which[keep], minlength=uf.soft_bins), np.bincount(which[keep & (pred != obs)], minlength=uf.soft_bins))
    assert hist[0].sum() == cnt[0] and hist[1].sum() == cnt[1]
    return pred, cnt, values.astype(np.uint32), hist


def soft_on_device(hp, uf, bits, row_bytes, rng, xor=None, test=None, offset=0):
    """The same from ``tsim_uf_decode_soft_device`` (``decode_device(soft=True)``) over the bit-packed rows, ``offset`` bytes into
    their buffer."""
    n, n_cols = bits.shape
    rows = packed(bits, row_bytes, rng)
    bufs = [hp.malloc(rows.nbytes + 64)]
    try:
        hp.h2d(bufs[0].ptr + offset, rows)
        masks = {}
        for name, m in (("d_xor", xor), ("d_test", test)):
            if m is not None:
                bufs.append(hp.malloc(64 + (n_cols + 7) // 8))
                hp.h2d(bufs[-1], np.packbits(m, bitorder="little"))
                masks[name] = bufs[-1].ptr
        return uf.decode_device(hp, bufs[0].ptr + offset, n, row_bytes, n_cols=n_cols, soft=True, **masks)
    finally:
        for b in bufs:
            b.free()


def same(got, want, note=""):
    """Predictions, counters, values and histograms, all of them, bit for bit."""
    pred, cnt, values, hist = got
    print(f"{note}: host {want[1]}, device {cnt}; rows whose prediction differs {int((pred != want[0]).sum())}, whose values differ "
          f"{int((values != want[2]).any(axis=1).sum())}; kept per bin {hist[0].tolist()}, wrong per bin {hist[1].tolist()}")
    assert np.array_equal(pred, want[0]) and cnt == want[1]
    assert values.dtype == np.uint32 and values.shape == want[2].shape and np.array_equal(values, want[2])
    assert np.array_equal(hist[0], want[3][0]) and np.array_equal(hist[1], want[3][1])


_ROWS: dict = {}


def surface(d, rounds, p, n, weighted=False):
    """``(decoder, rows)`` of a memory circuit, the rows and each decoder (with its cache of decoded syndromes) built once."""
    if (d, "rows") not in _ROWS:
        c = memory(d, p, rounds)
        _ROWS[d, "rows"] = (c, faults.fault_rows_host(c.compile_faults(), 0, n, (1, 2)).view(np.bool_))
    c, bits = _ROWS[d, "rows"]
    if (d, weighted) not in _ROWS:
        _ROWS[d, weighted] = UnionFindDecoder.from_circuit(c, weights="probability" if weighted else None)
    return _ROWS[d, weighted], bits


@pytest.mark.parametrize("metric,weighted", [(m, False) for m in METRICS] + [("largest_cluster", True)])
def test_d3_rows_bit_for_bit(hp, metric, weighted):
    """4133 rows of 5 bytes, 3 bytes into their buffer: the byte path, a last tile of 37 rows, several tiles per wave."""
    uf, bits = surface(3, 3, 0.02, 4133, weighted)
    soft = uf.with_soft_output(metric, 64)
    want = soft_statement(soft, bits)
    assert want[1][0] == 4133 and want[1][1] == (498 if weighted else 557)
    assert want[2].max(axis=0).tolist() == ([7, 28, 19, 11] if weighted else [2, 60, 25, 14])
    assert want[3][0][0] > 0 and (want[3][0] > 0).sum() >= 3 and want[3][1][1:].sum() > 0
    same(soft_on_device(hp, soft, bits, 5, np.random.default_rng(3), offset=3), want, f"d = 3, {metric}")


@pytest.mark.parametrize("metric,bins,weighted", [("full_edges", 16, False), ("largest_cluster", 16, False), ("correction_weight", 16, False),
                                                  ("rounds", 2, False), ("largest_cluster", 2, True), ("rounds", 16, True)])
def test_d5_rows_clamped_bins(hp, metric, bins, weighted):
    """2048 aligned 16-byte rows (the 8-byte loads), 121 nodes: 16 bins clamp full_edges, largest_cluster and correction_weight,
    none of them away entirely; 2 bins are "no defect" against the rest."""
    uf, bits = surface(5, 5, 0.01, 2048, weighted)
    soft = uf.with_soft_output(metric, bins)
    want = soft_statement(soft, bits)
    assert want[1][1] == (116 if weighted else 151)
    assert want[2].max(axis=0).tolist() == ([12, 100, 53, 23] if weighted else [4, 235, 95, 24])
    top = int(want[2][:, METRICS.index(metric)].max())
    assert want[3][0][min(top, bins - 1)] > 0 and (want[3][0] > 0).sum() >= min(bins, 4)
    if (metric, bins) != ("rounds", 16):
        assert top >= bins   # the clamp is exercised
    same(soft_on_device(hp, soft, bits, 16, np.random.default_rng(5)), want, f"d = 5, {metric} in {bins} bins")


@pytest.mark.parametrize("name,metric", [("no_boundary", "rounds"), ("no_boundary", "largest_cluster"), ("no_boundary", "correction_weight"),
                                         ("chain", "rounds"), ("chain", "full_edges"), ("chain", "largest_cluster")])
def test_hand_made_graphs_bit_for_bit(hp, name, metric):
    rng = np.random.default_rng(11)
    if name == "no_boundary":   # the miss path: a miss keeps rounds, full_edges and largest_cluster and has weight 0
        uf = UnionFindDecoder(no_boundary_graph())
        bits = rng.integers(0, 2, size=(200, 5)).astype(np.bool_)
    else:   # node indices beyond 64, more rounds than bins
        uf = UnionFindDecoder(chain_graph())
        bits = np.zeros((120, 70), np.bool_)
        for r in range(3, 120):
            bits[r, rng.choice(69, size=int(rng.integers(0, 5)), replace=False)] = True
        bits[0, [29, 49]] = bits[1, [44, 64]] = bits[2, [4, 67]] = True
        bits[:, 69] = rng.integers(0, 2, size=120).astype(np.bool_)
    soft = uf.with_soft_output(metric)
    want = soft_statement(soft, bits)
    if name == "no_boundary":
        missed = uf.missed(bits[:, :3])
        assert want[1][2] == 103 and want[2][missed, 1:3].min() >= 1 and not want[2][missed, 3].any()
    else:
        assert want[2][:, 0].max() > 64 and want[2][:, 2].max() > 40
        assert metric != "rounds" or want[3][0][63] > 0
    same(soft_on_device(hp, soft, bits, (bits.shape[1] + 7) // 8 + 1, rng), want, f"{name}, {metric}")


@pytest.mark.parametrize("metric,weighted", [("largest_cluster", False), ("full_edges", True), ("rounds", False)])
def test_heralded_rows_bit_for_bit(hp, metric, weighted):
    """The d = 3 erasure circuit through ``tsim_uf_create_heralds``: pre-grown edges count as full edges; a row with heralds and no
    defect is not decoded, has four zeros and lands in bin 0."""
    if "heralds" not in _ROWS:
        c = erasure_memory(3, 3, pe=0.05)
        bits = faults.fault_rows_host(c.compile_faults(), 0, 512, (1, 2)).view(np.bool_).copy()
        _ROWS["heralds"] = (c, bits, {})
    c, bits, decoders = _ROWS["heralds"]
    if weighted not in decoders:
        decoders[weighted] = UnionFindDecoder.from_circuit(c, weights="probability" if weighted else None, heralds=True)
        bits[:8, decoders[weighted].graph.node_det] = False
    uf = decoders[weighted]
    g = uf.graph
    assert (g.n_nodes, g.n_heralds) == (25, 144) and bits[:8, g.herald_det].any(axis=1).all() and not bits[:8, g.node_det].any()
    soft = uf.with_soft_output(metric, 32)
    want = soft_statement(soft, bits)
    assert not want[2][:8].any() and want[1][1] > 0
    decoded = bits[:, g.node_det].any(axis=1)
    assert (want[2][decoded, 0] == 0).any()   # growth that the pre-grown edges end before its first round
    same(soft_on_device(hp, soft, bits, 22, np.random.default_rng(8), offset=3), want, f"heralds, {metric}")


def test_masks_and_accumulation(hp):
    """``d_xor`` and ``d_test``: a row that is not kept lands in no bin and has zeros in ``d_soft``; two calls into the same
    ``d_hist`` and ``d_counters`` add up on what was there, and both launches count."""
    uf, bits = surface(3, 3, 0.02, 4133)
    bits = bits[:1500]
    soft = uf.with_soft_output("largest_cluster", 8)
    rng = np.random.default_rng(5)
    n_cols, nd = bits.shape[1], uf.num_detectors
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, np.bool_)
    test[[1, 7, 16]] = True
    want = soft_statement(soft, bits, xor, test)
    keep = ~((bits ^ xor) & test).any(axis=1)
    assert 0 < want[1][0] == keep.sum() < len(bits) and not want[2][~keep].any() and want[2][keep].any()
    same(soft_on_device(hp, soft, bits, 8, rng, xor=xor, test=test), want, "masks")

    rows = packed(bits, 8, rng)
    start_cnt, start_hist = np.array([5, 6, 7], np.uint64), np.arange(100, 116, dtype=np.uint64)
    h = hp.uf_create(uf.graph, n_cols)
    bufs = [hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(16 * 8), hp.malloc(64), hp.malloc(64)]
    d_rows, d_cnt, d_hist, d_xor, d_test = bufs
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, start_cnt)
        hp.h2d(d_hist, start_hist)
        hp.h2d(d_xor, np.packbits(xor, bitorder="little"))
        hp.h2d(d_test, np.packbits(test, bitorder="little"))
        for _ in range(2):
            hp.uf_decode_soft_device(h, d_rows.ptr, len(rows), 8, (nd, n_cols), d_cnt.ptr, "largest_cluster", 8, d_hist.ptr,
                                     d_xor=d_xor.ptr, d_test=d_test.ptr)
        hp.uf_decode_soft_device(h, d_rows.ptr, 0, 8, (nd, n_cols), d_cnt.ptr, 2, 8, d_hist.ptr)   # no rows: no launch
        info = hp.uf_info(h)   # (waits for the decodes)
        cnt, hist = np.zeros(3, np.uint64), np.zeros(16, np.uint64)
        hp.d2h(cnt, d_cnt)
        hp.d2h(hist, d_hist)
    finally:
        hp.uf_destroy(h)
        for b in bufs:
            b.free()
    assert cnt.tolist() == [5 + 2 * want[1][0], 6 + 2 * want[1][1], 7 + 2 * want[1][2]]
    assert hist.tolist() == (start_hist.astype(np.int64) + 2 * np.concatenate(want[3])).tolist()
    assert info["launches"] == 2 and info["rows_decoded"] == 2 * int((keep & (bits ^ xor)[:, :nd].any(axis=1)).sum())
    assert info["max_rounds"] == int(want[2][:, 0].max())


@pytest.mark.parametrize("weighted", [False, True])
def test_both_entry_points_on_one_handle(hp, weighted):
    """The same rows through ``tsim_uf_decode_device`` and ``tsim_uf_decode_soft_device``: the predictions and the counters agree,
    and a handle's state in LDS is what it was (``tsim_uf_info``)."""
    uf, bits = surface(3, 3, 0.02, 4133, weighted)
    n, n_cols, nd = len(bits), bits.shape[1], uf.num_detectors
    rows = packed(bits, 4, np.random.default_rng(6))
    want_pred, want_cnt = host_statement(uf, bits)
    h = hp.uf_create(uf.graph, n_cols, uf.edge_caps)
    bufs = [hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(64), hp.malloc(8 * n), hp.malloc(8 * n), hp.malloc(2 * 64 * 8)]
    d_rows, d_plain, d_soft, d_pred_plain, d_pred_soft, d_hist = bufs
    try:
        before = hp.uf_info(h)
        hp.h2d(d_rows, rows)
        for b in (d_plain, d_soft):
            hp.h2d(b, np.zeros(3, np.uint64))
        hp.h2d(d_hist, np.zeros(128, np.uint64))
        hp.uf_decode_device(h, d_rows.ptr, n, 4, (nd, n_cols), d_plain.ptr, d_pred=d_pred_plain.ptr)
        hp.uf_decode_soft_device(h, d_rows.ptr, n, 4, (nd, n_cols), d_soft.ptr, "correction_weight", 64, d_hist.ptr, d_pred=d_pred_soft.ptr)
        after = hp.uf_info(h)
        got = [np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(128, np.uint64)]
        for a, b in zip(got, (d_plain, d_soft, d_pred_plain, d_pred_soft, d_hist)):
            hp.d2h(a, b)
    finally:
        hp.uf_destroy(h)
        for b in bufs:
            b.free()
    assert got[0].tolist() == got[1].tolist() == list(want_cnt)
    assert np.array_equal(got[2], want_pred) and np.array_equal(got[3], want_pred)
    assert int(got[4][:64].sum()) == want_cnt[0] and int(got[4][64:].sum()) == want_cnt[1]
    assert after["launches"] == 2 and {k: v for k, v in after.items() if k not in ("launches", "max_rounds", "rows_decoded")} == \
        {k: v for k, v in before.items() if k not in ("launches", "max_rounds", "rows_decoded")}


def test_count_equals_the_host_tally_of_the_same_sample(hip):
    c = memory(3, 0.01, 3)
    uf = UnionFindDecoder.from_circuit(c)
    soft = uf.with_soft_output("largest_cluster", 16)
    nd = uf.num_detectors
    rows = c.compile_detector_sampler(seed=5, method="faults").sample(20000, append_observables=True)
    got = c.compile_detector_sampler(seed=5, method="faults").count(20000, decoder=soft)
    want = tally_rows(rows, num_detectors=nd, decoder=soft, histogram_columns=(nd,))
    plain = c.compile_detector_sampler(seed=5, method="faults").count(20000, decoder=uf)
    print(f"kept per bin {got.soft_kept.tolist()}, wrong per bin {got.soft_errors.tolist()}; host {want.soft_kept.tolist()}, "
          f"{want.soft_errors.tolist()}")
    assert got == want
    assert got.soft_output == "largest_cluster" and np.array_equal(got.soft_kept, want.soft_kept) and np.array_equal(got.soft_errors, want.soft_errors)
    assert int(got.soft_kept.sum()) == got.kept == 20000 and int(got.soft_errors.sum()) == got.decoded_errors > 0
    assert (got.soft_kept > 0).sum() >= 4
    assert plain.soft_output is None and plain.soft_kept is None and plain.soft_errors is None and plain != got
    fields = [f for f in ShotCounts.__dataclass_fields__ if not f.startswith("soft_")]
    assert ShotCounts(*(getattr(got, f) for f in fields)) == plain
    accepted, errors = got.rejection_curve()
    assert (accepted[-1], errors[-1]) == (got.kept, got.decoded_errors)
    # with a postselection mask the rows that are not kept land in no bin
    mask = np.zeros(nd, np.bool_)
    mask[[0, 13]] = True
    masked = c.compile_detector_sampler(seed=5, method="faults").count(20000, decoder=soft, postselection_mask=mask)
    assert masked == tally_rows(rows, num_detectors=nd, decoder=soft, postselection_mask=mask, histogram_columns=(nd,))
    assert int(masked.soft_kept.sum()) == masked.kept < 20000


def test_refusals(hp):
    """A bad metric, a bad number of bins and a missing histogram are refused on the host: nothing is launched or written."""
    uf, bits = surface(3, 3, 0.02, 4133)
    bits = bits[:128]
    n, n_cols, nd = len(bits), bits.shape[1], uf.num_detectors
    rows = packed(bits, 4, np.random.default_rng(7))
    h = hp.uf_create(uf.graph, n_cols)
    bufs = [hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(2 * 1024 * 8), hp.malloc(16 * n + 16)]
    d_rows, d_cnt, d_hist, d_values = bufs
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, np.zeros(3, np.uint64))
        hp.h2d(d_hist, np.zeros(2048, np.uint64))
        for bad in (dict(metric=-1), dict(metric=4), dict(n_bins=1), dict(n_bins=1025), dict(n_bins=0), dict(d_hist=0),
                    dict(d_hist=d_hist.ptr + 4), dict(d_soft=d_values.ptr + 8)):
            kw = dict(metric=2, n_bins=64, d_hist=d_hist.ptr, d_soft=0)
            kw.update(bad)
            with pytest.raises(ValueError):
                hp.uf_decode_soft_device(h, d_rows.ptr, n, 4, (nd, n_cols), d_cnt.ptr, kw["metric"], kw["n_bins"], kw["d_hist"],
                                         d_soft=kw["d_soft"])
            with pytest.raises(ValueError):   # refused without rows too
                hp.uf_decode_soft_device(h, d_rows.ptr, 0, 4, (nd, n_cols), d_cnt.ptr, kw["metric"], kw["n_bins"], kw["d_hist"],
                                         d_soft=kw["d_soft"])
        with pytest.raises(ValueError):
            hp.uf_decode_soft_device(h, d_rows.ptr, n, 4, (nd, n_cols), d_cnt.ptr, "confidence", 64, d_hist.ptr)
        assert hp.uf_info(h)["launches"] == 0
        cnt, hist = np.ones(3, np.uint64), np.ones(2048, np.uint64)
        hp.d2h(cnt, d_cnt)
        hp.d2h(hist, d_hist)
        assert not cnt.any() and not hist.any()
        with pytest.raises(ValueError, match="soft output"):
            uf.decode_device(hp, d_rows.ptr, n, 4, n_cols=n_cols, soft=True)
        # the largest number of bins and the per-row values, on the handle the refusals left
        hp.uf_decode_soft_device(h, d_rows.ptr, n, 4, (nd, n_cols), d_cnt.ptr, 1, 1024, d_hist.ptr, d_soft=d_values.ptr)
        values = np.zeros((n, 4), np.uint32)
        assert hp.uf_info(h)["launches"] == 1
        hp.d2h(values, d_values)
        hp.d2h(hist, d_hist)
    finally:
        hp.uf_destroy(h)
        for b in bufs:
            b.free()
    want = uf.soft_outputs(bits[:, :nd])
    assert np.array_equal(values, want)
    assert np.array_equal(hist[:1024].astype(np.int64), np.bincount(want[:, 1], minlength=1024)) and int(hist[1024:].sum()) > 0
