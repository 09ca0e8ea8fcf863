"""The complementary gap on the GPU (``tsim_uf_create_matching_gap``, ``tsim_uf_decode_gap_device``: ``k_gap_table`` of
``csrc/tsim_uf_match.hip.h`` and ``k_uf<., false, false, true, true>`` of ``csrc/tsim_uf.hip.h``): the class table, the
predictions, the counters, the deficits and both histograms bit for bit against the numpy statement, ``count(decoder=...)``
against ``tally_rows``, and what the new calls refuse.  Every graph and row is valid: nothing here asks a kernel for an index
its tables do not hold."""

import ctypes as C

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_unionfind import chain_graph
from test_unionfind_matching import issue_memory, matching_decoder, table_cases

from tsim_amd import _lib, faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import UnionFindDecoder, uf_match_shot_bytes

pytestmark = pytest.mark.gpu

_CASES: dict = {}


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def surface(d: int, rounds: int, p: float, n: int, K: int):
    """``(matching decoder, gap decoder, n rows)`` of a weighted memory experiment (``fault_rows_host`` under key (1, 2)), built once."""
    if (d, rounds, p, n, K) not in _CASES:
        c = issue_memory(d, rounds, p)
        um = UnionFindDecoder.from_circuit(c, weights="probability").with_cluster_matching(K)
        rows = faults.fault_rows_host(c.compile_faults(), 0, n, (1, 2)).view(np.bool_)
        _CASES[d, rounds, p, n, K] = (um, um.with_gap_output(), rows)
    return _CASES[d, rounds, p, n, K]


def statement(ug, bits, xor=None, test=None):
    """``(predictions, (kept, wrong, missed), deficits, kept per bin, errors per bin)`` of bool rows by the numpy statement."""
    nd, n_obs = ug.num_detectors, ug.num_observables
    pred, counts = host_statement(ug, bits, xor, test)
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    D = np.where(keep, ug.gap_outputs(b[:, :nd]), 0)
    obs = (b[:, nd:nd + n_obs].astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    bins = np.minimum(D // ug.gap_step, ug.soft_bins - 1)
    return (pred, counts, D, np.bincount(bins[keep], minlength=ug.soft_bins),
            np.bincount(bins[keep & (pred != obs)], minlength=ug.soft_bins))


def on_device(hp, ug, bits, row_bytes, rng, xor=None, test=None, offset=0):
    """The same from one ``tsim_uf_decode_gap_device`` over the bit-packed rows, ``offset`` bytes into their buffer, and
    ``tsim_uf_info`` after it."""
    n, n_cols = bits.shape
    nd, B = ug.num_detectors, ug.soft_bins
    rows = packed(bits, row_bytes, rng)
    pred, cnt, D, hist = np.zeros(n, np.uint64), np.zeros(3, np.uint64), np.zeros(n, np.uint32), np.zeros(2 * B, np.uint64)
    bufs = [hp.malloc(rows.nbytes + 64), hp.malloc(pred.nbytes + 16), hp.malloc(64), hp.malloc(D.nbytes + 16), hp.malloc(hist.nbytes + 16)]
    h, _, destroy = ug._handle(hp, n_cols)
    try:
        hp.h2d(bufs[0].ptr + offset, rows)
        hp.h2d(bufs[2], cnt)
        hp.h2d(bufs[4], hist)
        masks = {}
        for name, m in (("d_xor", xor), ("d_test", test)):
            if m is not None:
                bufs.append(hp.malloc(64 + (n_cols + 7) // 8))
                hp.h2d(bufs[-1], np.packbits(m, bitorder="little"))
                masks[name] = bufs[-1].ptr
        hp.uf_decode_gap_device(h, bufs[0].ptr + offset, n, row_bytes, (nd, nd + ug.num_observables), bufs[2].ptr, ug.gap_cap, ug.gap_step, B,
                                bufs[4].ptr, d_gap=bufs[3].ptr, d_pred=bufs[1].ptr, **masks)
        info = hp.uf_info(h)  # (synchronises)
        for a, b in ((pred, bufs[1]), (cnt, bufs[2]), (D, bufs[3]), (hist, bufs[4])):
            hp.d2h(a, b)
        return pred, tuple(int(x) for x in cnt), D.astype(np.int64), hist[:B].astype(np.int64), hist[B:].astype(np.int64), info
    finally:
        destroy(h)
        for b in bufs:
            b.free()


def check(hp, ug, bits, row_bytes, rng, xor=None, test=None, offset=0):
    want = statement(ug, bits, xor, test)
    got = on_device(hp, ug, bits, row_bytes, rng, xor, test, offset)
    print(f"K = {ug.match_defects}, G = {ug.gap_cap}, step {ug.gap_step}: host {want[1]}, device {got[1]}; rows whose prediction differs "
          f"{int((got[0] != want[0]).sum())}, whose deficit differs {int((got[2] != want[2]).sum())}; rows with 0 < D < G "
          f"{int(((want[2] > 0) & (want[2] < ug.gap_cap)).sum())}, with D = G {int((want[2] == ug.gap_cap).sum())}")
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert got[3].sum() == want[1][0] and got[4].sum() == want[1][1]
    g, info = ug.graph, got[5]
    assert info["lds_bytes_per_shot"] == uf_match_shot_bytes(g.n_nodes, g.n_edges, ug.edge_caps is not None, ug.match_defects, gap=True)
    assert 16 + info["shots_per_block"] * info["lds_bytes_per_shot"] <= 64 * 1024 and info["max_defects"] == ug.match_defects
    return want


# ---- the class table ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_boundary", "island70", "random130", "surface", "chain"])
def test_gap_table_bit_for_bit(hp, name):
    if name == "surface":
        um = surface(3, 3, 3e-3, 4096, 10)[0]
        assert um.graph.n_nodes == 25
    elif name == "chain":
        um = matching_decoder(chain_graph(20, 5), np.arange(1, 20))
    else:
        um = matching_decoder(*table_cases()[name])
    for k in range(um.num_observables):
        ug = um.with_gap_output(k, cap=5)
        want, want_w0 = ug.gap_table()
        h = hp.uf_create_matching_gap(um.graph, um.graph.n_nodes, um.match_weights, 10, k, um.edge_caps)
        try:
            dist2, w0 = hp.uf_gap_table(h)
            dist, _ = hp.uf_match_table(h)
            info = hp.uf_info(h)
        finally:
            hp.uf_destroy(h)
        assert np.array_equal(dist2, want) and w0 == want_w0
        assert (w0 is None) == (name == "chain")  # tsim_uf_gap_table's -1
        assert np.array_equal(dist, um.match_table()[0])
        assert info["device_bytes"] >= 20 * um.graph.n_nodes ** 2 and info["max_defects"] == 10 and info["launches"] == 0


# ---- decoded rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(3, 3, 3e-3, 4096, 10), (5, 5, 5e-3, 2048, 4)])
def test_decode_device_bit_for_bit(hp, case):
    """d = 5 at K = 4: matched and peeled clusters in one row."""
    um, ug, bits = surface(*case)
    nd = ug.num_detectors
    want = statement(ug, bits)
    rows = packed(bits, 16, np.random.default_rng(1))
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        pred, cnt, D, (kept, errors) = ug.decode_device(hp, d_rows.ptr, len(rows), 16, soft=True)
        plain = um.decode_device(hp, d_rows.ptr, len(rows), 16)
        as_matching = ug.decode_device(hp, d_rows.ptr, len(rows), 16)  # tsim_uf_decode_device on the gap handle
    finally:
        d_rows.free()
    matched, peeled = ug.match_counts(bits[:, :nd])
    print(f"{case}: counters {cnt} (statement {want[1]}), clusters matched {matched}, peeled {peeled}; D = 0: {int((want[2] == 0).sum())}, "
          f"0 < D < G: {int(((want[2] > 0) & (want[2] < ug.gap_cap)).sum())}, D = G: {int((want[2] == ug.gap_cap).sum())}")
    assert pred.dtype == np.uint64 and D.dtype == np.uint32 and D.shape == (len(rows),)
    assert np.array_equal(pred, want[0]) and cnt == want[1]
    assert np.array_equal(D, want[2])
    assert np.array_equal(kept, want[3]) and np.array_equal(errors, want[4])
    assert np.array_equal(plain[0], pred) and plain[1] == cnt
    assert np.array_equal(as_matching[0], pred) and as_matching[1] == cnt
    assert want[1][1] > 0 and ((want[2] > 0) & (want[2] < ug.gap_cap)).sum() > 20
    if case[4] == 4:
        dets = bits[:, :nd]
        assert peeled > 0 and any(all(ug.match_counts(dets[r:r + 1])) for r in np.flatnonzero(want[2] == ug.gap_cap)[:200])


@pytest.mark.parametrize("n", [1, 63, 65, 4096])
def test_row_counts_masks_and_stride(hp, n):
    """Rows of 5 bytes (no multiple of 8) at an odd offset into their buffer, an xor row and a test row; K = 2 at p = 2e-2 mixes
    matched and peeled clusters."""
    um, _, some = surface(3, 3, 2e-2, 512, 2)
    ug = um.with_gap_output(bins=16)
    bits = np.tile(some, (8, 1))[:n] if n > 1 else some[7:8]
    rng = np.random.default_rng(n)
    n_cols = bits.shape[1]
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, np.bool_)
    test[[1, 16]] = True
    want = check(hp, ug, bits, 5, rng, xor=xor, test=test, offset=3)
    if n >= 63:
        assert 0 < want[1][0] < n and (want[2] == ug.gap_cap).any() and ((want[2] > 0) & (want[2] < ug.gap_cap)).any()
    check(hp, ug, bits, 8, rng, offset=8)  # (the 8-byte loads; no masks)


def test_two_calls_accumulate(hp):
    um, ug, bits = surface(3, 3, 3e-3, 4096, 10)
    bits = bits[:1000]
    nd, B = ug.num_detectors, ug.soft_bins
    want = statement(ug, bits)
    rows = packed(bits, 4, np.random.default_rng(6))
    h, _, destroy = ug._handle(hp, nd + 1)
    d_rows, d_cnt, d_hist = hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(16 * B)
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, np.array([5, 0, 0], np.uint64))
        start = np.arange(2 * B, dtype=np.uint64)
        hp.h2d(d_hist, start)
        for _ in range(2):
            hp.uf_decode_gap_device(h, d_rows.ptr, len(rows), 4, (nd, nd + 1), d_cnt.ptr, ug.gap_cap, ug.gap_step, B, d_hist.ptr)  # (no d_gap, no d_pred)
        hp.uf_decode_gap_device(h, d_rows.ptr, 0, 4, (nd, nd + 1), d_cnt.ptr, ug.gap_cap, ug.gap_step, B, d_hist.ptr)  # n == 0: no launch
        info = hp.uf_info(h)
        cnt, hist = np.zeros(3, np.uint64), np.zeros(2 * B, np.uint64)
        hp.d2h(cnt, d_cnt)
        hp.d2h(hist, d_hist)
        assert cnt.tolist() == [5 + 2 * want[1][0], 2 * want[1][1], 2 * want[1][2]]
        assert np.array_equal(hist.astype(np.int64) - start.astype(np.int64), 2 * np.concatenate([want[3], want[4]]))
        matched, peeled = ug.match_counts(bits[:, :nd])
        assert (info["launches"], info["clusters_matched"], info["clusters_peeled"]) == (2, 2 * matched, 2 * peeled)
    finally:
        destroy(h)
        for b in (d_rows, d_cnt, d_hist):
            b.free()


# ---- count() -----------------------------------------------------------------------------------------------------------------

SHOTS = 20000


@pytest.mark.parametrize("corrected", [False, True])
def test_count_equals_the_statement(hip, corrected):
    if "count" not in _CASES:
        c = issue_memory(3, 3, 3e-3)
        ug = UnionFindDecoder.from_circuit(c, weights="probability").with_cluster_matching().with_gap_output()
        rows = c.compile_detector_sampler(seed=5, method="faults").sample(SHOTS, append_observables=True)
        rows.setflags(write=False)
        _CASES["count"] = (c, ug, rows)
    c, ug, rows = _CASES["count"]
    nd = ug.num_detectors
    got = c.compile_detector_sampler(seed=5, method="faults").count(SHOTS, decoder=ug, corrected=corrected)
    want = tally_rows(rows, num_detectors=nd, decoder=ug, corrected=corrected, histogram_columns=(nd,))
    print(f"kept {got.kept}, decoded errors {got.decoded_errors}, soft_kept {got.soft_kept.tolist()}, soft_errors {got.soft_errors.tolist()}")
    assert got == want
    assert got.soft_output == "gap" and got.soft_kept.sum() == got.kept == SHOTS and got.soft_errors.sum() == got.decoded_errors > 0
    assert got.corrected == corrected and (got.soft_kept[1:] > 0).sum() > 5
    mask = np.zeros(nd, np.bool_)
    mask[[2, 11]] = True
    got = c.compile_detector_sampler(seed=5, method="faults").count(SHOTS, decoder=ug, corrected=corrected, postselection_mask=mask)
    assert got == tally_rows(rows, num_detectors=nd, decoder=ug, corrected=corrected, histogram_columns=(nd,), postselection_mask=mask)
    assert got.soft_kept.sum() == got.kept < SHOTS


# ---- what the new calls refuse -----------------------------------------------------------------------------------------------

def test_refusals(hp):
    g = chain_graph(70)
    w = np.ones(69, np.int64)
    for observable in (-1, 64):
        with pytest.raises(ValueError, match="observable"):
            hp.uf_create_matching_gap(g, 70, w, 10, observable)
    with pytest.raises(ValueError, match="max_defects"):
        hp.uf_create_matching_gap(g, 70, w, 13, 0)
    # 1500 nodes: the matching handle of K = 12 fits a block's LDS, the handle with both dynamic programs does not (TSIM_ENOTSUP)
    long = chain_graph(1500, 3)
    fits = hp.uf_create_matching(long, 1500, np.ones(1499, np.int64), 12)
    hp.uf_destroy(fits)
    with pytest.raises(_lib.HipBackendError, match="bytes of LDS"):
        hp.uf_create_matching_gap(long, 1500, np.ones(1499, np.int64), 12, 0)
    lib = _lib.load()
    h = hp.uf_create_matching_gap(g, 70, w, 10, 0)
    matching = hp.uf_create_matching(g, 70, w, 10)
    d = hp.malloc(4096)
    try:
        with pytest.raises(ValueError, match="no soft outputs"):
            hp.uf_decode_soft_device(h, d.ptr, 1, 16, (69, 70), d.ptr + 1024, "rounds", 8, d.ptr + 2048)
        with pytest.raises(ValueError, match="no class table"):
            hp.uf_decode_gap_device(matching, d.ptr, 1, 16, (69, 70), d.ptr + 1024, 100, 1, 8, d.ptr + 2048)
        for cap, step, bins, what in ((0, 1, 8, "gap_cap"), ((1 << 31) - 1, 1, 8, "gap_cap"), (100, 0, 8, "gap_step"), (100, 1, 1, "n_bins"),
                                      (100, 1, 1025, "n_bins")):
            with pytest.raises(ValueError, match=what):
                hp.uf_decode_gap_device(h, d.ptr, 1, 16, (69, 70), d.ptr + 1024, cap, step, bins, d.ptr + 2048)
        with pytest.raises(ValueError, match="d_hist"):
            hp.uf_decode_gap_device(h, d.ptr, 1, 16, (69, 70), d.ptr + 1024, 100, 1, 8, 0)
        buf, w0 = (C.c_uint32 * (2 * 70 * 70))(), C.c_int64(0)
        assert lib.tsim_uf_gap_table(C.c_void_p(matching), buf, C.byref(w0)) == -22 and b"no class table" in lib.tsim_last_error()
        assert hp.uf_info(h)["launches"] == 0 and hp.uf_info(matching)["launches"] == 0
        assert hp.uf_info(h)["lds_bytes_per_shot"] == uf_match_shot_bytes(70, 69, False, 10, gap=True)
        assert hp.uf_info(matching)["lds_bytes_per_shot"] == uf_match_shot_bytes(70, 69, False, 10)  # (the matching handle keeps its layout)
        assert hp.uf_info(matching)["shots_per_block"] >= hp.uf_info(h)["shots_per_block"]
    finally:
        hp.uf_destroy(h)
        hp.uf_destroy(matching)
        d.free()
