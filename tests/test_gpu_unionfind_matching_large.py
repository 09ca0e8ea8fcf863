"""Cluster matching, the complementary gap, heralds, soft outputs and heralded windows on the GPU at the sizes they are advertised
for: the cases of ``test_unionfind_matching_large.py``.  The table kernels at 2048 nodes (``k_match_table`` / ``k_gap_table`` of
``csrc/tsim_uf_match.hip.h``) against references that are not the statement's, ``k_uf`` with the dynamic programs on d = 9 and
d = 11 with a shot that nearly fills a block's LDS and the refusal next to it, heralds on rows of 739 bytes, 1 .. 4 waves a block,
soft outputs at 65535 full edges, grids that wrap on the matching handles, and ``k_ufw`` with heralds over 23 windows of rows of
841 bytes.  Every comparison is over all rows and bit for bit against the numpy statement of ``tsim_amd/decode.py``: predictions
with ``np.array_equal``, counters, histograms, per-row values and every number of ``tsim_uf_info`` / ``tsim_uf_erasure_info``
with ``==``.  Every graph and row is valid: nothing here asks a kernel for an index its tables do not hold."""

import time

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_gpu_unionfind_erasure import check as check_heralds
from test_gpu_unionfind_erasure_matching import cluster_counts, on_device as erasure_on_device, statement as erasure_statement
from test_gpu_unionfind_gap import on_device as gap_on_device, statement as gap_statement
from test_gpu_unionfind_matching import on_device as matching_on_device
from test_gpu_unionfind_soft import METRICS, same, soft_on_device, soft_statement
from test_gpu_unionfind_windowed_erasure import check as check_windows
from test_unionfind_large import case
from test_unionfind_matching_large import D9_WAVES, D9E_HANDLES, D9E_WAVES, d9e_quiet, dense_erased, large, tiles, wrap_base

from tsim_amd import _lib, synth
from tsim_amd.backend import HipProgram
from tsim_amd.decode import MATCH_INF, DecodingGraph, uf_erasure_shot_bytes, uf_match_shot_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def two_layouts(n_cols: int):
    """``(row_bytes, offset)``: rows and address multiples of 8 (the 8-byte loads), and an odd stride at an odd offset."""
    used = (n_cols + 7) // 8
    return [((used + 7) // 8 * 8, 0), (used | 1, 3)]


def line(what, want, got, differ, info, t0):
    print(f"{what}: host {want}, device {got}, rows that differ {differ}, {info['lds_bytes_per_shot']} bytes a shot, "
          f"{info['shots_per_block']} shots a block, {info['grid_blocks']} blocks, {time.perf_counter() - t0:.3f} s")


def handle_info(hp, dec, n_cols):
    """``tsim_uf_info`` / ``tsim_ufw_info`` of a handle of ``dec`` that decodes nothing."""
    h, _, destroy = dec._handle(hp, n_cols)
    try:
        return (hp.ufw_info if destroy == hp.ufw_destroy else hp.uf_info)(h)
    finally:
        destroy(h)


# ---- 1. tables at the node limit -----------------------------------------------------------------------------------------------

def test_chain2048_tables_bit_for_bit(hp):
    """2048 blocks of up to 2047 sweeps and 2047 mask rounds each, distances up to 2047 * 65535; the references are closed forms."""
    c = large("chain2048")
    t0 = time.perf_counter()
    h = hp.uf_create_matching(c.graph, 2048, c.w, 10)
    try:
        dist, mask = hp.uf_match_table(h)   # (waits for the table kernel)
        t_match = time.perf_counter() - t0
        info = hp.uf_info(h)
    finally:
        hp.uf_destroy(h)
    want_dist, want_mask, _ = c.tables[0]
    print(f"chain2048: tsim_uf_create_matching and the copy of its table took {t_match:.3f} s; entries that differ: dist "
          f"{int((dist != want_dist).sum())}, mask {int((mask != want_mask).sum())}; {info['device_bytes']} device bytes")
    assert np.array_equal(dist, want_dist) and np.array_equal(mask, want_mask)
    assert info["n_nodes"] == 2048 and info["device_bytes"] >= 12 * 2048 ** 2 and info["launches"] == 0
    for k in (0, 1):
        t0 = time.perf_counter()
        h = hp.uf_create_matching_gap(c.graph, 2048, c.w, 10, k)
        try:
            dist2, w0 = hp.uf_gap_table(h)
            t_gap = time.perf_counter() - t0
            again = hp.uf_match_table(h) if k == 0 else None
        finally:
            hp.uf_destroy(h)
        want = c.tables[k][2]
        print(f"chain2048: tsim_uf_create_matching_gap of observable {k} and the copy of its class table took {t_gap:.3f} s; entries that "
              f"differ {int((dist2 != want).sum())}, W0 {w0}")
        assert np.array_equal(dist2, want) and w0 is None   # tsim_uf_gap_table's -1: no node reaches the boundary in both classes
        if again is not None:
            assert np.array_equal(again[0], want_dist) and np.array_equal(again[1], want_mask)


def test_sparse2048_tables_against_a_heap_dijkstra(hp):
    """45 sources against the reference over every target (a block is a source: each covers every trip of the strided loops),
    and the whole device table against the invariants that need no reference."""
    c = large("sparse2048")
    g = c.graph
    t0 = time.perf_counter()
    h = hp.uf_create_matching_gap(g, 2048, c.w, 10, 0)
    try:
        dist, mask = hp.uf_match_table(h)
        dist2, w0 = hp.uf_gap_table(h)
        info = hp.uf_info(h)
    finally:
        hp.uf_destroy(h)
    want_dist, want_mask, want_dist2 = c.rows
    print(f"sparse2048: both tables of {len(c.sources)} sources in {time.perf_counter() - t0:.3f} s; entries that differ: dist "
          f"{int((dist[c.sources] != want_dist).sum())}, mask {int((mask[c.sources] != want_mask).sum())}, dist2 "
          f"{int((dist2[c.sources] != want_dist2).sum())}; W0 {w0}, {info['lds_bytes_per_shot']} bytes a shot, {info['shots_per_block']} shots a block")
    assert np.array_equal(dist[c.sources], want_dist)
    assert np.array_equal(mask[c.sources], want_mask)
    assert np.array_equal(dist2[c.sources], want_dist2)
    assert np.array_equal(dist[1:, 1:], dist[1:, 1:].T)
    assert (dist[0, 1:] == MATCH_INF).all() and dist[0, 0] == 0 and (np.diag(dist) == 0).all()
    assert np.array_equal(dist2.min(axis=2), dist)
    assert (dist[2045:, 2045:] != MATCH_INF).all() and (dist[2045:, :2045] == MATCH_INF).all() and (dist[1:2045, 2045:] == MATCH_INF).all()
    assert not mask[dist == MATCH_INF].any() and int(mask.max()) == 3
    both = (dist2[1:, 0, 0] != MATCH_INF) & (dist2[1:, 0, 1] != MATCH_INF)
    assert w0 == int((dist2[1:, 0, 0].astype(np.int64) + dist2[1:, 0, 1])[both].min())
    assert info["device_bytes"] >= 20 * 2048 ** 2 and info["max_defects"] == 10


def test_one_node_more_than_a_table_holds_is_refused(hp):
    u = np.arange(2048)
    g = DecodingGraph(2049, u, u + 1, np.zeros(2048, np.uint64))
    with pytest.raises(_lib.HipBackendError, match="at most 2048"):
        hp.uf_create_matching(g, 2049, np.ones(2048, np.int64), 10)
    with pytest.raises(_lib.HipBackendError, match="at most 2048"):
        hp.uf_create_matching_gap(g, 2049, np.ones(2048, np.int64), 10, 0)


# ---- 2. cluster matching and the gap on large surface codes --------------------------------------------------------------------

def matching_rows(hp, um, bits, what, waves):
    """One ``tsim_uf_decode_device`` per row layout on a matching handle against the statement."""
    nd, g = um.num_detectors, um.graph
    dets = bits[:, :nd]
    want_pred, want = host_statement(um, bits)
    clusters = um.match_counts(dets)
    for row_bytes, offset in two_layouts(bits.shape[1]):
        t0 = time.perf_counter()
        pred, got, info = matching_on_device(hp, um, bits, row_bytes, np.random.default_rng(row_bytes), offset=offset)
        line(f"{what} K = {um.match_defects}, rows of {row_bytes} bytes at +{offset}, clusters matched and peeled: host {clusters}, device "
             f"{(info['clusters_matched'], info['clusters_peeled'])}", want, got, int((pred != want_pred).sum()), info, t0)
        assert np.array_equal(pred, want_pred)
        assert got == want
        assert (info["clusters_matched"], info["clusters_peeled"], info["max_defects"]) == clusters + (um.match_defects,)
        assert info["max_rounds"] == int(um.growth_rounds(dets).max()) and info["rows_decoded"] == int(dets.any(axis=1).sum())
        assert info["lds_bytes_per_shot"] == uf_match_shot_bytes(g.n_nodes, g.n_edges, True, um.match_defects)
        assert info["shots_per_block"] == waves and info["launches"] == 1
    return want, clusters


@pytest.mark.parametrize("K", [4, 12])
def test_d9_matching_bit_for_bit(hp, K):
    c = large("d9")
    want, clusters = matching_rows(hp, c.matching[K], c.bits, "d9", D9_WAVES[K])
    assert clusters == {4: (1590, 267), 12: (1756, 101)}[K] and want[0] == 96 and want[1] > 0


def test_d11_matching_bit_for_bit(hp):
    c = large("d11")
    want, clusters = matching_rows(hp, c.matching[10], c.bits, "d11", 1)
    assert clusters == (1784, 50) and want[0] == 64


def test_d9_gap_in_a_block_it_nearly_fills(hp):
    """K = 12 with the classes: 63424 bytes a shot, the class program's arrays end 2096 bytes before the block does."""
    c = large("d9")
    ug, bits = c.gap, c.bits
    want = gap_statement(ug, bits)
    clusters = ug.match_counts(bits[:, :720])
    assert clusters == (1756, 101) and len(np.unique(want[2])) == 9
    for row_bytes, offset in two_layouts(721):
        t0 = time.perf_counter()
        got = gap_on_device(hp, ug, bits, row_bytes, np.random.default_rng(row_bytes), offset=offset)
        info = got[5]
        line(f"d9 gap K = 12, G = {ug.gap_cap}, step {ug.gap_step}, rows of {row_bytes} bytes at +{offset}, rows whose deficit differs "
             f"{int((got[2] != want[2]).sum())}", want[1], got[1], int((got[0] != want[0]).sum()), info, t0)
        assert np.array_equal(got[0], want[0])
        assert got[1] == want[1]
        assert np.array_equal(got[2], want[2])
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        assert got[3].sum() == want[1][0] and got[4].sum() == want[1][1]
        assert info["lds_bytes_per_shot"] == 63424 and 64 * 1024 - 16 - info["lds_bytes_per_shot"] < 2100
        assert (info["shots_per_block"], info["max_defects"], info["launches"]) == (D9_WAVES["gap"], 12, 1)
        assert (info["clusters_matched"], info["clusters_peeled"]) == clusters
        assert info["max_rounds"] == int(ug.growth_rounds(bits[:, :720]).max()) and info["rows_decoded"] == int(bits[:, :720].any(axis=1).sum())


def test_d11_with_both_dynamic_programs_is_refused(hp):
    um = large("d11").matching[10]
    with pytest.raises(_lib.HipBackendError, match="dynamic programs of max_defects: the winners and the classes"):
        hp.uf_create_matching_gap(um.graph, 1321, um.match_weights, 12, 0, um.edge_caps)
    hp.uf_destroy(hp.uf_create_matching(um.graph, 1321, um.match_weights, 12, um.edge_caps))   # (the winners alone fit)


# ---- 3. heralds on wide rows -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
def test_d9e_peeling_and_its_soft_outputs(hp, weighted):
    """``tsim_uf_create_heralds`` on rows of 739 bytes: 5184 heralds, most of them beyond column 4095."""
    c = large("d9e")
    uf = c.peeling[weighted]
    for row_bytes, offset in two_layouts(5905):
        t0 = time.perf_counter()
        (_, want), info = check_heralds(hp, uf, c.bits, row_bytes, offset)
        line(f"d9e peeling weighted = {weighted}, rows of {row_bytes} bytes at +{offset}", want, want, 0, info, t0)
        assert want[0] == 64 and info["shots_per_block"] == 1
    for metric, (row_bytes, offset) in zip(("largest_cluster", "full_edges"), two_layouts(5905)):
        soft = uf.with_soft_output(metric, 64)
        want = soft_statement(soft, c.bits)
        assert want[2][:, 1].max() > 256 and want[2][:, 2].max() > 128
        same(soft_on_device(hp, soft, c.bits, row_bytes, np.random.default_rng(3), offset=offset), want, f"d9e weighted = {weighted}, {metric}")


@pytest.mark.parametrize("weighted,K,H,gap", [(w, K, H, gap) for w in (False, True) for K, H, gap in D9E_HANDLES])
def test_d9e_erasure_matching_bit_for_bit(hp, weighted, K, H, gap):
    """As many tiles as the handle has waves a block, so each wave of a block decodes on its own state."""
    c = large("d9e")
    waves = D9E_WAVES[weighted, K, H, gap]
    _, clusters = erasure_rows(hp, c.handles[weighted, K, H, gap], tiles(c.bits, waves), waves, "d9e")
    if (weighted, K, H) == (True, 4, 8):
        assert clusters[1] == 156 * waves and clusters[3] == 12 * waves


def test_d9e_gap_on_quiet_rows(hp):
    """The class program under heralds where its result shows: rows whose clusters are all matched, 19 distinct deficits."""
    ug, bits = d9e_quiet()
    want, clusters = erasure_rows(hp, ug, tiles(bits, 3), 3, "d9e, quiet rows,")
    assert len(np.unique(want[2])) >= 16 and min(clusters) > 0


def erasure_rows(hp, ue, bits, waves, what):
    """One decode call per row layout on a handle of ``tsim_uf_create_matching_heralds`` against the statement."""
    weighted, K, H, gap = ue.edge_caps is not None, ue.match_defects, ue.max_hubs, ue.gap_observable is not None
    want = erasure_statement(ue, bits)
    clusters = cluster_counts(ue, bits)
    g = ue.graph
    for row_bytes, offset in two_layouts(5905):
        t0 = time.perf_counter()
        got = erasure_on_device(hp, ue, bits, row_bytes, np.random.default_rng(K), offset=offset)
        info = got[5]
        seen = (info["clusters_matched"], info["clusters_peeled"], info["clusters_erased"], info["clusters_hub_overflow"])
        line(f"{what} weighted = {weighted}, K = {K}, H = {H}, gap = {gap}, rows of {row_bytes} bytes at +{offset}, clusters matched, peeled, with an "
             f"erased edge, over H: host {clusters}, device {seen}", want[1], got[1], int((got[0] != want[0]).sum()), info, t0)
        assert np.array_equal(got[0], want[0])
        assert got[1] == want[1]
        if gap:
            assert np.array_equal(got[2], want[2])
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
            assert got[3].sum() == want[1][0] and got[4].sum() == want[1][1]
        assert seen == clusters
        assert (info["erased_weight"], info["max_hubs"], info["max_defects"]) == (1, H, K)
        assert (info["n_heralds"], info["n_det_cols"], info["launches"]) == (5184, 5904, 1)
        assert info["lds_bytes_per_shot"] == uf_erasure_shot_bytes(g.n_nodes, g.n_edges, weighted, K, H, gap)
        assert info["shots_per_block"] == waves and info["rows_decoded"] == int(bits[:, g.node_det].any(axis=1).sum()) > 60 * waves
        assert info["max_rounds"] == int(ue.growth_rounds(bits[:, :5904]).max())
    return want, clusters


def test_d9e_with_both_dynamic_programs_and_32_hubs_is_refused(hp):
    for weighted, uf in large("d9e").peeling.items():
        ue = uf.with_erasure_matching(12, max_hubs=32)
        with pytest.raises(_lib.HipBackendError, match="bytes of LDS.*hub graph of max_hubs"):
            hp.uf_create_matching_heralds(ue.graph, 5905, ue.match_weights, 12, 1, 32, 0, ue.edge_caps)


# ---- 4. soft outputs at their bounds ---------------------------------------------------------------------------------------------

def soft_rows(hp, uf, bits, metrics, bins, what):
    """Every metric listed, the row layouts in turn: all four values of every row and both histograms against the statement."""
    n_cols = bits.shape[1]
    info = handle_info(hp, uf, n_cols)
    for i, metric in enumerate(metrics):
        row_bytes, offset = two_layouts(n_cols)[i % 2]
        soft = uf.with_soft_output(metric, bins)
        want = soft_statement(soft, bits)
        t0 = time.perf_counter()
        got = soft_on_device(hp, soft, bits, row_bytes, np.random.default_rng(i), offset=offset)
        line(f"{what}, {metric} in {bins} bins, rows of {row_bytes} bytes at +{offset}, rows whose values differ "
             f"{int((got[2] != want[2]).any(axis=1).sum())}", want[1], got[1], int((got[0] != want[0]).sum()), info, t0)
        same(got, want, f"{what}, {metric}")
    return want


def test_soft_outputs_of_65535_full_edges(hp):
    """The herald that erases every edge: ``full << 16 | most`` of ``soft_of_growth`` carries 65535 in its upper half."""
    c = dense_erased()
    want = soft_rows(hp, c.uf, c.bits, METRICS, 64, "dense, every edge erased")
    assert (want[2][:, 1] == 65535).all() and (want[2][:, 2] == 400).all() and not want[2][:, 0].any()


def test_soft_outputs_of_the_long_chain(hp):
    c = case("chain1500")
    want = soft_rows(hp, c.plain, c.bits, ("correction_weight", "rounds"), 64, "chain1500")
    assert want[2][0, 3] == 700 and want[2][:, 0].max() > 1024 and want[2][:, 3].max() > 1024


def test_soft_outputs_at_d15(hp):
    c = case("d15")
    want = soft_rows(hp, c.plain, c.bits, METRICS, 64, "d15")
    assert len(c.bits) == 48 and c.plain.graph.n_nodes == 3361 and want[2][:, 1].max() > 64


# ---- 5. a grid that wraps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["gap", "erasure"])
def test_matching_grids_wrap(hp, kind):
    """More tiles than the grid has waves, twice over and a ragged end, on a handle with both dynamic programs: a wave carries
    ``matched_acc``, ``peeled_acc``, ``erased_acc``, ``hubs_acc`` and the registers of its bin 0 across its tiles.  The rows are a
    base of 1061 seeded rows, repeated; the host decodes the base."""
    ug, base = wrap_base(kind)
    nd, n_cols, B = ug.num_detectors, base.shape[1], ug.soft_bins
    info = handle_info(hp, ug, n_cols)
    per_launch = info["grid_blocks"] * info["shots_per_block"] * 64
    n = 2 * per_launch + 64 * 3 + 5
    assert n > 3 * len(base) and len(base) % 64 and per_launch % len(base)   # (a wave's next tile is not the same rows again)
    dets = base[:, :nd]
    base_pred, base_D = ug.predictions(dets), ug.gap_outputs(dets)
    per_row = np.array([ug.match_counts(dets[r:r + 1]) + (ug.erasure_counts(dets[r:r + 1]) if kind == "erasure" else ()) for r in range(len(base))])
    wrong = np.resize(base_pred != base[:, nd].astype(np.uint64), n)
    bins = np.resize(np.minimum(base_D // ug.gap_step, B - 1), n)
    want = (n, int(wrong.sum()), int(np.resize(ug.missed(dets), n).sum()))
    want_clusters = tuple(int(x) for x in np.resize(per_row, (n, per_row.shape[1])).sum(axis=0))
    row_bytes = (n_cols + 7) // 8
    rows = np.resize(packed(base, row_bytes, np.random.default_rng(5)), (n, row_bytes))
    pred, cnt, D, hist = np.zeros(n, np.uint64), np.zeros(3, np.uint64), np.zeros(n, np.uint32), np.zeros(2 * B, np.uint64)
    bufs = [hp.malloc(rows.nbytes + 64), hp.malloc(pred.nbytes), hp.malloc(64), hp.malloc(D.nbytes), hp.malloc(hist.nbytes)]
    h, _, destroy = ug._handle(hp, n_cols)
    t0 = time.perf_counter()
    try:
        for a, b in ((rows, bufs[0]), (cnt, bufs[2]), (hist, bufs[4])):
            hp.h2d(b, a)
        hp.uf_decode_gap_device(h, bufs[0].ptr, n, row_bytes, (nd, nd + 1), bufs[2].ptr, ug.gap_cap, ug.gap_step, B, bufs[4].ptr, d_gap=bufs[3].ptr,
                                d_pred=bufs[1].ptr)
        info = dict(hp.uf_info(h), **(hp.uf_erasure_info(h) if kind == "erasure" else {}))   # (waits for the decode)
        for a, b in ((pred, bufs[1]), (cnt, bufs[2]), (D, bufs[3]), (hist, bufs[4])):
            hp.d2h(a, b)
    finally:
        destroy(h)
        for b in bufs:
            b.free()
    got = tuple(int(x) for x in cnt)
    seen = (info["clusters_matched"], info["clusters_peeled"]) + ((info["clusters_erased"], info["clusters_hub_overflow"]) if kind == "erasure" else ())
    line(f"{kind}: {n} rows, clusters host {want_clusters}, device {seen}, rows whose deficit differs {int((D != np.resize(base_D, n)).sum())}",
         want, got, int((pred != np.resize(base_pred, n)).sum()), info, t0)
    assert np.array_equal(pred, np.resize(base_pred, n))
    assert got == want and want[1] > 0
    assert np.array_equal(D, np.resize(base_D, n))
    assert np.array_equal(hist[:B].astype(np.int64), np.bincount(bins, minlength=B))
    assert np.array_equal(hist[B:].astype(np.int64), np.bincount(bins[wrong], minlength=B))
    assert seen == want_clusters and all(x > 0 for x in seen[:1] + seen[2:])
    assert info["rows_decoded"] == int(np.resize(base[:, ug.graph.node_det].any(axis=1), n).sum()) and info["launches"] == 1
    assert info["max_rounds"] == int(ug.growth_rounds(dets).max())


# ---- 6. windows with heralds on a long run ---------------------------------------------------------------------------------------

def test_d3x120e_windows_bit_for_bit(hp):
    """120 rounds in 23 windows, 5760 heralds on rows of 841 bytes: the herald sweep of ``k_ufw`` reads a second word a lane."""
    c = large("d3x120e")
    for row_bytes, offset in two_layouts(6721):
        t0 = time.perf_counter()
        (_, want), info = check_windows(hp, c.w, c.bits, row_bytes, offset)
        line(f"d3x120e rows of {row_bytes} bytes at +{offset}, windows decoded {info['windows_decoded']}", want, want, 0, info, t0)
        assert want[0] == 130 and info["n_windows"] == 23


@pytest.mark.parametrize("metric", ["largest_cluster", "rounds"])
def test_d3x120e_windowed_soft_outputs(hp, metric):
    c = large("d3x120e")
    info = handle_info(hp, c.w, 6721)
    soft = c.w.with_soft_output(metric, 16)
    want = soft_statement(soft, c.bits)
    assert want[2][:, 2].max() >= 16 and want[2][:, 1].max() > 255 and (want[3][0] > 0).sum() >= 3
    for row_bytes, offset in two_layouts(6721):
        t0 = time.perf_counter()
        got = soft_on_device(hp, soft, c.bits, row_bytes, np.random.default_rng(2), offset=offset)
        line(f"d3x120e {metric}, rows of {row_bytes} bytes at +{offset}, rows whose values differ {int((got[2] != want[2]).any(axis=1).sum())}",
             want[1], got[1], int((got[0] != want[0]).sum()), info, t0)
        same(got, want, f"d3x120e, {metric}")
