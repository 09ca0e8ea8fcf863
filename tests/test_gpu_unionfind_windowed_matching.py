"""Cluster matching in windows on the GPU (``tsim_ufw_create_matching``, ``k_ufw<., false, false, true>`` of ``csrc/tsim_ufw.hip.h``):
predictions, counters and cluster counts of the device bit for bit against the numpy statement
(``WindowedUnionFindDecoder.with_cluster_matching``), every window's table against ``window_match_table``, and ``count()``."""

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_gpu_unionfind_windowed import check, d3_rows, with_observables
from test_unionfind_windowed import fire, time_ladder
from test_unionfind_windowed_matching import fingerprint_decoder

from tsim_amd import synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import UnionFindDecoder, WindowedUnionFindDecoder, ufw_match_shot_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def on_handle(hp, wm, bits, row_bytes, seed):
    """Predictions and counters of a handle of ``ufw_create_matching`` that decoded ``bits``, bit for bit against the numpy
    statement; ``(tsim_ufw_info, tsim_ufw_match_info)`` of the handle afterwards."""
    want_pred, want = host_statement(wm, bits)
    rows = packed(bits, row_bytes, np.random.default_rng(seed))
    n_cols = bits.shape[1]
    h = hp.ufw_create_matching(wm.graph, n_cols, wm.match_weights, wm.match_defects, wm.commit, wm.window, wm.edge_caps)
    bufs = [hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(8 * len(rows) + 16)]
    try:
        hp.h2d(bufs[0], rows)
        hp.h2d(bufs[1], np.zeros(3, np.uint64))
        nd = wm.num_detectors
        hp.ufw_decode_device(h, bufs[0].ptr, len(rows), row_bytes, (nd, nd + wm.num_observables), bufs[1].ptr, d_pred=bufs[2].ptr)
        info, match = hp.ufw_info(h), hp.ufw_match_info(h)
        pred, cnt = np.zeros(len(rows), np.uint64), np.zeros(3, np.uint64)
        hp.d2h(pred, bufs[2])
        hp.d2h(cnt, bufs[1])
        with pytest.raises(ValueError, match="no soft outputs"):
            hp.ufw_decode_soft_device(h, bufs[0].ptr, len(rows), row_bytes, (nd, nd + 1), bufs[1].ptr, "rounds", 8, bufs[2].ptr)
    finally:
        hp.ufw_destroy(h)
        for b in bufs:
            b.free()
    print(f"host {want}, device {cnt.tolist()}, rows that differ {int((pred != want_pred).sum())}, {match}")
    assert np.array_equal(pred, want_pred) and tuple(int(x) for x in cnt) == want
    counts = wm.match_counts(bits[:, :wm.num_detectors]).sum(0)
    assert (match["clusters_matched"], match["clusters_peeled"]) == (int(counts[0]), int(counts[1])) and match["max_defects"] == wm.match_defects
    assert match["table_bytes"] == 6 * sum(w.graph.n_nodes ** 2 for w in distinct_windows(wm)) and 0 < match["longest_path"] < info["max_window_nodes"]
    return info, match


def distinct_windows(wm):
    """The first window of every set of windows whose local arrays are equal: those the library builds a table for."""
    seen, out = set(), []
    for w in wm.windows():
        g = w.graph
        key = (g.n_nodes, g.edge_u.tobytes(), g.edge_v.tobytes(), g.edge_obs.tobytes(), w.weights.tobytes(), w.committed.tobytes())
        if key not in seen:
            seen.add(key)
            out.append(w)
    return out


@pytest.mark.parametrize("weights,K,units", [(None, 10, False), ("probability", 10, False), (None, 2, False), ("probability", 2, False),
                                             (None, 10, True)])
def test_surface_code_rows_bit_for_bit(hp, weights, K, units):
    """The d = 3 rows of the windowed tests: 5 windows of 32 columns, 13-byte rows.  K = 2 peels most clusters of three and more
    defects beside the matched ones; unit match weights make every tie rule decide."""
    c, bits = d3_rows()
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights=weights)
    wm = w.with_cluster_matching(K, np.ones(w.graph.n_edges, np.int64) if units else None)
    info, match = on_handle(hp, wm, bits, 13, 1)
    assert info["n_windows"] == 5 and match["distinct_tables"] == len(distinct_windows(wm)) < 5
    assert info["lds_bytes_per_shot"] == ufw_match_shot_bytes(info["max_window_nodes"], info["max_window_edges"], weights is not None, K, 32)
    assert match["clusters_matched"] > 1000 and (match["clusters_peeled"] > 300) == (K == 2)   # (K = 10 peels two or three clusters)
    assert K == 2 or (wm.predictions(bits[:, :96]) != w.predictions(bits[:, :96])).any()


def test_a_fingerprint_of_the_committed_flips(hp):
    """64 observables, a random mask per edge: a prediction names the set of committed flips, of matched and of peeled clusters."""
    wm = fingerprint_decoder(6)
    _, bits = d3_rows()
    rng = np.random.default_rng(11)
    bits = with_observables(bits[:, :96], rng, 64)
    pred, want = check(hp, wm, bits, 24, 2)
    assert len(set(pred.tolist())) > 150 and want[2] == 0 and wm.match_counts(bits[:, :96])[:, 1].sum() > 0


def test_every_window_table(hp):
    c, _ = d3_rows()
    ladder, caps = time_ladder(3, 8)
    for wm in (WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights="probability").with_cluster_matching(10),
               WindowedUnionFindDecoder(ladder, 6, 12, edge_caps=caps).with_cluster_matching(4, np.ones(ladder.n_edges, np.int64))):
        h = hp.ufw_create_matching(wm.graph, wm.num_detectors + 1, wm.match_weights, wm.match_defects, wm.commit, wm.window, wm.edge_caps)
        try:
            for k in range(len(wm.windows())):
                dist, parent = hp.ufw_match_table(h, k)
                want_dist, want_parent = wm.window_match_table(k)
                assert np.array_equal(dist, want_dist) and np.array_equal(parent, want_parent), k
            with pytest.raises(ValueError, match="window"):
                hp.ufw_match_table(h, len(wm.windows()))
        finally:
            hp.ufw_destroy(h)


def test_a_carry_that_survives_two_window_advances(hp):
    """The skip ladder, commit = 2, window = 6: a committed edge of a path toggles a column that the window after the next commits."""
    g, caps = time_ladder(2, 6, both_ends=False, skip=True)
    rng = np.random.default_rng(3)
    for edge_caps in (None, caps):
        wm = WindowedUnionFindDecoder(g, 2, 6, edge_caps=edge_caps).with_cluster_matching(4, caps.astype(np.int64) * 100 + 1)
        assert wm.info()["n_windows"] == 4
        bits = with_observables(fire(g, rng, 300, 0.08), rng)
        assert (wm.mixed_pairs(bits[:, :12]) > 0).sum() > 5
        check(hp, wm, bits, 2, 4)


def test_masks_and_a_ragged_row_count(hp):
    """``d_xor`` and ``d_test``, 201 rows (no multiple of 64) at an odd address, 16-byte rows."""
    c, bits = d3_rows()
    wm = WindowedUnionFindDecoder.from_circuit(c, 16, 32).with_cluster_matching()
    rng = np.random.default_rng(5)
    xor = rng.random(97) < 0.05
    test = np.zeros(97, np.bool_)
    test[[3, 50, 90]] = True
    pred, want = check(hp, wm, bits[:201], 16, 2, xor=xor, test=test, offset=3)
    keep = ~((bits[:201] ^ xor) & test).any(axis=1)
    assert 0 < want[0] == int(keep.sum()) < 201 and want[1] > 0 and not pred[~keep].any() and pred[keep].any()


@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_equals_a_whole_graph_matching_handle(hp, weights):
    c, bits = d3_rows()
    um = UnionFindDecoder.from_circuit(c, weights=weights).with_cluster_matching(10)
    wm = WindowedUnionFindDecoder.from_circuit(c, 16, 96, weights=weights).with_cluster_matching(10)
    rows = packed(bits, 16, np.random.default_rng(8))
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        whole = um.decode_device(hp, d_rows.ptr, len(rows), 16)
        windowed = wm.decode_device(hp, d_rows.ptr, len(rows), 16)
    finally:
        d_rows.free()
    assert np.array_equal(windowed[0], whole[0]) and windowed[1] == whole[1] and whole[0].any()
    assert np.array_equal(whole[0], um.predictions(bits[:, :96]))


@pytest.mark.parametrize("K,commit,window", [(12, 32, 64), (10, 500, 1000)])
def test_the_time_ladder(hp, K, commit, window):
    """8 checks x 520 rounds: windows of 64 columns with the 2^12 subsets of K = 12, and windows of 1000 columns (tables of 1001^2
    pairs, the bulk windows sharing one)."""
    g, caps = time_ladder(8, 520)
    rng = np.random.default_rng(12)
    bits = with_observables(fire(g, rng, 160, 1e-3), rng)
    wm = WindowedUnionFindDecoder(g, commit, window, edge_caps=caps).with_cluster_matching(K, caps.astype(np.int64) * 100 + 1)
    info, match = on_handle(hp, wm, bits, 528, 13)
    assert info["max_window_nodes"] == window + 1 and info["lds_bytes_per_shot"] * info["shots_per_block"] + 16 <= 64 * 1024
    assert info["lds_bytes_per_shot"] == ufw_match_shot_bytes(window + 1, info["max_window_edges"], True, K, window)
    assert match["distinct_tables"] <= 4 < info["n_windows"]


def test_count_equals_the_host_tally_of_the_same_sample(hip):
    c, _ = d3_rows()
    wm = WindowedUnionFindDecoder.from_circuit(c, 16, 32).with_cluster_matching()
    nd = wm.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[0, 70]] = True
    for corrected in (False, True):
        rows = c.compile_detector_sampler(seed=21, method="faults").sample(4096, append_observables=True)
        got = c.compile_detector_sampler(seed=21, method="faults").count(4096, decoder=wm, postselection_mask=mask, corrected=corrected)
        want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=wm, histogram_columns=(nd,), corrected=corrected)
        assert got == want
        assert 0 < got.kept < 4096 and 0 < got.decoded_errors < got.kept and got.decoder_misses == 0
