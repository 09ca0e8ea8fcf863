"""Sliding-window union-find decoding on the GPU (``tsim_ufw_*``, ``k_ufw`` of ``csrc/tsim_ufw.hip.h``): predictions and counters
of ``decode_device`` bit for bit against the numpy statement (``tsim_amd.decode.WindowedUnionFindDecoder``), whose windows the
library builds a second time by itself; rows are packed by numpy and uploaded."""

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, on_device, packed
from test_unionfind_windowed import fire, long_memory, time_ladder

from tsim_amd import _lib, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import UnionFindDecoder, WindowedUnionFindDecoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def with_observables(dets: np.ndarray, rng, n_obs: int = 1) -> np.ndarray:
    return np.concatenate([dets, rng.integers(0, 2, size=(len(dets), n_obs)).astype(np.bool_)], axis=1)


_ROWS: dict = {}


def d3_rows():
    """The d = 3, 12 rounds circuit and 256 rows (96 detectors, 1 observable) from edge firing; rows 0 .. 7 are all zero in
    their detectors and rows 8 .. 23 have defects in the last window's columns [64, 96) only."""
    if not _ROWS:
        c = long_memory()
        g = UnionFindDecoder.from_circuit(c).graph
        rng = np.random.default_rng(7)
        dets = fire(g, rng, 256)
        dets[:8] = False
        dets[8:24, :64] = False
        dets[8:24, 64:] |= fire(g, rng, 16, 0.03)[:, 64:]
        _ROWS["d3"] = (c, with_observables(dets, rng))
    return _ROWS["d3"]


def check(hp, w, bits, row_bytes, seed, **kw):
    want_pred, want = host_statement(w, bits, kw.get("xor"), kw.get("test"))
    pred, got = on_device(hp, w, bits, row_bytes, np.random.default_rng(seed), **kw)
    print(f"host {want}, device {got}, rows that differ {int((pred != want_pred).sum())}")
    assert np.array_equal(pred, want_pred)
    assert got == want
    return want_pred, want


@pytest.mark.parametrize("weights", [None, "probability"])
def test_surface_code_rows_bit_for_bit(hp, weights):
    """5 windows of 32 columns, a carry bitmap of exactly 32 bits that wraps twice; weighted: the 4-bit counters."""
    c, bits = d3_rows()
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights=weights)
    assert w.info()["n_windows"] == 5 and not bits[:8, :96].any() and bits[8:24, 64:96].any(axis=1).all()
    pred, want = check(hp, w, bits, 13, 1)
    assert want[0] == 256 and 0 < want[1] < 256 and want[2] == 0 and pred.any() and not pred[:8].any()
    assert (pred != UnionFindDecoder.from_circuit(c, weights=weights).predictions(bits[:, :96])).any()  # (windows are not the whole graph)


def test_masks_and_a_ragged_row_count(hp):
    """``d_xor`` and ``d_test``, 201 rows (no multiple of 64) at an odd address."""
    c, bits = d3_rows()
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32)
    rng = np.random.default_rng(5)
    xor = rng.random(97) < 0.05
    test = np.zeros(97, np.bool_)
    test[[3, 50, 90]] = True
    pred, want = check(hp, w, bits[:201], 16, 2, xor=xor, test=test, offset=3)
    keep = ~((bits[:201] ^ xor) & test).any(axis=1)
    assert 0 < want[0] == int(keep.sum()) < 201 and want[1] > 0 and not pred[~keep].any() and pred[keep].any()


def test_a_carry_that_survives_two_window_advances(hp):
    """The hand-made ladder of 2 checks with edges that skip a round, commit = 2, window = 6 = 3 commit: a committed flip of a
    skip edge in window k toggles column lo + 4, which window k + 1 holds outside its commit region and window k + 2 commits."""
    g, caps = time_ladder(2, 6, both_ends=False, skip=True)
    rng = np.random.default_rng(3)
    for edge_caps in (None, caps):
        w = WindowedUnionFindDecoder(g, 2, 6, edge_caps=edge_caps)
        assert w.info()["n_windows"] == 4
        bits = with_observables(fire(g, rng, 300, 0.08), rng)
        skips = np.flatnonzero((g.edge_v - g.edge_u == 4) & (g.edge_u > 0) & (g.edge_u <= 4))  # (committed in windows 0 and 1)
        assert sum(np.isin(skips, f).any() for f in w.flipped_edges(bits[:, :12])) > 5
        check(hp, w, bits, 2, 4)


@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_equals_the_whole_graph_handle(hp, weights):
    c, bits = d3_rows()
    uf = UnionFindDecoder.from_circuit(c, weights=weights)
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 96, weights=weights)
    rows = packed(bits, 16, np.random.default_rng(8))
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        whole = uf.decode_device(hp, d_rows.ptr, len(rows), 16)
        windowed = w.decode_device(hp, d_rows.ptr, len(rows), 16)
    finally:
        d_rows.free()
    assert np.array_equal(windowed[0], whole[0]) and windowed[1] == whole[1] and whole[0].any()
    assert np.array_equal(whole[0], uf.predictions(bits[:, :96]))


def ladder_on_device(hp, w, bits, row_bytes, seed):
    """``decode_device``'s results and ``tsim_ufw_info`` of a handle that decoded the same rows."""
    want_pred, want = host_statement(w, bits)
    rows = packed(bits, row_bytes, np.random.default_rng(seed))
    n_cols = bits.shape[1]
    h = hp.ufw_create(w.graph, n_cols, w.commit, w.window, w.edge_caps)
    bufs = [hp.malloc(rows.nbytes), hp.malloc(64), hp.malloc(8 * len(rows) + 16)]
    try:
        hp.h2d(bufs[0], rows)
        hp.h2d(bufs[1], np.zeros(3, np.uint64))
        hp.ufw_decode_device(h, bufs[0].ptr, len(rows), row_bytes, (n_cols - 1, n_cols), bufs[1].ptr, d_pred=bufs[2].ptr)
        info = hp.ufw_info(h)
        pred, cnt = np.zeros(len(rows), np.uint64), np.zeros(3, np.uint64)
        hp.d2h(pred, bufs[2])
        hp.d2h(cnt, bufs[1])
    finally:
        hp.ufw_destroy(h)
        for b in bufs:
            b.free()
    print(f"host {want}, device {cnt.tolist()}, rows that differ {int((pred != want_pred).sum())}, info {info}")
    assert np.array_equal(pred, want_pred) and tuple(int(x) for x in cnt) == want
    return info, want


def test_a_graph_whose_state_does_not_fit_lds_decodes_in_windows(hp):
    """8 checks x 1300 rounds: 10401 nodes, 91 KiB of state for the whole graph; 324 windows of 65 nodes."""
    g, caps = time_ladder(8, 1300)
    with pytest.raises(_lib.HipBackendError, match="bytes of LDS"):
        hp.uf_create(g, g.n_nodes)
    w = WindowedUnionFindDecoder(g, 32, 64, edge_caps=caps)
    rng = np.random.default_rng(9)
    bits = with_observables(fire(g, rng, 64, 1.5e-3), rng)
    bits[0, :-1] = False
    info, want = ladder_on_device(hp, w, bits, (bits.shape[1] + 7) // 8, 10)
    assert (info["n_nodes"], info["n_windows"], info["max_window_nodes"], info["launches"]) == (10401, 324, 65, 1)
    assert info["rows_decoded"] == 63 and info["rows_decoded"] < info["windows_decoded"] < 63 * 324 and want[2] == 0 and 0 < want[1] < 64
    assert info["max_rounds"] == int(w.growth_rounds(bits[:, :-1]).max())


def test_one_to_four_shots_per_block_follow_from_the_window(hp):
    """8 checks x 520 rounds in windows of 64 columns (under 1 KB of state) and of 2000 columns (20 KB)."""
    g, caps = time_ladder(8, 520)
    rng = np.random.default_rng(12)
    bits = with_observables(fire(g, rng, 160, 1e-3), rng)
    seen = set()
    for commit, window in ((32, 64), (1000, 2000)):
        w = WindowedUnionFindDecoder(g, commit, window, edge_caps=caps)
        info, _ = ladder_on_device(hp, w, bits, 528, 13)
        assert info["max_window_nodes"] == window + 1 and info["lds_bytes_per_shot"] * info["shots_per_block"] + 16 <= 64 * 1024
        seen.add(info["shots_per_block"])
    assert len(seen) == 2


def test_count_equals_the_host_tally_of_the_same_sample(hip):
    c, _ = d3_rows()
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32)
    nd = w.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[0, 70]] = True
    rows = c.compile_detector_sampler(seed=21, method="faults").sample(4096, append_observables=True)
    got = c.compile_detector_sampler(seed=21, method="faults").count(4096, decoder=w, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=w, histogram_columns=(nd,))
    assert got == want
    assert 0 < got.kept < 4096 and 0 < got.decoded_errors < got.kept_with_observable_flip and got.decoder_misses == 0
