"""Cluster matching of the union-find decoder on the GPU (``tsim_uf_create_matching``, ``k_uf<., false, false, true>`` of
``csrc/tsim_uf.hip.h``, the table kernel of ``csrc/tsim_uf_match.hip.h``): the match table, the predictions, the counters and
``tsim_uf_info`` bit for bit against the numpy statement, ``count(decoder=...)``, ``count(..., corrected=True)`` and
``decode_file`` against it, and what ``tsim_uf_create_matching`` refuses.  Every graph and row is valid: nothing here asks the
kernel for an index its tables do not hold."""

import ctypes as C

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_unionfind import chain_graph
from test_unionfind_matching import chain_rows, issue_memory, matching_decoder, table_cases

from tsim_amd import _lib, faults, shotdata, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodeFileResult, UnionFindDecoder, uf_match_shot_bytes

pytestmark = pytest.mark.gpu

_ROWS: dict = {}


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def sample(p: float, weighted: bool):
    """``(peeling decoder, 512 rows)`` of d = 3, r = 3 at ``p`` (``fault_rows_host`` under key (1, 2)), built once."""
    if (p, weighted) not in _ROWS:
        c = issue_memory(3, 3, p)
        uf = UnionFindDecoder.from_circuit(c, weights="probability" if weighted else None)
        _ROWS[p, weighted] = (uf, faults.fault_rows_host(c.compile_faults(), 0, 512, (1, 2)).view(np.bool_))
    return _ROWS[p, weighted]


def on_device(hp, um, bits, row_bytes, rng, xor=None, test=None, offset=0):
    """``(predictions, (kept, wrong, missed), tsim_uf_info)`` of one decode call by a handle of ``um``."""
    n, n_cols = bits.shape
    nd = um.num_detectors
    rows = packed(bits, row_bytes, rng)
    pred, cnt = np.zeros(n, np.uint64), np.zeros(3, np.uint64)
    bufs = [hp.malloc(rows.nbytes + 64), hp.malloc(pred.nbytes + 16), hp.malloc(64)]
    h, decode, destroy = um._handle(hp, n_cols)
    try:
        hp.h2d(bufs[0].ptr + offset, rows)
        hp.h2d(bufs[2], cnt)
        masks = {}
        for name, m in (("d_xor", xor), ("d_test", test)):
            if m is not None:
                bufs.append(hp.malloc(64 + (n_cols + 7) // 8))
                hp.h2d(bufs[-1], np.packbits(m, bitorder="little"))
                masks[name] = bufs[-1].ptr
        decode(h, bufs[0].ptr + offset, n, row_bytes, (nd, nd + um.num_observables), bufs[2].ptr, d_pred=bufs[1].ptr, **masks)
        info = hp.uf_info(h)  # (synchronises)
        hp.d2h(pred, bufs[1])
        hp.d2h(cnt, bufs[2])
        return pred, tuple(int(x) for x in cnt), info
    finally:
        destroy(h)
        for b in bufs:
            b.free()


def check(hp, um, bits, row_bytes, rng, xor=None, test=None, offset=0):
    """One decode call against the statement: predictions, counters and every number of ``tsim_uf_info`` the rows decide."""
    nd, g = um.num_detectors, um.graph
    want_pred, want = host_statement(um, bits, xor, test)
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    dets = b[keep][:, :nd]
    pred, got, info = on_device(hp, um, bits, row_bytes, rng, xor, test, offset)
    matched, peeled = um.match_counts(dets)
    print(f"K = {um.match_defects}: host {want}, device {got}, rows that differ {int((pred != want_pred).sum())}, clusters matched {matched} "
          f"({info['clusters_matched']}), peeled {peeled} ({info['clusters_peeled']})")
    assert np.array_equal(pred, want_pred)
    assert got == want
    assert (info["clusters_matched"], info["clusters_peeled"], info["max_defects"]) == (matched, peeled, um.match_defects)
    assert info["max_rounds"] == (int(um.growth_rounds(dets).max()) if len(dets) else 0)
    assert info["rows_decoded"] == int(dets.any(axis=1).sum())
    assert info["lds_bytes_per_shot"] == uf_match_shot_bytes(g.n_nodes, g.n_edges, um.edge_caps is not None, um.match_defects)
    assert 16 + info["shots_per_block"] * info["lds_bytes_per_shot"] <= 64 * 1024
    return want, (matched, peeled)


# ---- the match table ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(table_cases()))
def test_match_table_bit_for_bit(hp, name):
    graph, w = table_cases()[name]
    um = matching_decoder(graph, w)
    want_dist, want_mask = um.match_table()
    h = hp.uf_create_matching(graph, graph.n_nodes, w, 10)
    try:
        dist, mask = hp.uf_match_table(h)
        info = hp.uf_info(h)
    finally:
        hp.uf_destroy(h)
    assert np.array_equal(dist, want_dist)
    assert np.array_equal(mask, want_mask)
    assert info["device_bytes"] >= 12 * graph.n_nodes ** 2 and info["max_defects"] == 10 and info["launches"] == 0


# ---- decoded rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 10, 12])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("p", [3e-3, 2e-2])
def test_surface_code_rows_bit_for_bit(hp, p, weighted, K):
    """p = 2e-2 gives clusters of more than two defects and, at K = 1 and 2, matched and peeled clusters in one row."""
    uf, bits = sample(p, weighted)
    um = uf.with_cluster_matching(K)
    want, (matched, peeled) = check(hp, um, bits, 4, np.random.default_rng(K))
    assert want[0] == 512 and matched > 0
    if p == 2e-2:
        assert want[1] > 0
        if K <= 2:  # a row that holds both kinds
            dets = bits[:, :um.num_detectors]
            assert peeled > 0
            assert any(um.match_counts(dets[r:r + 1])[0] and um.match_counts(dets[r:r + 1])[1] for r in range(len(dets)))


@pytest.mark.parametrize("K", [1, 2, 10, 12])
@pytest.mark.parametrize("weighted", [False, True])
def test_chain_rows_of_k_and_k_plus_one_defects(hp, K, weighted):
    """Runs of exactly K and of K + 1 defects on the chain of 70 nodes (node indices beyond 64), alone and together, a row of
    boundary clusters only, and two single defects far apart; weights that rise along the chain."""
    caps = np.resize([1, 14, 3, 8], 69) if weighted else None
    um = matching_decoder(chain_graph(70), np.arange(1, 70), K, caps)
    dets = chain_rows([[(20, K)], [(20, K + 1)], [(10, K), (40, K + 1)], [(50, K + 1), (30, K)], [(1, 1)], [(1, 2)], [(2, 1)], [(29, 1), (49, 1)],
                       [(56, 12)], [(57, 13)]])
    bits = np.concatenate([dets, np.zeros((len(dets), 1), np.bool_)], axis=1)
    bits[::2, -1] = True
    _, (matched, peeled) = check(hp, um, bits, 10, np.random.default_rng(K))
    assert matched >= 4 and peeled >= 2


def test_stride_offset_and_masks(hp):
    """Rows of 5 bytes (no multiple of 8) at an odd offset into their buffer, an xor mask and a test mask."""
    uf, bits = sample(2e-2, True)
    um = uf.with_cluster_matching(2)
    rng = np.random.default_rng(5)
    n_cols = bits.shape[1]
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, np.bool_)
    test[[1, 16]] = True
    want, (matched, peeled) = check(hp, um, bits, 5, rng, xor=xor, test=test, offset=3)
    assert 0 < want[0] < len(bits) and want[1] > 0 and matched > 0 and peeled > 0
    check(hp, um, bits, 8, rng, offset=8)  # (the 8-byte loads)


def test_two_calls_accumulate(hp):
    uf, bits = sample(2e-2, False)
    um = uf.with_cluster_matching(2)
    nd = um.num_detectors
    rows = packed(bits, 4, np.random.default_rng(6))
    _, want = host_statement(um, bits)
    matched, peeled = um.match_counts(bits[:, :nd])
    h = hp.uf_create_matching(um.graph, nd + 1, um.match_weights, 2)
    d_rows, d_cnt = hp.malloc(rows.nbytes), hp.malloc(64)
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, np.array([5, 0, 0], np.uint64))
        for _ in range(2):
            hp.uf_decode_device(h, d_rows.ptr, len(rows), 4, (nd, nd + 1), d_cnt.ptr)
        info = hp.uf_info(h)
        cnt = np.zeros(3, np.uint64)
        hp.d2h(cnt, d_cnt)
        assert cnt.tolist() == [5 + 2 * want[0], 2 * want[1], 2 * want[2]]
        assert (info["launches"], info["clusters_matched"], info["clusters_peeled"]) == (2, 2 * matched, 2 * peeled)
        plain = hp.uf_create(um.graph, nd + 1)
        try:
            other = hp.uf_info(plain)
        finally:
            hp.uf_destroy(plain)
        assert (other["max_defects"], other["clusters_matched"], other["clusters_peeled"]) == (0, 0, 0)
    finally:
        hp.uf_destroy(h)
        d_rows.free()
        d_cnt.free()


# ---- count() and decode_file -------------------------------------------------------------------------------------------------

SHOTS = 4096


def counted():
    """``(circuit, matching decoder, sample(4096) under seed 5 by method="faults")`` of d = 3, r = 3 at p = 1e-2, built once."""
    if "count" not in _ROWS:
        c = issue_memory(3, 3, 1e-2)
        um = UnionFindDecoder.from_circuit(c, weights="probability").with_cluster_matching()
        rows = c.compile_detector_sampler(seed=5, method="faults").sample(SHOTS, append_observables=True)
        rows.setflags(write=False)
        _ROWS["count"] = (c, um, rows)
    return _ROWS["count"]


@pytest.mark.parametrize("corrected", [False, True])
def test_count_equals_the_statement(hip, corrected):
    c, um, rows = counted()
    nd = um.num_detectors
    got = c.compile_detector_sampler(seed=5, method="faults").count(SHOTS, decoder=um, corrected=corrected)
    want = tally_rows(rows, num_detectors=nd, decoder=um, corrected=corrected, histogram_columns=(nd,))
    obs = np.asarray(rows)[:, nd].astype(np.uint64)
    wrong = int((um.predictions(np.asarray(rows)[:, :nd].astype(np.bool_)) != obs).sum())
    print(f"kept {got.kept}, decoded errors {got.decoded_errors} (statement {wrong}), misses {got.decoder_misses}")
    assert got == want
    assert (got.kept, got.decoded_errors, got.decoder_misses) == (SHOTS, wrong, 0) and wrong > 0
    assert got.corrected == corrected


def test_decode_file_equals_the_statement(hp, tmp_path):
    _, um, rows = counted()
    rows = np.asarray(rows).astype(np.bool_)
    nd, n_obs = um.num_detectors, um.num_observables
    src, dst = tmp_path / "events.b8", tmp_path / "predictions.01"
    shotdata.write_shot_data_file(data=np.ascontiguousarray(rows), path=src, format="b8", num_detectors=nd, num_observables=n_obs)
    want = um.decode(rows[:, :nd])
    wrong = int((want != rows[:, nd:]).any(axis=1).sum())
    res = um.decode_file(detection_events_filepath=src, detection_events_format="b8", predictions_filepath=dst, predictions_format="01",
                         observables_appended=True, hp=hp)
    assert res == DecodeFileResult(SHOTS, SHOTS, wrong, 0) and wrong > 0
    got = shotdata.read_shot_data_file(path=dst, format="01", num_observables=n_obs)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- what tsim_uf_create_matching refuses ------------------------------------------------------------------------------------

def test_refusals(hp):
    g = chain_graph(70)
    w = np.ones(69, np.int64)
    with pytest.raises(_lib.HipBackendError, match="2049 nodes"):  # TSIM_ENOTSUP
        hp.uf_create_matching(chain_graph(2049, 3), 2048, np.ones(2048, np.int64), 10)
    zero = w.copy()
    zero[17] = 0
    with pytest.raises(ValueError, match="edge 17 has match weight 0"):  # TSIM_EINVAL
        hp.uf_create_matching(g, 70, zero, 10)
    for K in (13, 0):
        with pytest.raises(ValueError, match="max_defects"):
            hp.uf_create_matching(g, 70, w, K)
    with pytest.raises(ValueError, match="match_weights"):
        hp.uf_create_matching(g, 70, w[:5], 10)
    lib = _lib.load()
    assert lib.tsim_uf_match_table(None, None, None) == -22
    h = hp.uf_create_matching(g, 70, w, 10)
    plain = hp.uf_create(g, 70)
    d = hp.malloc(4096)
    try:
        with pytest.raises(ValueError, match="no soft outputs"):
            hp.uf_decode_soft_device(h, d.ptr, 1, 16, (69, 70), d.ptr + 1024, "rounds", 8, d.ptr + 2048)
        buf = (C.c_uint64 * (70 * 70))()
        assert lib.tsim_uf_match_table(C.c_void_p(plain), buf, buf) == -22 and b"no match table" in lib.tsim_last_error()
        assert hp.uf_info(h)["launches"] == 0
    finally:
        hp.uf_destroy(h)
        hp.uf_destroy(plain)
        d.free()
