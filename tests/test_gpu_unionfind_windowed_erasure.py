"""Sliding-window union-find decoding with heralded erasures on the GPU (``tsim_ufw_create_heralds``, ``k_ufw<Weighted, true>`` of
``csrc/tsim_ufw.hip.h``): every prediction, the three counters and what ``tsim_ufw_info`` counts, bit for bit against the numpy
statement (``tsim_amd.decode.WindowedUnionFindDecoder(..., heralds=True)``), whose windows and herald lists the library builds a
second time by itself; rows are packed by numpy and uploaded."""

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, on_device, packed
from test_unionfind_windowed import fire
from test_unionfind_windowed_erasure import LADDER_HERALD_COLS, erasure_memory, herald_ladder

from tsim_amd import faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def windows_decoded(w, dets) -> int:
    """The windows the statement decodes over the rows ``dets`` (none of them a miss): window ``k`` of a row is decoded iff the
    node columns, XOR the ends of the flips committed by the windows before ``k``, have a bit in ``[lo_k, hi_k)``."""
    g, C, K = w.graph, w.commit, len(w.windows())
    low = np.where(g.edge_u > 0, g.edge_u, g.edge_v) - 1
    commit_window = np.minimum(low // C, K - 1)
    total = 0
    for row, flips in zip(dets, w.flipped_edges(dets)):
        r = row[g.node_det].copy()
        if not r.any():
            continue
        for k, x in enumerate(w.windows()):
            total += bool(r[x.lo:x.hi].any())
            for e in flips[commit_window[flips] == k]:
                if g.edge_u[e]:
                    r[g.edge_u[e] - 1] ^= True
                r[g.edge_v[e] - 1] ^= True
    return total


def check(hp, w, bits, row_bytes, offset=0, xor=None, test=None, seed=0):
    """One call on a handle of ``tsim_ufw_create_heralds`` against the statement: predictions, counters, and the handle's info
    after the call.  Returns the statement's ``(predictions, counters)`` and the info."""
    g, nd = w.graph, w.num_detectors
    n, n_cols = bits.shape
    want_pred, want = host_statement(w, bits, xor, test)
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(n, np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    work = keep & b[:, g.node_det].any(axis=1)   # kept rows with a defect on a node column
    assert want[2] == 0
    rounds = int(w.growth_rounds(b[work, :nd]).max()) if work.any() else 0
    rows = packed(bits, row_bytes, np.random.default_rng(seed))
    pred, cnt = np.zeros(n, np.uint64), np.zeros(3, np.uint64)
    h = hp.ufw_create(g, n_cols, w.commit, w.window, w.edge_caps, heralds=True)
    bufs = []
    try:
        bufs += [hp.malloc(rows.nbytes + 64), hp.malloc(pred.nbytes + 16), hp.malloc(64)]
        d_rows, d_pred, d_cnt = bufs
        masks = {}
        for name, m in (("d_xor", xor), ("d_test", test)):
            if m is not None:
                bufs.append(hp.malloc(64 + (n_cols + 7) // 8))
                hp.h2d(bufs[-1], np.packbits(m, bitorder="little"))
                masks[name] = bufs[-1].ptr
        hp.h2d(d_rows.ptr + offset, rows)
        hp.h2d(d_cnt, cnt)
        hp.ufw_decode_device(h, d_rows.ptr + offset, n, row_bytes, (nd, nd + w.num_observables), d_cnt.ptr, d_pred=d_pred.ptr, **masks)
        info = hp.ufw_info(h)  # (waits for the decode)
        hp.d2h(pred, d_pred)
        hp.d2h(cnt, d_cnt)
    finally:
        hp.ufw_destroy(h)
        for x in bufs:
            x.free()
    got = tuple(int(x) for x in cnt)
    decoded = windows_decoded(w, b[work, :nd])
    print(f"rows of {row_bytes} bytes at +{offset}: host {want}, device {got}, rows that differ {int((pred != want_pred).sum())}, growth "
          f"rounds {info['max_rounds']} (host {rounds}), rows decoded {info['rows_decoded']} (host {int(work.sum())}), windows decoded "
          f"{info['windows_decoded']} (host {decoded})")
    assert np.array_equal(pred, want_pred)
    assert got == want
    assert info["max_rounds"] == rounds and info["rows_decoded"] == int(work.sum()) and info["windows_decoded"] == decoded and info["launches"] == 1
    assert (info["n_heralds"], info["n_det_cols"], info["n_nodes"], info["n_edges"], info["n_cols"]) == (g.n_heralds, nd, g.n_nodes, g.n_edges, n_cols)
    assert (info["n_windows"], info["max_window_nodes"], info["max_window_edges"]) == tuple(w.info()[k] for k in ("n_windows", "max_window_nodes", "max_window_edges"))
    return (want_pred, want), info


# ---- d = 3, 12 rounds: 97 nodes, 576 heralds, 5 windows of 32 nodes --------------------------------------------------------

_D3: dict = {}


def d3(weights=None):
    """``(circuit, rows, windowed decoder)``: 320 seeded rows of 673 columns, then 8 all-zero rows and 8 rows with heralds and no
    defect on a node column; commit = 16, window = 32."""
    if "c" not in _D3:
        c = erasure_memory()
        form = c.compile_faults()
        bits = faults.fault_rows_host(form, 0, 320, (1, 2)).view(np.bool_)
        g = UnionFindDecoder.from_circuit(c, heralds=True).graph
        extra = np.zeros((16, bits.shape[1]), np.bool_)
        extra[8:, g.herald_det] = np.random.default_rng(6).random((8, g.n_heralds)) < 0.02
        extra[8:, g.herald_det[:8]] |= np.eye(8, dtype=np.bool_)
        extra[::2, 672] = True
        _D3["c"] = (c, np.concatenate([bits, extra]))
    if weights not in _D3:
        _D3[weights] = WindowedUnionFindDecoder.from_circuit(_D3["c"][0], 16, 32, weights=weights, resolution=4, heralds=True)
    return _D3["c"] + (_D3[weights],)


@pytest.mark.parametrize("weights", [None, "probability"])
@pytest.mark.parametrize("row_bytes,offset", [(85, 3), (88, 0)])
def test_d3_heralded_rows_bit_for_bit(hp, weights, row_bytes, offset):
    """5 windows, a carry bitmap of exactly 32 bits that wraps, about 208 heralds to a window (the herald loop strides more than
    once); weighted: the 4-bit counters stay untouched by the pre-grown edges.  Rows of 85 bytes at an odd address (the byte
    path) and of 88 bytes 8-aligned (the 8-byte loads)."""
    _, bits, w = d3(weights)
    g = w.graph
    assert bits.shape == (336, 673) and w.info()["n_windows"] == 5 and all(len(x.heralds) > 128 for x in w.windows())
    nodes, heralds = bits[:, g.node_det], bits[:, g.herald_det]
    assert int(nodes[:320].any(axis=1).sum()) == 317 and int((~nodes[:320].any(axis=1) & heralds[:320].any(axis=1)).sum()) == 3
    assert int((nodes[:320, 64:].any(axis=1) & ~nodes[:320, :64].any(axis=1)).sum()) == 13
    assert not bits[320:328, :672].any() and not nodes[328:].any() and heralds[328:].any(axis=1).all()
    (pred, want), info = check(hp, w, bits, row_bytes, offset)
    assert want[0] == 336 and 0 < want[1] < 336 and pred.any() and not pred[320:].any()
    assert (pred != w.predictions(bits[:, :672] & ~np.isin(np.arange(672), g.herald_det))).any()   # (the heralds matter)
    assert info["shots_per_block"] >= 2
    for t in range(info["shots_per_block"]):   # every wave of the first block decodes
        assert nodes[64 * t:64 * t + 64].any()


def test_masks_and_a_ragged_row_count(hp):
    """``d_xor`` and ``d_test``, 201 rows (no multiple of 64): an xor bit on a herald column (its site's edges start full in every
    row but those that have the herald) and on a node column, a test bit on a herald column (its erased shots are discarded) and
    on a node column."""
    _, bits, w = d3()
    g = w.graph
    fired = np.flatnonzero(bits[:201, g.herald_det].any(axis=0))
    listed = fired[np.diff(g.herald_ptr)[fired] > 0]
    xor, test = np.zeros(673, np.bool_), np.zeros(673, np.bool_)
    xor[[int(g.herald_det[listed[0]]), int(g.node_det[40]), 672]] = True
    test[[int(g.herald_det[listed[1]]), int(g.node_det[3])]] = True
    (pred, want), _ = check(hp, w, bits[:201], 85, 1, xor=xor, test=test)
    keep = ~((bits[:201] ^ xor) & test).any(axis=1)
    assert 0 < want[0] == int(keep.sum()) < 201 and want[1] > 0 and not pred[~keep].any() and pred[keep].any()
    unmasked, _ = host_statement(w, bits[:201])
    assert (pred[keep] != unmasked[keep]).any()


@pytest.mark.parametrize("weighted", [False, True])
def test_hand_made_ladder_bit_for_bit(hp, weighted):
    """The ladder of the CPU test: a herald across ``hi_0``, a merged pair, a shared edge, an empty list, a herald without an edge
    in a window; 300 fired rows with random heralds."""
    g, caps = herald_ladder()
    w = WindowedUnionFindDecoder(g, 4, 8, edge_caps=caps if weighted else None, heralds=True)
    rng = np.random.default_rng(3)
    bits = np.zeros((300, 19), np.bool_)
    bits[:, g.node_det] = fire(g, rng, 300, 0.08)
    bits[:, LADDER_HERALD_COLS] = rng.random((300, 6)) < 0.3
    bits[:, 18] = rng.integers(0, 2, size=300).astype(np.bool_)
    assert all(bits[:, c].sum() > 50 for c in LADDER_HERALD_COLS)
    blind = bits.copy()
    blind[:, LADDER_HERALD_COLS] = False
    assert (w.predictions(bits[:, :18]) != w.predictions(blind[:, :18])).any() or (w.growth_rounds(bits[:, :18]) != w.growth_rounds(blind[:, :18])).any()
    check(hp, w, bits, 3, 1)
    check(hp, w, bits, 8, 0)


@pytest.mark.parametrize("weights", [None, "probability"])
def test_one_window_equals_the_whole_graph_handle_with_heralds(hp, weights):
    c, bits, _ = d3()
    uf = UnionFindDecoder.from_circuit(c, weights=weights, heralds=True)
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 96, weights=weights, heralds=True)
    assert w.info()["n_windows"] == 1
    rows = packed(bits, 88, np.random.default_rng(8))
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        whole = uf.decode_device(hp, d_rows.ptr, len(rows), 88)
        windowed = w.decode_device(hp, d_rows.ptr, len(rows), 88)
    finally:
        d_rows.free()
    assert np.array_equal(windowed[0], whole[0]) and windowed[1] == whole[1] and whole[0].any()
    assert np.array_equal(whole[0], uf.predictions(bits[:, :672]))


def test_heralds_true_on_a_graph_without_heralds_is_the_plain_handle(hp):
    g, caps = herald_ladder()
    plain = WindowedUnionFindDecoder(DecodingGraph(g.n_nodes, g.edge_u, g.edge_v, g.edge_obs), 4, 8, edge_caps=caps, heralds=True)
    rng = np.random.default_rng(5)
    bits = np.concatenate([fire(plain.graph, rng, 100, 0.08), rng.integers(0, 2, size=(100, 1)).astype(np.bool_)], axis=1)
    want_pred, want = host_statement(plain, bits)
    pred, got = on_device(hp, plain, bits, 2, rng)
    assert np.array_equal(pred, want_pred) and got == want and pred.any()


# ---- count(decoder=wuf) -----------------------------------------------------------------------------------------------------

def test_count_equals_the_host_tally_of_the_same_sample(hip):
    """d = 5, 10 rounds, commit = 48, window = 96: 4 windows of at most 97 nodes and 392 edges, 1600 heralds, 1841 columns."""
    c = erasure_memory(5, 10)
    w = WindowedUnionFindDecoder.from_circuit(c, 48, 96, heralds=True)
    nd = w.num_detectors
    info = w.info()
    assert (nd, info["n_heralds"], info["n_windows"], info["max_window_nodes"], info["max_window_edges"]) == (1840, 1600, 4, 97, 392)
    mask = np.zeros(nd, np.bool_)
    mask[[int(w.graph.herald_det[7]), int(w.graph.node_det[130])]] = True   # a herald column and a node column
    rows = c.compile_detector_sampler(seed=21, method="faults").sample(4096, append_observables=True)
    got = c.compile_detector_sampler(seed=21, method="faults").count(4096, decoder=w, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=w, histogram_columns=(nd,))
    assert got == want
    assert 0 < got.kept < 4096 and 0 < got.decoded_errors < got.kept_with_observable_flip and got.decoder_misses == 0
