"""Erasure-aware union-find decoding on the GPU (``tsim_uf_create_heralds``, ``k_uf<Weighted, true>`` of ``csrc/tsim_uf.hip.h``):
every prediction, the three counters, the most growth rounds and the rows decoded in LDS bit for bit against the numpy
statement (``tsim_amd.decode.UnionFindDecoder`` over a graph with heralds), on the heralded d = 3 surface code, a chain with
hand-made heralds, a graph of 65535 edges, through ``count(decoder=uf)``, and what the entry refuses."""

import types

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_unionfind import chain_graph
from test_unionfind_erasure import erasure_memory
from test_unionfind_large import dense_graph, random_caps

from tsim_amd import faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodingGraph, UnionFindDecoder, uf_shot_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def decode_rows(hp, uf, bits, row_bytes, offset=0, xor=None, test=None, seed=0):
    """``(predictions uint64[n], (kept, wrong, missed), tsim_uf_info after the call)`` of bool rows (detectors, observables),
    bit-packed to ``row_bytes`` with random padding and put ``offset`` bytes into their buffer, by one handle."""
    n, n_cols = bits.shape
    nd = uf.num_detectors
    rows = packed(bits, row_bytes, np.random.default_rng(seed))
    pred, cnt = np.zeros(n, np.uint64), np.zeros(3, np.uint64)
    h = hp.uf_create(uf.graph, n_cols, uf.edge_caps)
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
        hp.uf_decode_device(h, d_rows.ptr + offset, n, row_bytes, (nd, nd + uf.num_observables), d_cnt.ptr, d_pred=d_pred.ptr, **masks)
        info = hp.uf_info(h)  # (waits for the decode)
        hp.d2h(pred, d_pred)
        hp.d2h(cnt, d_cnt)
        return pred, tuple(int(x) for x in cnt), info
    finally:
        hp.uf_destroy(h)
        for b in bufs:
            b.free()


def check(hp, uf, bits, row_bytes, offset=0, xor=None, test=None):
    """One call on the device against the statement: predictions, counters, growth rounds, rows decoded in LDS.  Returns the
    statement's ``(predictions, counters)`` and the handle's info."""
    g, nd = uf.graph, uf.num_detectors
    want_pred, want = host_statement(uf, bits, xor, test)
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    work = keep & b[:, g.node_det].any(axis=1)   # kept rows with a real defect
    rounds = int(uf.growth_rounds(b[work, :nd]).max()) if work.any() else 0
    pred, got, info = decode_rows(hp, uf, bits, row_bytes, offset, xor, test)
    print(f"rows of {row_bytes} bytes at +{offset}: host {want}, device {got}, rows that differ {int((pred != want_pred).sum())}, growth "
          f"rounds {info['max_rounds']} (host {rounds}), rows decoded {info['rows_decoded']} (host {int(work.sum())})")
    assert np.array_equal(pred, want_pred)
    assert got == want
    assert info["max_rounds"] == rounds and info["rows_decoded"] == int(work.sum()) and info["launches"] == 1
    assert (info["n_heralds"], info["n_det_cols"], info["n_nodes"], info["n_edges"]) == (g.n_heralds, nd, g.n_nodes, g.n_edges)
    assert info["lds_bytes_per_shot"] == uf_shot_bytes(g.n_nodes, g.n_edges, uf.edge_caps is not None)   # (heralds add no state)
    return (want_pred, want), info


# ---- d = 3, 3 rounds: 25 nodes, 144 heralds ---------------------------------------------------------------------------------

_D3: dict = {}


def d3_rows():
    if not _D3:
        c = erasure_memory(3, 3, pe=0.05)
        form = c.compile_faults()
        _D3["c"] = (form, faults.fault_rows_host(form, 0, 512, (1, 2)).view(np.bool_), {})
    return _D3["c"]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("row_bytes,offset", [(22, 3), (24, 0)])
def test_d3_heralded_rows_bit_for_bit(hp, weighted, row_bytes, offset):
    """169 columns, most rows with several heralds; 512 rows are 8 tiles, so the 4 waves of a block each decode on their own
    state.  Rows of 22 bytes at an odd address (the byte path) and of 24 bytes aligned (the 8-byte loads)."""
    form, bits, decoders = d3_rows()
    if weighted not in decoders:
        g = DecodingGraph.from_form(form, heralds=True)
        decoders[weighted] = UnionFindDecoder(g, 1, g.growth_caps(4) if weighted else None)
    uf = decoders[weighted]
    g = uf.graph
    assert (g.n_nodes, g.n_heralds, uf.num_detectors, bits.shape) == (25, 144, 168, (512, 169))
    assert np.median(bits[:, g.herald_det].sum(axis=1)) >= 4
    (_, want), info = check(hp, uf, bits, row_bytes, offset)
    assert want[0] == 512 and want[1] > 0 and info["shots_per_block"] == 4
    for t in range(info["shots_per_block"]):   # every wave of the first block decodes
        assert bits[64 * t:64 * t + 64, g.node_det].any()


# ---- a chain with hand-made heralds ----------------------------------------------------------------------------------------

HERALD_COLS = [2, 5, 66, 67, 70, 73, 75, 76]
HERALD_LISTS = [[],                      # an empty list
                [3, 4], [10, 20],        # two heralds in one 32-bit word of `full`: the word is listed once
                [40, 41], [41, 42],      # two heralds list edge 41
                [68],                    # the last edge, in the last word
                list(range(30, 50)),     # a run over two words, the observable edge 40 in it
                [0]]


def toy_chain(weighted: bool) -> UnionFindDecoder:
    """0 - 1 - ... - 69 with 8 heralds: 77 detector columns, the heralds among the node columns and beyond column 64."""
    base = chain_graph()
    g = DecodingGraph(70, base.edge_u, base.edge_v, base.edge_obs, node_det=np.setdiff1d(np.arange(77), HERALD_COLS),
                      herald_det=HERALD_COLS, herald_ptr=np.cumsum([0] + [len(x) for x in HERALD_LISTS]),
                      herald_edges=[e for x in HERALD_LISTS for e in x])
    return UnionFindDecoder(g, edge_caps=np.resize([3, 1, 8, 2, 5], 69) if weighted else None)


def toy_rows(uf, n=192, seed=12):
    rng = np.random.default_rng(seed)
    g = uf.graph
    bits = np.zeros((n, 78), np.bool_)
    for r in range(n):
        bits[r, rng.choice(g.node_det, size=int(rng.integers(0, 5)), replace=False)] = True
    bits[:, HERALD_COLS] = rng.random((n, 8)) < 0.3
    bits[:, 77] = rng.integers(0, 2, size=n).astype(np.bool_)
    # by hand: defects far apart that an erased run joins; both heralds of edge 41; the heralds of one word; heralds only
    bits[:6] = False
    bits[0, [g.node_det[29], g.node_det[49], 75]] = True
    bits[1, [g.node_det[39], g.node_det[42], 67, 70]] = True
    bits[2, [g.node_det[2], g.node_det[20], 5, 66]] = True
    bits[3, HERALD_COLS] = True
    bits[4, [g.node_det[68], 73, 2]] = True
    bits[5, [g.node_det[0], 76]] = True
    return bits


@pytest.mark.parametrize("weighted", [False, True])
def test_toy_chain_bit_for_bit(hp, weighted):
    uf = toy_chain(weighted)
    bits = toy_rows(uf)
    nodes = uf.graph.node_det
    assert uf.growth_rounds(bits[:1, :77])[0] == 0 and UnionFindDecoder(chain_graph()).growth_rounds(bits[:1, nodes])[0] > 0
    only_heralds = ~bits[:, nodes].any(axis=1) & bits[:, HERALD_COLS].any(axis=1)
    assert only_heralds[3] and only_heralds.sum() >= 3
    (pred, want), _ = check(hp, uf, bits, 11, 1)
    assert want[0] == len(bits) and want[1] > 0 and not pred[only_heralds].any()
    check(hp, uf, bits, 16, 0)


def test_rows_with_heralds_only_are_not_decoded(hp):
    uf = toy_chain(False)
    bits = np.zeros((130, 78), np.bool_)
    bits[:, HERALD_COLS] = np.random.default_rng(4).random((130, 8)) < 0.5
    bits[::3, 77] = True
    assert bits[:, HERALD_COLS].any(axis=1).sum() > 100
    (pred, want), info = check(hp, uf, bits, 10)
    assert info["rows_decoded"] == 0 and info["max_rounds"] == 0 and not pred.any() and want == (130, 44, 0)


@pytest.mark.parametrize("weighted", [False, True])
def test_toy_chain_masks(hp, weighted):
    """An xor mask that flips a herald column (75), a node column and the observable; a test mask on the herald column 70, which
    discards the shots erased there, and on a node column."""
    uf = toy_chain(weighted)
    bits = toy_rows(uf, seed=13)
    xor, test = np.zeros(78, np.bool_), np.zeros(78, np.bool_)
    xor[[75, uf.graph.node_det[11], 77]] = True
    test[[70, uf.graph.node_det[50]]] = True
    (pred, want), _ = check(hp, uf, bits, 10, 3, xor=xor, test=test)
    erased = bits[:, 70]
    assert want[0] == int((~erased & ~bits[:, uf.graph.node_det[50]]).sum()) and 0 < want[0] < len(bits) and not pred[erased].any()
    # (on a chain the correction is unique, so the pre-grown edges show in the growth rounds:) the flipped herald column joins
    # the defects of these rows before the first round; without that bit of the mask they grow towards each other
    pair = np.zeros((70, 78), np.bool_)
    pair[:, [uf.graph.node_det[29], uf.graph.node_det[49]]] = True
    pair[:, uf.graph.node_det[11]] = True   # (flipped back by the mask)
    pair[::2, 77] = True
    _, info = check(hp, uf, pair, 16, 0, xor=xor)
    xor[75] = False
    assert info["max_rounds"] == 0 and info["rows_decoded"] == 70 and uf.growth_rounds((pair ^ xor)[:1, :77])[0] > 0


# ---- 400 nodes, 65535 edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
def test_dense_graph_first_and_last_words(hp, weighted):
    """Heralds on edge 0, 32767, 32768 and 65534 (``herald_edges`` beyond int16, the first and the last word of the bitmap) and
    one that erases every edge: a row with it takes no growth round."""
    base = dense_graph()
    cols = [0, 100, 200, 300, 403]
    lists = [[0], [32767], [32768], [65534], list(range(65535))]
    g = DecodingGraph(400, base.edge_u, base.edge_v, base.edge_obs, node_det=np.setdiff1d(np.arange(404), cols), herald_det=cols,
                      herald_ptr=np.cumsum([0] + [len(x) for x in lists]), herald_edges=[e for x in lists for e in x])
    uf = UnionFindDecoder(g, 2, random_caps(g, 32) if weighted else None)
    rng = np.random.default_rng(65)
    bits = np.zeros((20, 406), np.bool_)
    for r in range(20):
        bits[r, rng.choice(g.node_det, size=int(rng.integers(1, 30)), replace=False)] = True
    bits[:, cols[:4]] = rng.random((20, 4)) < 0.5
    bits[:4, cols[:4]] = np.eye(4, dtype=np.bool_)
    for i, e in enumerate([0, 32767, 32768, 65534]):   # the defects at the ends of the herald's edge: peeling alone
        bits[i, g.node_det] = False
        bits[i, g.node_det[[x - 1 for x in (g.edge_u[e], g.edge_v[e]) if x]]] = True
    bits[:, 404:] = rng.integers(0, 2, size=(20, 2)).astype(np.bool_)
    assert (uf.growth_rounds(bits[:4, :404]) == 0).all() and uf.growth_rounds(bits[4:, :404]).min() >= 1
    check(hp, uf, bits, 51, 1)
    bits[:, 403] = True   # every edge erased
    _, info = check(hp, uf, bits, 56, 0)
    assert info["max_rounds"] == 0 and info["rows_decoded"] == 20


# ---- refusals, on the host --------------------------------------------------------------------------------------------------

def test_create_heralds_refusals(hp):
    def graph(n_det_cols=6, **kw):
        a = dict(node_det=[0, 2, 3, 5], herald_det=[1, 4], herald_ptr=[0, 1, 3], herald_edges=[3, 0, 3])
        a.update(kw)
        u = np.arange(4, dtype=np.int32)
        return types.SimpleNamespace(n_nodes=5, edge_u=u, edge_v=u + 1, edge_obs=np.zeros(4, np.uint64), num_detectors=n_det_cols,
                                     **{k: np.array(v, np.int32) for k, v in a.items()})

    hp.uf_destroy(hp.uf_create(graph(), 7))
    hp.uf_destroy(hp.uf_create(graph(), 6, [1, 2, 3, 14]))
    for kw, n_cols, match in ((dict(herald_det=[1, 3]), 7, "named twice"), (dict(herald_det=[4, 4]), 7, "named twice"),
                              (dict(herald_edges=[3, 0, 4]), 7, "of 4 edges"), (dict(herald_ptr=[0, 2, 1]), 7, "must not fall"),
                              ({}, 5, "n_cols = 5")):
        with pytest.raises(ValueError, match=match):
            hp.uf_create(graph(**kw), n_cols)
        with pytest.raises(ValueError, match=match):
            hp.uf_create(graph(**kw), n_cols, [1, 2, 3, 4])


# ---- count(decoder=uf) ------------------------------------------------------------------------------------------------------

def test_count_equals_the_host_tally_of_the_same_sample(hip, hp):
    c = erasure_memory(3, 3)
    uf = UnionFindDecoder.from_circuit(c, heralds=True)
    nd = uf.num_detectors
    assert nd == 168 and uf.info()["n_heralds"] == 144
    mask = np.zeros(nd, np.bool_)
    mask[[int(uf.graph.herald_det[7]), int(uf.graph.node_det[13])]] = True   # a herald column and a node column
    rows = c.compile_detector_sampler(seed=21, method="faults").sample(20000, append_observables=True)
    got = c.compile_detector_sampler(seed=21, method="faults").count(20000, decoder=uf, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=uf, histogram_columns=(nd,))
    assert got == want
    assert 0 < got.kept < 20000 and 0 < got.decoded_errors < got.kept_with_observable_flip and got.decoder_misses == 0
    h = hp.uf_create(uf.graph, nd + 1)
    try:
        info = hp.uf_info(h)
    finally:
        hp.uf_destroy(h)
    assert (info["n_heralds"], info["n_det_cols"], info["n_nodes"], info["n_cols"]) == (144, 168, 25, 169)
