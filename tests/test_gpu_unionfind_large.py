"""The union-find decoder on the GPU at the sizes it is advertised for (``k_uf<false>`` / ``k_uf<true>``, ``csrc/tsim_uf.hip.h``):
the cases of ``test_unionfind_large.py`` (d = 9, d = 15, 65535 edges, a shot that fills a block's LDS, 1 .. 4 waves a block,
a chain of 1500 nodes), masks on wide rows, a grid that wraps, the refusal next to the largest graph, a call cut into two
launches and ``count(decoder=uf)`` at d = 9.  Every comparison is over all rows and bit for bit against the numpy statement
(``tsim_amd.decode.UnionFindDecoder``): predictions with ``np.array_equal``, the counters with ``==``."""

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, on_device, packed
from test_unionfind import memory
from test_unionfind_large import (CASES, SHOTS_PER_BLOCK, case, decoders, fits_graph, fits_weighted_graph, random_caps, shot_bytes)

from tsim_amd import _lib, faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodingGraph, UnionFindDecoder

pytestmark = pytest.mark.gpu

assert set(SHOTS_PER_BLOCK.values()) == {1, 2, 3, 4}  # every number of waves a block can have launches below


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def decode_rows(hp, uf, rows, n_cols, offset=0):
    """``(predictions uint64[n], (kept, wrong, missed), tsim_uf_info after the call)`` of bit-packed rows ``uint8[n, row_bytes]``
    put ``offset`` bytes into their buffer, by one handle."""
    n, row_bytes = rows.shape
    nd = uf.num_detectors
    pred, cnt = np.zeros(n, np.uint64), np.zeros(3, np.uint64)
    h = hp.uf_create(uf.graph, n_cols, uf.edge_caps)
    bufs = []
    try:
        bufs += [hp.malloc(rows.nbytes + 64), hp.malloc(pred.nbytes + 16), hp.malloc(64)]
        d_rows, d_pred, d_cnt = bufs
        hp.h2d(d_rows.ptr + offset, rows)
        hp.h2d(d_cnt, cnt)
        assert hp.uf_info(h)["launches"] == 0
        hp.uf_decode_device(h, d_rows.ptr + offset, n, row_bytes, (nd, nd + uf.num_observables), d_cnt.ptr, d_pred=d_pred.ptr)
        info = hp.uf_info(h)  # (waits for the decode)
        hp.d2h(pred, d_pred)
        hp.d2h(cnt, d_cnt)
        return pred, tuple(int(x) for x in cnt), info
    finally:
        hp.uf_destroy(h)
        for b in bufs:
            b.free()


def layouts(name, n_cols):
    """``(row_bytes, offset)``: 8-byte loads (rows and address multiples of 8) and the byte path at an odd address."""
    used = (n_cols + 7) // 8
    if name in ("d9", "d15"):
        assert used % 8 and used == {"d9": 91, "d15": 421}[name]
        return [((used + 7) // 8 * 8, 0), (used, 3)]
    return [(used + 1, 5)] if name in ("dense", "chain1500") else [((used + 7) // 8 * 8 + 8, 0)]


@pytest.mark.parametrize("name,weighted", [(name, w) for name in CASES for w in (False, True) if (name, w) in SHOTS_PER_BLOCK])
def test_large_cases_bit_for_bit(hp, name, weighted):
    c = case(name)
    uf = dict(decoders(c))[weighted]
    nd = uf.num_detectors
    want_pred, want = host_statement(uf, c.bits)
    rounds = int(uf.growth_rounds(c.bits[:, :nd]).max())
    for row_bytes, offset in layouts(name, c.bits.shape[1]):
        rows = packed(c.bits, row_bytes, np.random.default_rng(row_bytes))
        pred, got, info = decode_rows(hp, uf, rows, c.bits.shape[1], offset)
        print(f"{name} weighted={weighted} rows of {row_bytes} bytes at +{offset}: host {want}, device {got}, rows that differ "
              f"{int((pred != want_pred).sum())}, growth rounds {info['max_rounds']} (host {rounds}), "
              f"{info['lds_bytes_per_shot']} bytes a shot, {info['shots_per_block']} shots a block, {info['grid_blocks']} blocks")
        assert np.array_equal(pred, want_pred)
        assert got == want
        assert info["max_rounds"] == rounds
        assert info["lds_bytes_per_shot"] == shot_bytes(uf)
        assert info["shots_per_block"] == SHOTS_PER_BLOCK[name, weighted]
        assert info["rows_decoded"] == int(c.bits[:, :nd].any(axis=1).sum()) and info["launches"] == 1


def test_masks_on_wide_rows(hp):
    """d = 9, 91-byte rows: ``d_xor`` over every byte of the row, ``d_test`` in the first word, beyond column 64 and on the
    last detector."""
    c = case("d9")
    rng = np.random.default_rng(9)
    n_cols = c.bits.shape[1]
    xor = rng.random(n_cols) < 0.05
    test = np.zeros(n_cols, np.bool_)
    test[[3, 40, 77, 400, 719]] = True
    keep = ~((c.bits ^ xor) & test).any(axis=1)
    for uf in (c.plain, c.weighted):
        want_pred, want = host_statement(uf, c.bits, xor, test)
        assert want[0] == int(keep.sum()) and 0 < want[0] < len(c.bits)
        for row_bytes, offset in layouts("d9", n_cols):
            pred, got = on_device(hp, uf, c.bits, row_bytes, rng, xor=xor, test=test, offset=offset)
            assert np.array_equal(pred, want_pred) and got == want
            assert 0 < got[0] < len(c.bits) and not pred[~keep].any() and pred[keep].any()


@pytest.mark.parametrize("d,p,base_rows", [(3, 0.02, 4096 + 37), (15, 1e-3, 48)])
def test_persistent_grid_wraps(hp, d, p, base_rows):
    """More tiles than the grid has waves, twice over and a ragged end: every wave takes a second and a third tile and carries
    its counters across them.  The rows are a base of seeded rows, repeated; the host decodes the base.  Neither base is a whole
    number of tiles, so the tiles of one wave differ from each other: a wave that read an earlier tile again would show."""
    circuit = memory(d, p)
    form = circuit.compile_faults()
    uf = UnionFindDecoder.from_circuit(circuit)
    nd, n_cols = uf.num_detectors, uf.num_detectors + 1
    h = hp.uf_create(uf.graph, n_cols)
    try:
        info = hp.uf_info(h)
    finally:
        hp.uf_destroy(h)
    assert info["shots_per_block"] == (4 if d == 3 else 1)
    n = info["grid_blocks"] * info["shots_per_block"] * 64 * 2 + 64 * 3 + 5
    base = faults.fault_rows_host(form, 0, base_rows, (1, 2)).view(np.bool_)
    base_pred, base_cnt = host_statement(uf, base)
    assert base_cnt[0] == base_rows and n > 3 * base_rows and base_rows % 64
    assert (info["grid_blocks"] * info["shots_per_block"] * 64) % base_rows  # (a wave's next tile is not the same rows again)
    row_bytes = (n_cols + 7) // 8 * 8 if d == 15 else (n_cols + 7) // 8
    rows = np.resize(packed(base, row_bytes, np.random.default_rng(d)), (n, row_bytes))
    obs = base[:, nd].astype(np.uint64)
    want = (n, int(np.resize(base_pred != obs, n).sum()), int(np.resize(uf.missed(base[:, :nd]), n).sum()))
    pred, got, info = decode_rows(hp, uf, rows, n_cols)
    print(f"d = {d}: {n} rows on {info['grid_blocks']} blocks of {info['shots_per_block']} waves: host {want}, device {got}")
    assert np.array_equal(pred, np.resize(base_pred, n))
    assert got == want and (want[1] > 0 or d == 15)
    assert info["rows_decoded"] == int(np.resize(base[:, :nd].any(axis=1), n).sum()) > 0
    assert info["max_rounds"] == int(uf.growth_rounds(base[:, :nd]).max()) and info["launches"] == 1


def test_one_more_node_than_the_largest_graph_is_refused(hp):
    """``fits`` and ``fits_weighted`` decode (above); the same graphs with one more node are refused when the handle is made."""
    for graph, caps in ((fits_graph(extra_nodes=1), None), (fits_weighted_graph(extra_nodes=1), True)):
        with pytest.raises(_lib.HipBackendError, match="bytes of LDS"):
            hp.uf_create(graph, graph.n_nodes + 1, random_caps(graph, 44) if caps else None)


def test_a_call_cut_into_two_launches(hp):
    """2^30 + 200 rows of one byte: the second launch starts at row 2^30 and adds to the same counters.  The graph is the edge
    (0, 1) flipping observable 0: a row 0b01 (defect, observable 0) is decoded wrongly, 0b11 rightly, 0 has no defect.  All
    rows are 0 but the last 264, which straddle the seam; only a second launch can count the last 200."""
    uf = UnionFindDecoder(DecodingGraph(2, [0], [1], np.array([1], np.uint64)))
    n, tail_rows = (1 << 30) + 200, 264
    rng = np.random.default_rng(30)
    tail = np.zeros(tail_rows, np.uint8)
    order = rng.permutation(tail_rows)
    tail[order[:132]], tail[order[132:200]] = 0b01, 0b11
    tail |= (rng.integers(0, 64, size=tail_rows) << 2).astype(np.uint8)  # pad bits
    assert (tail[:64] & 3 == 1).any() and (tail[64:] & 3 == 1).any()
    rows = np.zeros(n, np.uint8)
    rows[-tail_rows:] = tail
    h = hp.uf_create(uf.graph, 2)
    bufs = []
    try:
        bufs += [hp.malloc(n), hp.malloc(64), hp.malloc(8 * tail_rows)]
        d_rows, d_cnt, d_pred = bufs
        hp.h2d(d_rows, rows)
        del rows
        hp.h2d(d_cnt, np.zeros(3, np.uint64))
        hp.uf_decode_device(h, d_rows.ptr, n, 1, (1, 2), d_cnt.ptr)  # (no predictions: counters only)
        info = hp.uf_info(h)
        cnt = np.zeros(3, np.uint64)
        hp.d2h(cnt, d_cnt)
        assert cnt.tolist() == [n, 132, 0]
        rounds = int(uf.growth_rounds((tail & 1).astype(np.bool_)[:, None]).max())
        assert info["launches"] == 2 and info["rows_decoded"] == 200 and info["max_rounds"] == rounds > 0
        # the same bytes around the seam as a small call of their own, with predictions
        hp.h2d(d_cnt, np.zeros(3, np.uint64))
        hp.uf_decode_device(h, d_rows.ptr + (n - tail_rows), tail_rows, 1, (1, 2), d_cnt.ptr, d_pred=d_pred.ptr)
        assert hp.uf_info(h)["launches"] == 3
        pred = np.zeros(tail_rows, np.uint64)
        hp.d2h(pred, d_pred)
        hp.d2h(cnt, d_cnt)
        assert np.array_equal(pred, (tail & 1).astype(np.uint64)) and cnt.tolist() == [tail_rows, 132, 0]
    finally:
        hp.uf_destroy(h)
        for b in bufs:
            b.free()


def test_count_at_d9_equals_the_host_tally_of_the_same_sample(hip):
    c = memory(9, 1e-3)
    uf = UnionFindDecoder.from_circuit(c, weights="probability")
    nd = uf.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[5, 300]] = True
    rows = c.compile_detector_sampler(seed=21, method="faults").sample(1024, append_observables=True)
    got = c.compile_detector_sampler(seed=21, method="faults").count(1024, decoder=uf, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=uf, histogram_columns=(nd,))
    assert got == want
    assert 0 < got.kept < 1024 and got.kept == int((~(rows[:, :nd] & mask).any(axis=1)).sum())
