"""The union-find decoder on the GPU (``tsim_uf_*``, ``csrc/tsim_uf.hip.h``): predictions and counters bit for bit against the
numpy statement (``tsim_amd.decode.UnionFindDecoder``), the masks, accumulation, ``count(decoder=uf)`` against the host tally
of the same seeded ``sample()``, and what ``tsim_uf_create`` refuses."""

import types

import numpy as np
import pytest

from test_unionfind import chain_graph, memory, no_boundary_graph, wide_observable_graph

from tsim_amd import _lib, faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import UnionFindDecoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def packed(bits: np.ndarray, row_bytes: int, rng) -> np.ndarray:
    """bool ``[n, n_cols]`` -> ``uint8[n, row_bytes]`` little-endian; the pad bits and padding bytes are random."""
    n, n_cols = bits.shape
    full = rng.integers(0, 2, size=(n, 8 * row_bytes), dtype=np.uint8)
    full[:, :n_cols] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little"))


def host_statement(uf, bits, xor=None, test=None):
    """``(predictions uint64[n], (kept, wrong, missed))`` of bool rows (detectors, then observables) by the numpy statement."""
    nd, n_obs = uf.num_detectors, uf.num_observables
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    pred = np.where(keep, uf.predictions(b[:, :nd]), np.uint64(0))
    miss = keep & uf.missed(b[:, :nd])
    obs = (b[:, nd:nd + n_obs].astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    return pred, (int(keep.sum()), int((keep & (pred != obs)).sum()), int(miss.sum()))


def on_device(hp, uf, bits, row_bytes, rng, xor=None, test=None, offset=0):
    """The same from ``tsim_uf_decode_device`` over the bit-packed rows, ``offset`` bytes into their buffer."""
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
        return uf.decode_device(hp, bufs[0].ptr + offset, n, row_bytes, n_cols=n_cols, **masks)
    finally:
        for b in bufs:
            b.free()


def surface_rows(d, rounds, p, n):
    c = memory(d, p, rounds)
    form = c.compile_faults()
    return UnionFindDecoder.from_circuit(c), faults.fault_rows_host(form, 0, n, (1, 2)).view(np.bool_)


@pytest.mark.parametrize("d,rounds,p,n,row_bytes,offset", [(3, 3, 0.02, 4096 + 37, 5, 3), (5, 5, 0.01, 2048, 16, 0)])
def test_surface_code_rows_bit_for_bit(hp, d, rounds, p, n, row_bytes, offset):
    """d = 3: clusters merge and reach the boundary, rows of 5 bytes at an odd address, a row count that is no multiple of 64
    or of a block's shots.  d = 5: 121 columns in aligned 16-byte rows (the 8-byte loads)."""
    uf, bits = surface_rows(d, rounds, p, n)
    want_pred, want = host_statement(uf, bits)
    assert want[0] == n and want[1] > 0 and uf.growth_rounds(bits[:, :uf.num_detectors]).max() >= (2 if d == 3 else 4)
    pred, got = on_device(hp, uf, bits, row_bytes, np.random.default_rng(d), offset=offset)
    print(f"d = {d}: host {want}, device {got}, rows that differ {int((pred != want_pred).sum())}")
    assert np.array_equal(pred, want_pred)
    assert got == want


def random_syndromes(rng, n, nd, n_obs, weight):
    bits = np.zeros((n, nd + n_obs), np.bool_)
    for r in range(n):
        bits[r, rng.choice(nd, size=int(rng.integers(0, weight + 1)), replace=False)] = True
    bits[:, nd:] = rng.integers(0, 2, size=(n, n_obs)).astype(np.bool_)
    return bits


@pytest.mark.parametrize("name", ["chain", "no_boundary", "wide_observables"])
def test_hand_made_graphs_bit_for_bit(hp, name):
    rng = np.random.default_rng(11)
    if name == "chain":  # indices beyond 64, up to 116 growth rounds, levels in the dozens
        uf = UnionFindDecoder(chain_graph())
        bits = random_syndromes(rng, 120, 69, 1, 4)
        bits[:3] = False
        bits[0, [29, 49]] = bits[1, [44, 64]] = bits[2, [4, 67]] = True
    elif name == "no_boundary":  # the miss path
        uf = UnionFindDecoder(no_boundary_graph())
        bits = rng.integers(0, 2, size=(200, 5)).astype(np.bool_)
    else:  # three observables, bit 63 among them
        uf = UnionFindDecoder(wide_observable_graph(), 64)
        bits = random_syndromes(rng, 200, 9, 64, 5)
    want_pred, want = host_statement(uf, bits)
    if name == "no_boundary":
        assert want[2] > 50
    if name == "wide_observables":
        assert (want_pred >> np.uint64(63)).any()
    pred, got = on_device(hp, uf, bits, (bits.shape[1] + 7) // 8 + 1, rng)
    assert np.array_equal(pred, want_pred)
    assert got == want


def test_masks(hp):
    """``d_xor`` and ``d_test``: the kept count and the predictions of the kept rows match the host, rows not kept give 0."""
    uf, bits = surface_rows(3, 3, 0.02, 1500)
    rng = np.random.default_rng(5)
    n_cols = bits.shape[1]
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, np.bool_)
    test[[1, 7, 16]] = True
    want_pred, want = host_statement(uf, bits, xor, test)
    assert 0 < want[0] < len(bits) and want[1] > 0
    pred, got = on_device(hp, uf, bits, 8, rng, xor=xor, test=test)
    assert np.array_equal(pred, want_pred) and got == want
    keep = ~((bits ^ xor) & test).any(axis=1)
    assert not pred[~keep].any() and pred[keep].any()


def test_two_calls_accumulate_and_info(hp):
    uf, bits = surface_rows(3, 3, 0.02, 1000)
    rng = np.random.default_rng(6)
    rows = packed(bits, 4, rng)
    _, want = host_statement(uf, bits)
    nd = uf.num_detectors
    h = hp.uf_create(uf.graph, nd + 1)
    d_rows, d_cnt = hp.malloc(rows.nbytes), hp.malloc(64)
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, np.array([5, 0, 0], np.uint64))
        for _ in range(2):
            hp.uf_decode_device(h, d_rows.ptr, len(rows), 4, (nd, nd + 1), d_cnt.ptr)
        hp.uf_decode_device(h, d_rows.ptr, 0, 4, (nd, nd + 1), d_cnt.ptr)  # no rows: no launch
        info = hp.uf_info(h)
        cnt = np.zeros(3, np.uint64)
        hp.d2h(cnt, d_cnt)
        assert cnt.tolist() == [5 + 2 * want[0], 2 * want[1], 2 * want[2]]
        assert (info["n_nodes"], info["n_edges"], info["launches"], info["n_cols"]) == (25, 78, 2, 25)
        assert info["max_rounds"] == int(uf.growth_rounds(bits[:, :nd]).max())
        assert info["rows_decoded"] == 2 * int(bits[:, :nd].any(axis=1).sum())
        assert 1 <= info["shots_per_block"] <= 4 and info["lds_bytes_per_shot"] < 1024
        for bad in (dict(row_bytes=3), dict(observables=(nd, nd + 2)), dict(d_counters=0)):
            kw = dict(row_bytes=4, observables=(nd, nd + 1), d_counters=d_cnt.ptr)
            kw.update(bad)
            with pytest.raises(ValueError):
                hp.uf_decode_device(h, d_rows.ptr, len(rows), kw["row_bytes"], kw["observables"], kw["d_counters"])
        assert hp.uf_info(h)["launches"] == 2
    finally:
        hp.uf_destroy(h)
        d_rows.free()
        d_cnt.free()


@pytest.mark.parametrize("method", ["faults", "autoregressive"])
def test_count_equals_the_host_tally_of_the_same_sample(hip, method):
    c = memory(3, 0.01, 3)
    uf = UnionFindDecoder.from_circuit(c)
    nd = uf.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[0, 13]] = True
    kw = dict(method=method) if method == "faults" else {}
    rows = c.compile_detector_sampler(seed=21, **kw).sample(4096, append_observables=True)
    got = c.compile_detector_sampler(seed=21, **kw).count(4096, decoder=uf, postselection_mask=mask)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, decoder=uf, histogram_columns=(nd,))
    assert got == want
    assert 0 < got.kept < 4096 and 0 < got.decoded_errors < got.kept_with_observable_flip and got.decoder_misses == 0


def test_create_refusals(hp):
    def graph(n_nodes, u, v):
        return types.SimpleNamespace(n_nodes=n_nodes, edge_u=np.asarray(u, np.int32), edge_v=np.asarray(v, np.int32),
                                     edge_obs=np.zeros(len(u), np.uint64))

    with pytest.raises(ValueError, match="leaves the nodes"):
        hp.uf_create(graph(4, [0, 1], [1, 4]), 4)
    with pytest.raises(ValueError, match="strictly ascending"):
        hp.uf_create(graph(4, [0, 0], [2, 1]), 4)
    u = np.arange(19999)
    with pytest.raises(_lib.HipBackendError, match="bytes of LDS"):
        hp.uf_create(graph(20000, u, u + 1), 20000)
