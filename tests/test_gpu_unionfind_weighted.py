"""Weighted growth of the union-find decoder on the GPU (``tsim_uf_create_weighted``, ``k_uf<true>`` of ``csrc/tsim_uf.hip.h``):
predictions and counters bit for bit against the numpy statement with the same caps, caps of 2 against the unweighted handle,
the masks, accumulation, ``tsim_uf_info`` and ``count(decoder=...)`` against the host tally of the same seeded ``sample()``."""

import itertools

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, on_device, packed, random_syndromes
from test_unionfind import chain_graph, memory, no_boundary_graph, wide_observable_graph

from tsim_amd import faults, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import UnionFindDecoder, uf_shot_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


_ROWS: dict = {}


def surface_rows(d, rounds, p, n):
    """``(circuit, weighted decoder at resolution 4, unweighted decoder, rows)``, built once (the decoders cache syndromes)."""
    if (d, rounds, p, n) not in _ROWS:
        c = memory(d, p, rounds)
        form = c.compile_faults()
        rows = faults.fault_rows_host(form, 0, n, (1, 2)).view(np.bool_)
        _ROWS[d, rounds, p, n] = (c, UnionFindDecoder.from_circuit(c, weights="probability"), UnionFindDecoder.from_circuit(c), rows)
    return _ROWS[d, rounds, p, n]


@pytest.mark.parametrize("d,rounds,p,n,row_bytes,offset", [(3, 3, 0.02, 4096 + 37, 5, 3), (5, 5, 0.01, 2048, 16, 0)])
def test_surface_code_rows_bit_for_bit(hp, d, rounds, p, n, row_bytes, offset):
    _, uf, plain, bits = surface_rows(d, rounds, p, n)
    nd = uf.num_detectors
    want_pred, want = host_statement(uf, bits)
    most, most_plain = int(uf.growth_rounds(bits[:, :nd]).max()), int(plain.growth_rounds(bits[:, :nd]).max())
    assert want[0] == n and want[1] > 0 and want[2] == 0
    assert most > most_plain  # the counters pass 2
    pred, got = on_device(hp, uf, bits, row_bytes, np.random.default_rng(d), offset=offset)
    print(f"d = {d}: host {want}, device {got}, rows that differ {int((pred != want_pred).sum())}, growth rounds at most {most} "
          f"(unweighted {most_plain}, {host_statement(plain, bits)[1][1]} decoded errors)")
    assert np.array_equal(pred, want_pred)
    assert got == want


def light_patterns(nd, n_obs, weight, rng):
    """Every defect pattern of at most ``weight`` defects, then 512 random rows; random observables."""
    sets = [s for k in range(weight + 1) for s in itertools.combinations(range(nd), k)]
    bits = np.zeros((len(sets) + 512, nd + n_obs), np.bool_)
    for r, s in enumerate(sets):
        bits[r, list(s)] = True
    bits[len(sets):, :nd] = rng.random((512, nd)) < rng.random((512, 1))
    bits[:, nd:] = rng.integers(0, 2, size=(len(bits), n_obs)).astype(np.bool_)
    return bits


@pytest.mark.parametrize("name", ["chain75", "chain69", "no_boundary", "wide_observables"])
def test_hand_made_graphs_bit_for_bit(hp, name):
    """chain75: 75 edges, so the borders of the counter words (8 edges) and of the bitmap words (32) fall inside, caps
    1, 14, 3, 8 in turn: every pattern of at most one defect, 512 random rows of up to 4 defects and three pairs that lie far
    apart (all patterns of up to 3 defects would be 70376 rows and minutes of the numpy statement).  The small graphs: every
    pattern of at most 3 defects and 512 random rows."""
    rng = np.random.default_rng(12)
    if name.startswith("chain"):
        n_edges = int(name[5:])
        caps = np.resize([1, 14, 3, 8], n_edges) if n_edges == 75 else rng.integers(1, 15, size=n_edges)
        uf = UnionFindDecoder(chain_graph(n_edges + 1), edge_caps=caps)
        bits = np.concatenate([light_patterns(n_edges, 1, 1, rng)[:n_edges + 1], random_syndromes(rng, 512, n_edges, 1, 4)])
        bits[-3:] = False
        bits[-3, [29, 49]] = bits[-2, [44, 64]] = bits[-1, [4, 67]] = True
        assert n_edges % 8 and n_edges % 32
    elif name == "no_boundary":  # the miss path
        uf = UnionFindDecoder(no_boundary_graph(), edge_caps=[3, 14])
        bits = light_patterns(3, 2, 3, rng)
    else:  # three observables, bit 63 among them; 12 edges
        uf = UnionFindDecoder(wide_observable_graph(), 64, edge_caps=rng.integers(1, 15, size=12))
        bits = light_patterns(9, 64, 3, rng)
    want_pred, want = host_statement(uf, bits)
    if name == "no_boundary":
        assert want[2] > 100
    else:
        assert want[2] == 0
    if name == "wide_observables":
        assert (want_pred >> np.uint64(63)).any()
    pred, got = on_device(hp, uf, bits, (bits.shape[1] + 7) // 8 + 1, rng)
    print(f"{name}: host {want}, device {got}, growth rounds at most {int(uf.growth_rounds(bits[:, :uf.num_detectors]).max())}")
    assert np.array_equal(pred, want_pred)
    assert got == want


def test_caps_of_two_equal_the_unweighted_handle(hp):
    _, _, plain, bits = surface_rows(3, 3, 0.02, 4096 + 37)
    two = UnionFindDecoder(plain.graph, plain.num_observables, edge_caps=np.full(plain.graph.n_edges, 2))
    pred_a, got_a = on_device(hp, plain, bits, 4, np.random.default_rng(8))
    pred_b, got_b = on_device(hp, two, bits, 4, np.random.default_rng(8))
    want_pred, want = host_statement(plain, bits)
    assert np.array_equal(pred_a, pred_b) and got_a == got_b
    assert np.array_equal(pred_b, want_pred) and got_b == want and want[1] > 0


def test_masks(hp):
    _, uf, _, bits = surface_rows(3, 3, 0.02, 4096 + 37)
    bits = bits[:1500]
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
    _, uf, _, bits = surface_rows(3, 3, 0.02, 4096 + 37)
    bits = bits[:1000]
    rows = packed(bits, 4, np.random.default_rng(6))
    _, want = host_statement(uf, bits)
    nd = uf.num_detectors
    h = hp.uf_create(uf.graph, nd + 1, uf.edge_caps)
    h_plain = hp.uf_create(uf.graph, nd + 1)
    d_rows, d_cnt = hp.malloc(rows.nbytes), hp.malloc(64)
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, np.array([5, 0, 0], np.uint64))
        for _ in range(2):
            hp.uf_decode_device(h, d_rows.ptr, len(rows), 4, (nd, nd + 1), d_cnt.ptr)
        info, info_plain = hp.uf_info(h), hp.uf_info(h_plain)
        cnt = np.zeros(3, np.uint64)
        hp.d2h(cnt, d_cnt)
        assert cnt.tolist() == [5 + 2 * want[0], 2 * want[1], 2 * want[2]]
        assert (info["n_nodes"], info["n_edges"], info["launches"], info["n_cols"]) == (25, 78, 2, 25)
        assert info["max_cap"] == int(uf.edge_caps.max()) == 8 and info_plain["max_cap"] == 0
        assert info["lds_bytes_per_shot"] == uf_shot_bytes(25, 78, True) and info_plain["lds_bytes_per_shot"] == uf_shot_bytes(25, 78, False)
        assert info["lds_bytes_per_shot"] > info_plain["lds_bytes_per_shot"]
        assert info["max_rounds"] == int(uf.growth_rounds(bits[:, :nd]).max())
        assert info["rows_decoded"] == 2 * int(bits[:, :nd].any(axis=1).sum())
        assert 1 <= info["shots_per_block"] <= 4
    finally:
        hp.uf_destroy(h)
        hp.uf_destroy(h_plain)
        d_rows.free()
        d_cnt.free()


def test_count_equals_the_host_tally_of_the_same_sample(hip):
    c = memory(3, 0.01)
    uf = UnionFindDecoder.from_circuit(c, weights="probability")
    nd = uf.num_detectors
    mask = np.zeros(nd, np.bool_)
    mask[[0, 13]] = True
    rows = c.compile_detector_sampler(seed=5, method="faults").sample(20000, append_observables=True)
    for kw in ({}, dict(postselection_mask=mask)):
        got = c.compile_detector_sampler(seed=5, method="faults").count(20000, decoder=uf, **kw)
        want = tally_rows(rows, num_detectors=nd, decoder=uf, histogram_columns=(nd,), **kw)
        assert (got.kept, got.decoded_errors, got.decoder_misses) == (want.kept, want.decoded_errors, want.decoder_misses)
        assert got == want
        assert 0 < got.decoded_errors < got.kept_with_observable_flip and got.decoder_misses == 0
        assert (got.kept < 20000) == bool(kw)
