"""Cluster matching and the complementary gap under heralded erasures on the GPU (``tsim_uf_create_matching_heralds``:
``k_uf<., true, false, true, Gap, true>`` of ``csrc/tsim_uf.hip.h``): predictions, counters, ``tsim_uf_info``,
``tsim_uf_erasure_info``, deficits and both histograms bit for bit against the numpy statement, the front ends against it, and what
the new calls refuse.  Every graph and row is valid: nothing here asks a kernel for an index its tables do not hold."""

import ctypes as C

import numpy as np
import pytest

from test_gpu_unionfind import host_statement, packed
from test_unionfind_erasure import erasure_memory
from test_unionfind_erasure_matching import INNER_W, inner_chain, long_chain, row_of, with_heralds, without_heralds

from tsim_amd import _lib, shotdata, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodeFileResult, UnionFindDecoder, uf_erasure_shot_bytes, uf_shot_bytes

pytestmark = pytest.mark.gpu

_CASES: dict = {}


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def surface(d: int, rounds: int, p: float, pe: float, n: int, weighted: bool = True):
    """``(circuit, plain herald decoder, n rows bool)`` of a memory experiment with heralded erasures (``method="faults"``, seed 5),
    built once."""
    key = (d, rounds, p, pe, n, weighted)
    if key not in _CASES:
        c = erasure_memory(d, rounds, p, pe)
        uf = UnionFindDecoder.from_circuit(c, weights="probability" if weighted else None, heralds=True)
        rows = c.compile_detector_sampler(seed=5, method="faults").sample(n, append_observables=True).astype(np.bool_)
        rows.setflags(write=False)
        _CASES[key] = (c, uf, rows)
    return _CASES[key]


def statement(ue, bits, xor=None, test=None):
    """``(predictions, (kept, wrong, missed), deficits, kept per bin, errors per bin)`` of bool rows by the numpy statement; the
    last three are ``None`` for a decoder without the gap."""
    nd, n_obs = ue.num_detectors, ue.num_observables
    pred, counts = host_statement(ue, bits, xor, test)
    if ue.gap_observable is None:
        return pred, counts, None, None, None
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    D = np.where(keep, ue.gap_outputs(b[:, :nd]), 0)
    obs = (b[:, nd:nd + n_obs].astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    bins = np.minimum(D // ue.gap_step, ue.soft_bins - 1)
    return (pred, counts, D, np.bincount(bins[keep], minlength=ue.soft_bins), np.bincount(bins[keep & (pred != obs)], minlength=ue.soft_bins))


def cluster_counts(ue, bits, xor=None, test=None):
    """``(matched, peeled, matched with an erased edge, peeled for their hubs)`` over the kept rows, by the numpy statement."""
    b = bits if xor is None else bits ^ xor[None, :]
    keep = np.ones(len(b), np.bool_) if test is None else ~(b & test[None, :]).any(axis=1)
    dets = b[keep][:, :ue.num_detectors]
    return ue.match_counts(dets) + ue.erasure_counts(dets)


def on_device(hp, ue, bits, row_bytes, rng, xor=None, test=None, offset=0):
    """The same from one ``tsim_uf_decode_gap_device`` (``tsim_uf_decode_device`` without the gap) over the bit-packed rows,
    ``offset`` bytes into their buffer, then ``tsim_uf_info`` and ``tsim_uf_erasure_info``."""
    n, n_cols = bits.shape
    nd, gap = ue.num_detectors, ue.gap_observable is not None
    B = ue.soft_bins if gap else 1
    rows = packed(bits, row_bytes, rng)
    pred, cnt, D, hist = np.zeros(n, np.uint64), np.zeros(3, np.uint64), np.zeros(n, np.uint32), np.zeros(2 * B, np.uint64)
    bufs = [hp.malloc(rows.nbytes + 64), hp.malloc(pred.nbytes + 16), hp.malloc(64), hp.malloc(D.nbytes + 16), hp.malloc(hist.nbytes + 16)]
    h, _, destroy = ue._handle(hp, n_cols)
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
        if gap:
            hp.uf_decode_gap_device(h, bufs[0].ptr + offset, n, row_bytes, (nd, nd + ue.num_observables), bufs[2].ptr, ue.gap_cap, ue.gap_step, B,
                                    bufs[4].ptr, d_gap=bufs[3].ptr, d_pred=bufs[1].ptr, **masks)
        else:
            hp.uf_decode_device(h, bufs[0].ptr + offset, n, row_bytes, (nd, nd + ue.num_observables), bufs[2].ptr, d_pred=bufs[1].ptr, **masks)
        info = dict(hp.uf_info(h), **hp.uf_erasure_info(h))  # (synchronises)
        for a, b in ((pred, bufs[1]), (cnt, bufs[2]), (D, bufs[3]), (hist, bufs[4])):
            hp.d2h(a, b)
        if not gap:
            return pred, tuple(int(x) for x in cnt), None, None, None, info
        return pred, tuple(int(x) for x in cnt), D.astype(np.int64), hist[:B].astype(np.int64), hist[B:].astype(np.int64), info
    finally:
        destroy(h)
        for b in bufs:
            b.free()


def check(hp, ue, bits, row_bytes, rng, xor=None, test=None, offset=0):
    want = statement(ue, bits, xor, test)
    clusters = cluster_counts(ue, bits, xor, test)
    got = on_device(hp, ue, bits, row_bytes, rng, xor, test, offset)
    info = got[5]
    print(f"K = {ue.match_defects}, H = {ue.max_hubs}, w_h = {ue.erased_weight}, gap {ue.gap_observable}: host {want[1]}, device {got[1]}; rows whose "
          f"prediction differs {int((got[0] != want[0]).sum())}; clusters matched, peeled, with an erased edge, over H: host {clusters}, device "
          f"{(info['clusters_matched'], info['clusters_peeled'], info['clusters_erased'], info['clusters_hub_overflow'])}")
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    if ue.gap_observable is not None:
        print(f"  rows whose deficit differs {int((got[2] != want[2]).sum())}; 0 < D < G: {int(((want[2] > 0) & (want[2] < ue.gap_cap)).sum())}")
        assert np.array_equal(got[2], want[2])
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        assert got[3].sum() == want[1][0] and got[4].sum() == want[1][1]
    g = ue.graph
    assert (info["clusters_matched"], info["clusters_peeled"], info["clusters_erased"], info["clusters_hub_overflow"]) == clusters
    assert (info["erased_weight"], info["max_hubs"], info["max_defects"]) == (ue.erased_weight, ue.max_hubs, ue.match_defects)
    assert (info["n_heralds"], info["n_det_cols"], info["launches"]) == (g.n_heralds, g.num_detectors, 1)
    assert info["lds_bytes_per_shot"] == uf_erasure_shot_bytes(g.n_nodes, g.n_edges, ue.edge_caps is not None, ue.match_defects, ue.max_hubs,
                                                                ue.gap_observable is not None)
    assert 16 + info["shots_per_block"] * info["lds_bytes_per_shot"] <= 64 * 1024
    return want, clusters


# ---- the main case: d = 3, 3 rounds --------------------------------------------------------------------------------------------

# (pe, K, max_hubs, weighted growth, erased weight, with the gap): every K of 1, 2, 10, 12, max_hubs = K (which forces overflow),
# 12 and 32, both growths and both erased weights at both rates; K = 12 with 32 hubs and the classes does not fit a block's LDS
MAIN = [(1e-2, 10, 32, True, 1, True), (1e-2, 1, 1, True, 1, True), (1e-2, 2, 12, False, 65535, True), (1e-2, 12, 32, True, 1, False),
        (1e-2, 12, 12, False, 1, True), (5e-2, 10, 10, True, 1, True), (5e-2, 12, 12, True, 65535, True), (5e-2, 2, 2, False, 1, False),
        (5e-2, 10, 32, True, 1, True), (5e-2, 1, 12, False, 65535, True), (5e-2, 12, 32, True, 1, False), (5e-2, 2, 32, True, 1, True)]


@pytest.mark.parametrize("pe,K,H,weighted,w_h,gap", MAIN)
def test_d3_bit_for_bit(hp, pe, K, H, weighted, w_h, gap):
    _, uf, bits = surface(3, 3, 3e-3, pe, 4096, weighted)
    assert (uf.graph.n_nodes, bits.shape[1]) == (25, 169)
    ue = uf.with_erasure_matching(K, erased_weight=w_h, max_hubs=H)
    if gap:
        ue = ue.with_gap_output(0)
    want, clusters = check(hp, ue, bits, 24, np.random.default_rng(K))
    assert want[1][1] > 0 and clusters[0] > 300 and clusters[2] > 300
    if H == K and (pe == 5e-2 or K == 1):
        assert clusters[3] > 500   # clusters of at most K defects with more than K hubs
    if pe == 5e-2 and K == 10:
        dets = bits[:, :ue.num_detectors]
        assert (uf.soft_outputs(dets)[:, 2] > 12).any() and clusters[1] > clusters[3]   # large clusters; some have more than 10 defects


def test_d5_matched_and_peeled_clusters_mix(hp):
    _, uf, bits = surface(5, 5, 3e-3, 1e-2, 2000)
    ug = uf.with_erasure_matching(4, max_hubs=12).with_gap_output(0)
    want, clusters = check(hp, ug, bits, 120, np.random.default_rng(5))
    assert min(clusters) > 0 and ((want[2] > 0) & (want[2] < ug.gap_cap)).sum() > 20
    dets = bits[:, :ug.num_detectors]
    assert any(all(ug.match_counts(dets[r:r + 1])) for r in np.flatnonzero(want[2] == ug.gap_cap)[:300])   # both kinds in one row


# ---- the hand graphs ---------------------------------------------------------------------------------------------------------

def test_hand_graphs(hp):
    rng = np.random.default_rng(2)
    g = inner_chain(0)
    ue = UnionFindDecoder(g).with_erasure_matching(weights=INNER_W)
    rows = np.concatenate([row_of(g, d, h) for d, h in (([1, 4], [0]), ([1, 4], []), ([2, 3], [0]), ([1], [0]), ([1, 2, 3, 4], [0]), ([3], []))])
    bits = np.concatenate([rows, rng.random((len(rows), 1)) < 0.5], axis=1)
    want, _ = check(hp, ue, bits, 1, rng)
    assert want[0][:2].tolist() == [0, 1]   # erased: the inner path; clear: both defects to the boundary
    check(hp, ue.with_gap_output(0, cap=1000, bins=128), bits, 8, rng)
    check(hp, UnionFindDecoder(g).with_erasure_matching(weights=INNER_W, erased_weight=65535).with_gap_output(0, cap=1000), bits, 3, rng)
    g = long_chain()
    uf = UnionFindDecoder(g)
    rows = np.concatenate([row_of(g, d, h) for d, h in (([1, 9], [0]), ([2, 5, 9], [0]), ([1, 9], []), ([4], [0]))])
    bits = np.concatenate([rows, np.zeros((len(rows), 1), np.bool_)], axis=1)
    w = np.full(9, 100)
    for K, H in ((2, 9), (2, 8), (3, 9)):   # n = H, n = H + 1, and K + 1 defects
        _, clusters = check(hp, uf.with_erasure_matching(K, w, 1, H).with_gap_output(0, cap=50), bits, 2, rng)
        assert clusters[3] == (2 if H == 8 else 0)


# ---- row counts, masks, stride -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 65, 4096])
def test_row_counts_masks_and_stride(hp, n):
    """Rows of 23 bytes (no multiple of 8) at an odd offset into their buffer, an xor row over detectors, heralds and the
    observable, and a test row; K = 2 at pe = 5e-2 mixes matched and peeled clusters."""
    _, uf, some = surface(3, 3, 3e-3, 5e-2, 4096)
    ug = uf.with_erasure_matching(2, max_hubs=12).with_gap_output(bins=16)
    bits = some[:n] if n > 1 else some[7:8]
    rng = np.random.default_rng(n)
    n_cols = bits.shape[1]
    xor = rng.random(n_cols) < 0.02
    test = np.zeros(n_cols, np.bool_)
    test[[1, 16]] = True
    want, clusters = check(hp, ug, bits, 23, rng, xor=xor, test=test, offset=3)
    if n >= 63:
        assert 0 < want[1][0] < n and clusters[0] > 0 and clusters[1] > 0
    check(hp, ug, bits, 24, rng, offset=8)  # (the 8-byte loads; no masks)


def test_five_byte_rows_at_an_odd_offset(hp):
    """A stride of 5 bytes: the hand-made chain of 9 nodes and 8 heralds, 17 detector columns and an observable."""
    rng = np.random.default_rng(8)
    base = long_chain()
    lists = [[e] for e in range(1, 9)]
    g = with_heralds(without_heralds(base), lists)
    ug = UnionFindDecoder(g).with_erasure_matching(3, rng.integers(1, 30, size=9), 2, 6).with_gap_output(0, cap=40, bins=8)
    n_cols = g.num_detectors + 1
    bits = rng.random((700, n_cols)) < 0.25
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, np.bool_)
    test[3] = True
    want, clusters = check(hp, ug, bits, 5, rng, xor=xor, test=test, offset=3)
    assert min(clusters) > 0 and 0 < want[1][0] < 700


# ---- the front ends ----------------------------------------------------------------------------------------------------------

SHOTS = 6000


@pytest.mark.parametrize("corrected", [False, True])
def test_count_equals_the_statement(hip, corrected):
    c, uf, _ = surface(3, 3, 3e-3, 1e-2, 4096)
    if "count" not in _CASES:
        rows = c.compile_detector_sampler(seed=7, method="faults").sample(SHOTS, append_observables=True)
        rows.setflags(write=False)
        _CASES["count"] = (uf.with_erasure_matching(), uf.with_erasure_matching().with_gap_output(), rows)
    ue, ug, rows = _CASES["count"]
    nd = ug.num_detectors
    got = c.compile_detector_sampler(seed=7, method="faults").count(SHOTS, decoder=ug, corrected=corrected)
    want = tally_rows(rows, num_detectors=nd, decoder=ug, corrected=corrected, histogram_columns=(nd,))
    print(f"kept {got.kept}, decoded errors {got.decoded_errors}, soft_kept {got.soft_kept.tolist()}, soft_errors {got.soft_errors.tolist()}")
    assert got == want
    assert got.soft_output == "gap" and got.soft_kept.sum() == got.kept == SHOTS and got.soft_errors.sum() == got.decoded_errors > 0
    assert got.corrected == corrected and (got.soft_kept[1:] > 0).sum() > 5
    plain = c.compile_detector_sampler(seed=7, method="faults").count(SHOTS, decoder=ue, corrected=corrected)
    assert plain == tally_rows(rows, num_detectors=nd, decoder=ue, corrected=corrected, histogram_columns=(nd,))
    assert plain.decoded_errors == got.decoded_errors and plain.soft_output is None


def test_decode_file_and_decode_device_equal_the_statement(hp, tmp_path):
    _, uf, bits = surface(3, 3, 3e-3, 1e-2, 4096)
    ue = uf.with_erasure_matching()
    ug = ue.with_gap_output()
    bits = bits[:1500]
    nd = ue.num_detectors
    want = statement(ug, bits)
    src, dst = tmp_path / "events.b8", tmp_path / "predictions.01"
    shotdata.write_shot_data_file(data=np.ascontiguousarray(bits), path=src, format="b8", num_detectors=nd, num_observables=1)
    res = ue.decode_file(detection_events_filepath=src, detection_events_format="b8", predictions_filepath=dst, predictions_format="01",
                         observables_appended=True, hp=hp)
    assert res == DecodeFileResult(1500, 1500, want[1][1], 0) and want[1][1] > 0
    got = shotdata.read_shot_data_file(path=dst, format="01", num_observables=1)
    assert got.shape == (1500, 1) and np.array_equal(got[:, 0].astype(np.uint64), want[0])
    rows = packed(bits, 24, np.random.default_rng(3))
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        pred, cnt, D, (kept, errors) = ug.decode_device(hp, d_rows.ptr, len(rows), 24, soft=True)
        plain = ue.decode_device(hp, d_rows.ptr, len(rows), 24)
        as_matching = ug.decode_device(hp, d_rows.ptr, len(rows), 24)   # tsim_uf_decode_device on the handle with the classes
    finally:
        d_rows.free()
    assert np.array_equal(pred, want[0]) and cnt == want[1] and np.array_equal(D, want[2])
    assert np.array_equal(kept, want[3]) and np.array_equal(errors, want[4])
    assert np.array_equal(plain[0], pred) and plain[1] == cnt and np.array_equal(as_matching[0], pred) and as_matching[1] == cnt


# ---- what the new calls refuse -----------------------------------------------------------------------------------------------

def test_refusals(hp):
    g = inner_chain(0)
    w = np.ones(5, np.int64)
    for kw, what in ((dict(max_defects=13), "max_defects"), (dict(erased_weight=0), "erased_w"), (dict(max_hubs=33), "max_hubs"),
                     (dict(max_defects=10, max_hubs=9), "max_hubs"), (dict(observable=64), "observable"), (dict(observable=-2), "observable")):
        args = dict(dict(max_defects=10, erased_weight=1, max_hubs=24), **kw)
        with pytest.raises(ValueError, match=what):
            hp.uf_create_matching_heralds(g, 6, w, **args)
    with pytest.raises(ValueError, match="no heralds"):
        hp.uf_create_matching_heralds(without_heralds(g), 5, w, 10, 1, 24)
    with pytest.raises(_lib.HipBackendError, match="bytes of LDS"):   # TSIM_ENOTSUP: both programs at K = 12 and 32 hubs with their classes
        hp.uf_create_matching_heralds(g, 6, w, 12, 1, 32, 0)
    fits = hp.uf_create_matching_heralds(g, 6, w, 12, 1, 32)   # (without the classes it fits)
    hp.uf_destroy(fits)
    lib = _lib.load()
    h = hp.uf_create_matching_heralds(g, 6, w, 10, 1, 24, 0)
    no_gap = hp.uf_create_matching_heralds(g, 6, w, 10, 1, 24)
    plain = hp.uf_create(g, 6)
    d = hp.malloc(4096)
    try:
        for handle in (h, no_gap):
            with pytest.raises(ValueError, match="no soft outputs"):
                hp.uf_decode_soft_device(handle, d.ptr, 1, 16, (5, 6), d.ptr + 1024, "rounds", 8, d.ptr + 2048)
        with pytest.raises(ValueError, match="no class table"):
            hp.uf_decode_gap_device(no_gap, d.ptr, 1, 16, (5, 6), d.ptr + 1024, 100, 1, 8, d.ptr + 2048)
        with pytest.raises(ValueError, match="gap_cap"):
            hp.uf_decode_gap_device(h, d.ptr, 1, 16, (5, 6), d.ptr + 1024, 0, 1, 8, d.ptr + 2048)
        with pytest.raises(ValueError, match="tsim_uf_create_matching_heralds"):
            hp.uf_erasure_info(plain)
        out = (C.c_int64 * 4)()
        assert lib.tsim_uf_erasure_info(C.c_void_p(plain), out) == -22
        assert hp.uf_erasure_info(h) == dict(erased_weight=1, max_hubs=24, clusters_erased=0, clusters_hub_overflow=0)
        assert hp.uf_info(h)["launches"] == 0 and hp.uf_info(h)["max_defects"] == 10 and hp.uf_info(h)["n_heralds"] == 1
        assert hp.uf_info(h)["lds_bytes_per_shot"] == uf_erasure_shot_bytes(5, 5, False, 10, 24, True)
        assert hp.uf_info(no_gap)["lds_bytes_per_shot"] == uf_erasure_shot_bytes(5, 5, False, 10, 24)
        dist, _ = hp.uf_match_table(no_gap)
        assert np.array_equal(dist, UnionFindDecoder(g).with_erasure_matching(weights=w).match_table()[0])
        # the handles that were there keep their layout: a plain herald handle has no byte of the new arrays
        assert hp.uf_info(plain)["lds_bytes_per_shot"] == uf_shot_bytes(5, 5, False) and hp.uf_info(plain)["max_defects"] == 0
    finally:
        for handle in (h, no_gap, plain):
            hp.uf_destroy(handle)
        d.free()
