"""Predictions into rows on the GPU: ``tsim_pred_rows_device`` (``csrc/tsim_predrows.hip.h``) against a numpy bit loop in both
modes, what it refuses, the prediction outlet of the lookup decoder (``tsim_rowtab_decode_pred_device``) against
``LookupDecoder.decode``, and decode-then-correct over rows with 64 observable columns, bit 63 among them."""

import numpy as np
import pytest

from test_gpu_unionfind import packed, random_syndromes
from test_unionfind import wide_observable_graph

from tsim_amd import synth
from tsim_amd.backend import HipProgram
from tsim_amd.decode import LookupDecoder, UnionFindDecoder

pytestmark = pytest.mark.gpu

N = 4096 + 37
# (n_obs, col0, row_bytes, buffer offset); the last two reach the 8-byte path
CASES = [(1, 0, 1, 0), (1, 39, 5, 3), (3, 24, 5, 3), (64, 7, 9, 1), (64, 64, 16, 0), (17, 120, 24, 8)]


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def predictions(rng, n: int, n_obs: int) -> np.ndarray:
    """Random uint64 with random bits above ``n_obs`` too; about half of them are 0."""
    p = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=n, dtype=np.uint64)
    p[rng.random(n) < 0.5] = 0
    return p


def bit_loop(rows: np.ndarray, pred: np.ndarray, n_obs: int, col0: int, mode: str) -> np.ndarray:
    """The statement of include/tsim_hip.h, column by column on unpacked bits."""
    bits = np.unpackbits(rows, axis=1, bitorder="little")
    if mode == "write":
        bits[:, 8 * (col0 // 8):8 * ((col0 + n_obs - 1) // 8) + 8] = 0
    for k in range(n_obs):
        bits[:, col0 + k] ^= ((pred >> np.uint64(k)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


def run(hp, rows: np.ndarray, pred: np.ndarray, n_obs: int, col0: int, offset: int, mode) -> np.ndarray:
    """``pred_rows_device`` over ``rows`` placed ``offset`` bytes into a buffer: the whole buffer afterwards (the bytes around
    the rows were random too)."""
    n, rb = rows.shape
    whole = np.random.default_rng(99).integers(0, 256, size=offset + rows.size + 24, dtype=np.uint8)
    whole[offset:offset + rows.size] = rows.reshape(-1)
    d_rows, d_pred = hp.malloc(whole.nbytes), hp.malloc(pred.nbytes + 16)
    try:
        hp.h2d(d_rows, whole)
        if pred.nbytes:
            hp.h2d(d_pred, pred)
        hp.pred_rows_device(d_pred.ptr, n, n_obs, d_rows.ptr + offset, rb, col0, mode)
        hp.synchronize()
        got = np.zeros_like(whole)
        hp.d2h(got, d_rows)
    finally:
        d_rows.free()
        d_pred.free()
    assert np.array_equal(got[:offset], whole[:offset]) and np.array_equal(got[offset + rows.size:], whole[offset + rows.size:])
    return got[offset:offset + rows.size].reshape(n, rb)


@pytest.mark.parametrize("mode", ["xor", "write"])
@pytest.mark.parametrize("n_obs,col0,row_bytes,offset", CASES)
def test_against_a_numpy_bit_loop(hp, n_obs, col0, row_bytes, offset, mode):
    rng = np.random.default_rng(1000 * col0 + n_obs)
    rows = rng.integers(0, 256, size=(N, row_bytes), dtype=np.uint8)  # pad bits and padding bytes are random
    pred = predictions(rng, N, n_obs)
    keep = np.uint64((1 << n_obs) - 1)
    assert 0.3 < (pred == 0).mean() < 0.7 and ((pred & ~keep) != 0).any() == (n_obs < 64)
    got = run(hp, rows, pred, n_obs, col0, offset, mode)
    want = bit_loop(rows, pred, n_obs, col0, mode)
    assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} rows differ"
    b0, b1 = col0 // 8, (col0 + n_obs - 1) // 8
    outside = np.ones(row_bytes, np.bool_)
    outside[b0:b1 + 1] = False
    assert np.array_equal(got[:, outside], rows[:, outside]), "bytes outside the range changed"
    if mode == "xor":
        zero = (pred & keep) == 0
        assert zero.any() and np.array_equal(got[zero], rows[zero]), "a row that predicts no flip changed"
        assert (got[~zero] != rows[~zero]).any(axis=1).all()


def test_no_rows_is_a_no_op_and_bad_arguments_are_refused(hp):
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 256, size=(64, 5), dtype=np.uint8)
    pred = predictions(rng, 64, 3) | np.uint64(1)
    whole = rows.reshape(-1)
    d_rows, d_pred = hp.malloc(whole.nbytes + 16), hp.malloc(pred.nbytes)
    try:
        hp.h2d(d_rows, whole)
        hp.h2d(d_pred, pred)
        hp.pred_rows_device(d_pred.ptr, 0, 3, d_rows.ptr, 5, 24, "xor")  # n == 0
        hp.pred_rows_device(0, 0, 3, 0, 5, 24, "write")
        for n_obs, col0 in ((3, 38), (0, 0), (65, 0), (64, -1)):  # past the row, no column, too many, a negative column
            for mode in ("xor", "write"):
                with pytest.raises(ValueError):
                    hp.pred_rows_device(d_pred.ptr, 64, n_obs, d_rows.ptr, 5, col0, mode)
        with pytest.raises(ValueError):
            hp.pred_rows_device(d_pred.ptr, 64, 3, d_rows.ptr, 5, 24, 2)  # no such mode
        with pytest.raises(ValueError):
            hp.pred_rows_device(d_pred.ptr + 4, 64, 3, d_rows.ptr, 5, 24, "xor")  # d_pred is not 8-byte aligned
        hp.synchronize()
        got = np.zeros_like(whole)
        hp.d2h(got, d_rows)
        assert np.array_equal(got, whole)
        hp.pred_rows_device(d_pred.ptr, 64, 3, d_rows.ptr, 5, 37, "xor")  # the last three columns of the row are fine
        hp.synchronize()
        hp.d2h(got, d_rows)
        assert np.array_equal(got.reshape(64, 5), bit_loop(rows, pred, 3, 37, "xor"))
    finally:
        d_rows.free()
        d_pred.free()


def test_lookup_decoder_predictions_row_by_row(hp):
    """``rowtab_decode_device(..., d_pred=...)``: known and unknown syndromes, rows that are not kept; the counters are those of
    the call without ``d_pred``."""
    rng = np.random.default_rng(7)
    nd, n_obs, n = 11, 5, N
    syndromes = np.unique(rng.integers(0, 2, size=(300, nd)).astype(np.bool_), axis=0)
    dec = LookupDecoder(syndromes, rng.integers(0, 2, size=(len(syndromes), n_obs)).astype(np.bool_))
    bits = rng.integers(0, 2, size=(n, nd + n_obs)).astype(np.bool_)
    test = np.zeros(nd + n_obs, np.bool_)
    test[[2, 9]] = True
    keep = ~(bits & test).any(axis=1)
    known = ~dec.missed(bits[:, :nd])
    assert (keep & known).any() and (keep & ~known).any() and (~keep & known).any()
    want = (dec.decode(bits[:, :nd]).astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    want[~keep] = 0
    assert want.any() and not want[keep & ~known].any()
    rows = packed(bits, 3, rng)
    h = hp.rowtab_create(nd + n_obs, range(nd), 1024)
    bufs = [hp.malloc(rows.nbytes + 16), hp.malloc(64), hp.malloc(8 * n + 16), hp.malloc(64)]
    try:
        hp.rowtab_load(h, *dec.table())
        hp.h2d(bufs[0], rows)
        hp.h2d(bufs[1], np.zeros(6, np.uint64))
        hp.h2d(bufs[2], np.full(n, 0xFFFF, np.uint64))
        hp.h2d(bufs[3], np.packbits(test, bitorder="little"))
        hp.rowtab_decode_device(h, bufs[0].ptr, n, 3, (nd, nd + n_obs), bufs[1].ptr, d_test=bufs[3].ptr)
        hp.rowtab_decode_device(h, bufs[0].ptr, n, 3, (nd, nd + n_obs), bufs[1].ptr + 24, d_pred=bufs[2].ptr, d_test=bufs[3].ptr)
        hp.rowtab_decode_device(h, bufs[0].ptr, 0, 3, (nd, nd + n_obs), bufs[1].ptr + 24, d_pred=bufs[2].ptr)  # no rows: no launch
        hp.synchronize()
        cnt, pred = np.zeros(6, np.uint64), np.zeros(n, np.uint64)
        hp.d2h(cnt, bufs[1])
        hp.d2h(pred, bufs[2])
    finally:
        hp.rowtab_destroy(h)
        for b in bufs:
            b.free()
    assert np.array_equal(pred, want), f"{int((pred != want).sum())} rows differ"
    obs = (bits[:, nd:].astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert cnt[:3].tolist() == cnt[3:].tolist() == [int(keep.sum()), int((keep & (want != obs)).sum()), int((keep & ~known).sum())]


def test_decode_then_correct_64_observables_bit_for_bit(hp):
    """Three observables, bit 63 among them: 9 detector and 64 observable columns in 11-byte rows at an odd address, decoded with
    ``decode_device`` and corrected where they lie."""
    rng = np.random.default_rng(11)
    uf = UnionFindDecoder(wide_observable_graph(), 64)
    n, nd, rb = 1000, 9, 11
    bits = random_syndromes(rng, n, nd, 64, 5)
    pred_host = uf.predictions(bits[:, :nd])
    assert (pred_host >> np.uint64(63)).any() and (pred_host & np.uint64(3)).any()
    rows = packed(bits, rb, rng)
    want = bit_loop(rows, pred_host, 64, nd, "xor")
    whole = np.concatenate([np.zeros(1, np.uint8), rows.reshape(-1), np.zeros(16, np.uint8)])
    bufs = [hp.malloc(whole.nbytes), hp.malloc(8 * n + 16)]
    try:
        hp.h2d(bufs[0], whole)
        assert (bufs[0].ptr + 1) % 2 == 1
        pred, cnt = uf.decode_device(hp, bufs[0].ptr + 1, n, rb, n_cols=nd + 64)
        hp.h2d(bufs[1], pred)
        hp.pred_rows_device(bufs[1].ptr, n, 64, bufs[0].ptr + 1, rb, nd, "xor")
        hp.synchronize()
        got = np.zeros_like(whole)
        hp.d2h(got, bufs[0])
    finally:
        for b in bufs:
            b.free()
    assert np.array_equal(pred, pred_host) and cnt[0] == n
    assert np.array_equal(got[1:1 + rows.size].reshape(n, rb), want) and got[0] == 0 and not got[1 + rows.size:].any()
    # the corrected observables, unpacked: what numpy gives
    left = np.unpackbits(want, axis=1, bitorder="little")[:, nd:nd + 64].astype(np.bool_)
    assert np.array_equal(left, bits[:, nd:] ^ uf.decode(bits[:, :nd]))
