"""The row contract of ``csrc/tsim_bitrows.hip.h`` across its five consumers: the tally (``tsim_tally_rows_device``), the pair
counter (``tsim_pairs_*``), the row table and its lookup decoder (``tsim_rowtab_*``), and the two union-find decoders
(``tsim_uf_*``, ``tsim_ufw_*``) keep the same rows of the same buffer - those numpy keeps - whatever the stride and the
alignment; what lies in the rows' pad bits and padding bytes is no column; the pad bits of the masks are cut by everyone but
the tally, which is given zeros there (include/tsim_hip.h); and a bad row argument is refused by all in the same words."""

import ctypes as C

import numpy as np
import pytest

from test_unionfind import chain_graph

from tsim_amd import _lib, synth
from tsim_amd.backend import HipProgram

gpu = pytest.mark.gpu  # (test_seeds_split_the_rows needs no device and is not marked)

N_ROWS = (1, 64, 65, 130)
N_COLS = (5, 64, 70, 1030)  # 1030 columns are 129 bytes: the first size past kChunk
OBS = (3, 4)                # the decoders: a chain of four nodes, detectors in columns 0 .. 2, the observable in column 3
MAX_PAIR_COLS = 70


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def layouts(used):
    """(stride, byte offset of the base): tight (byte loads), odd, 8-aligned (the 8-byte path of row_word), 8-aligned and padded."""
    r8 = (used + 7) // 8 * 8
    return ((used, 0), (used + 3, 1), (r8, 0), (r8 + 8, 8))


def case_inputs(n, n_cols):
    """bool rows of density 0.3, a bool xor row, a test mask of two set columns (column 1 and the last one)."""
    rng = np.random.default_rng(1000 * n_cols + n)
    bits = rng.random((n, n_cols)) < 0.3
    xor = rng.random(n_cols) < 0.3
    test = np.zeros(n_cols, np.bool_)
    test[[1, n_cols - 1]] = True
    return rng, bits, xor, test


def numpy_statement(bits, xor, test):
    """The rule: ``(kept rows, per-column counts over the kept rows)``."""
    v = bits ^ xor[None, :]
    keep = ~(v & test[None, :]).any(axis=1)
    return int(keep.sum()), v[keep].sum(axis=0).astype(np.int64)


def packed_rows(bits, stride, rng):
    """uint8 ``[n, stride]`` little-endian; the pad bits of the last byte and the padding bytes are random."""
    n, n_cols = bits.shape
    full = rng.integers(0, 2, size=(n, 8 * stride), dtype=np.uint8)
    full[:, :n_cols] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little"))


def packed_mask(m, pad_ones):
    p = np.packbits(m, bitorder="little")
    if pad_ones and len(m) % 8:
        p[-1] |= np.uint8((0xFF << (len(m) % 8)) & 0xFF)
    return p


def pair_columns(n_cols):
    """All columns up to MAX_PAIR_COLS of them; of wider rows the first ones and the last two (the second chunk)."""
    return list(range(n_cols)) if n_cols <= MAX_PAIR_COLS else list(range(MAX_PAIR_COLS - 2)) + [n_cols - 2, n_cols - 1]


class Consumers:
    """One handle of each kind for rows of ``n_cols`` columns, and the device buffers of a case."""

    def __init__(self, hp, n_cols):
        self.hp, self.n_cols, self.bufs = hp, n_cols, []
        self.pcols = pair_columns(n_cols)
        self.pairs = hp.pairs_create(n_cols, self.pcols)
        self.tab = hp.rowtab_create(n_cols, self.pcols, 1024)     # keyed by all columns where there are at most 70
        self.look = hp.rowtab_create(n_cols, (0, 1, 2), 64)       # the lookup decoder: an empty loaded table
        hp.rowtab_load(self.look, np.zeros((0, 1), np.uint8), np.zeros(0, np.uint64))
        graph = chain_graph(4, obs_edge=1)
        self.uf = hp.uf_create(graph, n_cols)
        self.ufw = hp.ufw_create(graph, n_cols, 1, 2)

    def up(self, a, offset=0):
        b = self.hp.malloc(a.nbytes + 64)
        self.bufs.append(b)
        self.hp.h2d(b.ptr + offset, a)
        return b.ptr + offset

    def read(self, d, n):
        out = np.zeros(n, np.uint64)
        self.hp.d2h(out, d)
        return out.astype(np.int64)

    def run(self, rows, n, stride, offset, xor, test, pad_ones):
        """What every consumer counts of the n rows: a dict of kept counts, and of column counts."""
        hp, n_cols = self.hp, self.n_cols
        d_rows = self.up(rows, offset)
        masks = dict(d_xor=self.up(packed_mask(xor, pad_ones)), d_test=self.up(packed_mask(test, pad_ones)))
        kept, cols = {}, {}
        if not pad_ones:  # (the tally compares the test mask's whole bytes: its pad bits are zero by contract)
            d_c = self.up(np.zeros(2 + n_cols + 1, np.uint64))
            hp.tally_rows_device(d_rows, n, stride, n_cols, d_c, **masks)
            got = self.read(d_c, 2 + n_cols + 1)
            kept["tally"], cols["tally"] = int(got[0]), got[2:2 + n_cols][self.pcols]
        hp.pairs_add_device(self.pairs, d_rows, n, stride, **masks)
        cols["pairs"] = np.diagonal(hp.pairs_read(self.pairs, len(self.pcols))).copy()
        _lib.check(hp._lib.tsim_pairs_reset(C.c_void_p(self.pairs), C.c_void_p(hp.stream_ptr())), "tsim_pairs_reset")
        hp.rowtab_add_device(self.tab, d_rows, n, stride, **masks)
        _keys, counts, info = hp.rowtab_read(self.tab, len(self.pcols))
        assert info[4] == 0 and info[5] == 0, info  # no overflow, no collision
        kept["rowtab stats"] = int(info[3])
        if n_cols <= MAX_PAIR_COLS:
            kept["rowtab patterns"] = int(np.asarray(counts, np.uint64).sum())
        hp.rowtab_reset(self.tab)
        for name, decode, h in (("rowtab decode", hp.rowtab_decode_device, self.look), ("uf", hp.uf_decode_device, self.uf),
                                ("ufw", hp.ufw_decode_device, self.ufw)):
            d_dec = self.up(np.zeros(3, np.uint64))
            decode(h, d_rows, n, stride, OBS, d_dec, **masks)
            kept[name] = int(self.read(d_dec, 3)[0])
        return kept, cols

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def close(self):
        self.free()
        self.hp.pairs_destroy(self.pairs)
        self.hp.rowtab_destroy(self.tab)
        self.hp.rowtab_destroy(self.look)
        self.hp.uf_destroy(self.uf)
        self.hp.ufw_destroy(self.ufw)


@pytest.fixture(scope="module", params=N_COLS)
def consumers(hp, request):
    c = Consumers(hp, request.param)
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("pad_ones", [False, True], ids=["mask pad bits zero", "mask pad bits set"])
@pytest.mark.parametrize("n", N_ROWS)
def test_consumers_keep_the_same_rows(consumers, n, pad_ones):
    """Every consumer's kept count is numpy's and the column counts of tally and pairs are numpy's, over the four layouts.  With
    the masks' pad bits set (everyone but the tally) the counts are those with the pad bits zero."""
    n_cols = consumers.n_cols
    rng, bits, xor, test = case_inputs(n, n_cols)
    want_kept, want_cols = numpy_statement(bits, xor, test)
    if n >= 64:
        assert 0 < want_kept < n, (want_kept, n)  # neither nothing nor everything: the mask decides
    for stride, offset in layouts((n_cols + 7) // 8):
        try:
            kept, cols = consumers.run(packed_rows(bits, stride, rng), n, stride, offset, xor, test, pad_ones)
        finally:
            consumers.free()
        assert kept == dict.fromkeys(kept, want_kept), (stride, offset, kept, want_kept)
        assert len(kept) == 6 - pad_ones - (n_cols > MAX_PAIR_COLS) and len(cols) == 2 - pad_ones
        for name, got in cols.items():
            assert np.array_equal(got, want_cols[consumers.pcols]), (stride, offset, name)


def test_seeds_split_the_rows():
    """(No device.)  The fixed seeds give kept sets that are neither empty nor full wherever there are 64 rows or more."""
    for n_cols in N_COLS:
        for n in N_ROWS:
            _rng, bits, xor, test = case_inputs(n, n_cols)
            kept, _ = numpy_statement(bits, xor, test)
            assert n < 64 or 0 < kept < n, (n_cols, n, kept)


@gpu
def test_one_refusal_for_all(consumers):
    """row_bytes = used - 1 and n = -1: the same code and the same text from every entry point that takes rows."""
    hp, lib, n_cols = consumers.hp, consumers.hp._lib, consumers.n_cols
    used = (n_cols + 7) // 8
    d_rows, d_out = consumers.up(np.zeros(256, np.uint8)), consumers.up(np.zeros(2 + n_cols + 1, np.uint64))
    p, s = C.c_void_p, C.c_void_p(hp.stream_ptr())
    rows = (p(d_rows), -1, used - 1)
    calls = {
        "tally": lambda: lib.tsim_tally_rows_device(hp.device, *rows, n_cols, None, None, 0, 0, None, 0, p(d_out), s),
        "pairs add": lambda: lib.tsim_pairs_add_device(p(consumers.pairs), *rows, None, None, s),
        "rowtab add": lambda: lib.tsim_rowtab_add_device(p(consumers.tab), *rows, None, None, s),
        "rowtab decode": lambda: lib.tsim_rowtab_decode_device(p(consumers.look), *rows, None, None, *OBS, p(d_out), s),
        "uf decode": lambda: lib.tsim_uf_decode_device(p(consumers.uf), *rows, None, None, *OBS, p(d_out), None, s),
        "ufw decode": lambda: lib.tsim_ufw_decode_device(p(consumers.ufw), *rows, None, None, *OBS, p(d_out), None, s),
    }
    try:
        got = {name: (call(), _lib.last_error()) for name, call in calls.items()}
    finally:
        consumers.free()
    assert got["tally"][0] == -22 and got["tally"][1], got
    assert got == dict.fromkeys(got, got["tally"]), got
