"""count(pair_columns=...) and the pair kernels (tsim_pairs_*) on the device: the kernels exact against the numpy product
over widths, row counts, selections, strides, masks and reference rows; accumulation, reset and counts past 2^32; the
samplers' count(pair_columns=...) equal to the tally of what sample() returns for the same seed and arguments, with the
keys left where sample() leaves them; rows of the measurements -> detection events converter tallied where they lie."""

import ctypes as C
import warnings

import numpy as np
import pytest

from tsim_amd import _lib, circuits, synth
from tsim_amd.backend import HipProgram
from tsim_amd.channels import ChannelSampler, error_probs
from tsim_amd.circuits import rotated_surface_code_memory
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.counts import tally_pairs_device, tally_rows
from tsim_amd.sampler import CompiledDetectorSampler

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def numpy_pairs(bits, cols, xor=None, test=None):
    """B = bits[:, cols] over the kept rows; B.T @ B.  The product runs in float32 blocks of 8192 rows (sums of 0/1
    products below 2^24: exact) and is added up in int64 - the integer product itself, at BLAS speed."""
    v = bits ^ xor[None, :] if xor is not None else bits
    if test is not None:
        v = v[~(v & test[None, :]).any(axis=1)]
    out = np.zeros((len(cols), len(cols)), np.int64)
    for lo in range(0, len(v), 8192):
        B = v[lo:lo + 8192][:, list(cols)].astype(np.float32)
        out += (B.T @ B).astype(np.int64)
    return out


def packed_rows(bits, row_bytes, rng):
    n, n_cols = bits.shape
    rows = np.zeros((n, row_bytes), np.uint8)
    p = np.packbits(bits, axis=1, bitorder="little")
    rows[:, :p.shape[1]] = p
    if n_cols % 8:  # garbage in the pad bits of the last byte and in the padding bytes: never counted
        rows[:, p.shape[1] - 1] |= rng.integers(0, 256, n).astype(np.uint8) & np.uint8((0xFF << (n_cols % 8)) & 0xFF)
    rows[:, p.shape[1]:] = rng.integers(0, 256, (n, row_bytes - p.shape[1]))
    return rows


def random_bits(rng, n, n_cols, density):
    """(in blocks of rows: the float draws of a wide block stay small)"""
    bits = np.empty((n, n_cols), bool)
    for lo in range(0, n, 4096):
        bits[lo:lo + 4096] = rng.random((min(4096, n - lo), n_cols), dtype=np.float32) < density
    return bits


def selection(n_cols, k, rng):
    """k distinct columns in shuffled order, the 64-bit word boundaries and the last column among them where they fit."""
    must = [c for c in dict.fromkeys([n_cols - 1, 0, 63, 64, 127, 128, 1023, 1024, 2047, 2048]) if 0 <= c < n_cols][:k]
    rest = [c for c in rng.permutation(n_cols).tolist() if c not in must][:k - len(must)]
    cols = np.array(must + rest)
    rng.shuffle(cols)
    return tuple(int(c) for c in cols)


class Pairs:
    """A pair counter of the library and device copies of rows and masks (``offset``: the rows' base address mod 16)."""

    def __init__(self, hp, n_cols, cols):
        self.hp, self.n_cols, self.k = hp, n_cols, len(cols)
        self.bufs = []
        self.h = hp.pairs_create(n_cols, cols)

    def up(self, a, offset=0):
        b = self.hp.malloc(max(16, a.nbytes + 32))
        self.bufs.append(b)
        if a.nbytes:
            self.hp.h2d(b.ptr + offset, a)
        return b.ptr + offset

    def mask(self, bits):
        return self.up(np.packbits(bits, bitorder="little")) if bits is not None else 0

    def add(self, d_rows, n, row_bytes, d_xor=0, d_test=0):
        self.hp.pairs_add_device(self.h, d_rows, n, row_bytes, d_xor=d_xor, d_test=d_test)

    def read(self):
        return self.hp.pairs_read(self.h, self.k)

    def info(self):
        out = (C.c_int64 * 4)()
        _lib.check(_lib.load().tsim_pairs_info(C.c_void_p(self.h), out), "tsim_pairs_info")
        return list(out)

    def reset(self):
        _lib.check(_lib.load().tsim_pairs_reset(C.c_void_p(self.h), C.c_void_p(self.hp.stream_ptr())), "tsim_pairs_reset")

    def close(self):
        self.hp.pairs_destroy(self.h)
        for b in self.bufs:
            b.free()


def run_case(hp, bits, cols, row_bytes, offset, rng, xor=None, test=None):
    n, n_cols = bits.shape
    p = Pairs(hp, n_cols, cols)
    try:
        d_rows = p.up(packed_rows(bits, row_bytes, rng), offset)
        p.add(d_rows, n, row_bytes, p.mask(xor), p.mask(test))
        got = p.read()
    finally:
        p.close()
    np.testing.assert_array_equal(got, numpy_pairs(bits, cols, xor, test))
    return got


KS = [1, 2, 24, 64, 65, 1300, 4096]


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 2047, 2049, 9300])
def test_kernels_match_numpy(hp, n_cols):
    """1000 rows (all-zero and all-ones rows among them), every k that fits, with and without xor and test; strides tight
    and padded, even and odd, base addresses aligned and odd."""
    rng = np.random.default_rng(n_cols)
    n = 1000
    bits = rng.random((n, n_cols)) < 0.3
    bits[rng.random(n) < 0.2] = False
    bits[rng.random(n) < 0.05] = True
    used = (n_cols + 7) // 8
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, bool)
    test[rng.choice(n_cols, size=min(n_cols, 3), replace=False)] = True
    layouts = [(used, 0), ((used + 7) // 8 * 8 + 8, 0), (used + 3 + (used % 2), 1), ((used + 3) // 4 * 4, 4)]
    for ki, k in enumerate(k for k in KS if k <= n_cols):
        cols = selection(n_cols, k, rng)
        for i, (use_xor, use_test) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
            row_bytes, offset = layouts[(i + ki) % 4]
            got = run_case(hp, bits, cols, row_bytes, offset, rng, xor if use_xor else None, test if use_test else None)
            assert use_test or got.any(), (k, use_xor)


@pytest.mark.parametrize("n", [1, 63, 64])
@pytest.mark.parametrize("n_cols", [65, 2049])
def test_kernels_few_rows(hp, n, n_cols):
    rng = np.random.default_rng(n * n_cols)
    bits = rng.random((n, n_cols)) < 0.4
    bits[0] = True
    xor = rng.random(n_cols) < 0.5
    test = np.zeros(n_cols, bool)
    test[n_cols // 2] = True
    for k in (k for k in KS if k <= n_cols):
        cols = selection(n_cols, k, rng)
        run_case(hp, bits, cols, (n_cols + 7) // 8 + 1, 1, rng)
        run_case(hp, bits, cols, (n_cols + 7) // 8, 0, rng, xor, test)


@pytest.mark.parametrize("n_cols,k,density", [(63, 24, 0.3), (300, 65, 0.1), (1500, 1300, 0.02), (9300, 4096, 0.01)])
def test_kernels_one_slab_and_a_row(hp, n_cols, k, density):
    """n = the handle's slab + 1: the second pair of launches takes one row (an all-ones row, which every count sees)."""
    rng = np.random.default_rng(k)
    cols = selection(n_cols, k, rng)
    p = Pairs(hp, n_cols, cols)
    try:
        k_info, ws_bytes, slab, launches = p.info()
        assert k_info == k and launches == 0 and 1 << 16 <= slab <= 1 << 20 and slab % 1024 == 0
        assert 0 < ws_bytes <= 32 << 20
        n = slab + 1
        used = (n_cols + 7) // 8
        bits = random_bits(rng, n, n_cols, density)
        bits[-1] = True
        test = np.zeros(n_cols, bool)
        test[cols[0]] = True
        rows = packed_rows(bits, used, rng)
        d_rows = p.up(rows)
        p.add(d_rows, n, used)
        assert p.info()[3] == 4
        want = numpy_pairs(bits, cols)
        np.testing.assert_array_equal(p.read(), want)
        assert want.min() >= 1
        p.reset()
        p.add(d_rows, n, used, 0, p.mask(test))
        np.testing.assert_array_equal(p.read(), numpy_pairs(bits, cols, None, test))
    finally:
        p.close()


def test_counts_accumulate_and_reset(hp):
    rng = np.random.default_rng(5)
    n, n_cols = 70_001, 200
    bits = rng.random((n, n_cols)) < 0.5
    cols = selection(n_cols, 70, rng)
    once = numpy_pairs(bits, cols)
    other = rng.random((333, n_cols)) < 0.5
    p = Pairs(hp, n_cols, cols)
    try:
        d_rows = p.up(packed_rows(bits, 25, rng))  # odd stride: byte staging
        d_other = p.up(packed_rows(other, 32, rng))
        assert not p.read().any()  # zero after create
        p.add(d_rows, n, 25)
        p.add(d_rows, n, 25)
        np.testing.assert_array_equal(p.read(), 2 * once)
        p.add(d_other, 333, 32)  # the counts read so far survive: a further block, of another stride, adds to them
        np.testing.assert_array_equal(p.read(), 2 * once + numpy_pairs(other, cols))
        p.add(d_rows, 0, 25)  # nothing
        np.testing.assert_array_equal(p.read(), 2 * once + numpy_pairs(other, cols))
        p.reset()
        assert not p.read().any()
        p.add(d_rows, n, 25)
        np.testing.assert_array_equal(p.read(), once)
    finally:
        p.close()


def test_counts_past_32_bits(hp):
    """A block of all-ones rows added until every count exceeds 2^32: the uint64 counters carry."""
    n_cols, cols = 8, (7, 0, 3)
    p = Pairs(hp, n_cols, cols)
    try:
        n = p.info()[2]  # one slab: two launches per call
        calls = (1 << 32) // n + 1
        assert calls <= 1 << 16
        d_rows = p.up(np.full((n, 1), 0xFF, np.uint8))
        for _ in range(calls):
            p.add(d_rows, n, 1)
        got = p.read()
        assert n * calls > 1 << 32 and (got == n * calls).all(), (got, n * calls)
        assert p.info()[3] == 2 * calls
    finally:
        p.close()


def test_add_device_checks_arguments(hp):
    p = Pairs(hp, 20, (0, 19))
    try:
        d_rows = p.up(np.zeros((4, 3), np.uint8))
        with pytest.raises(ValueError):
            p.add(d_rows, 4, 2)  # row_bytes < ceil(20 / 8)
        with pytest.raises(ValueError):
            p.add(0, 4, 3)       # no rows
        with pytest.raises(ValueError):
            p.add(d_rows, -1, 3)
        assert p.info()[3] == 0 and not p.read().any()
    finally:
        p.close()
    for cols in ((), (1, 1), (20,), tuple(range(4097))):
        with pytest.raises(ValueError):
            hp.pairs_create(20 if len(cols) < 100 else 5000, cols)


def test_public_tally_pairs_device(hp):
    rng = np.random.default_rng(9)
    n, n_cols = 5000, 70
    bits = rng.random((n, n_cols)) < 0.1
    rows = packed_rows(bits, 16, rng)
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        got = tally_pairs_device(d_rows.ptr, n, row_bytes=16, n_cols=n_cols, pair_columns=(69, 0, 64, 63), device=hp.device,
                                 stream=hp.stream_ptr())
    finally:
        d_rows.free()
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, tally_rows(bits, num_detectors=68, pair_columns=(69, 0, 64, 63)).pair_counts)


def test_m2d_rows_are_tallied_where_they_lie(hip):
    """sample_steps_device -> convert_device -> the pair kernels on the events in HBM == the host product of the events."""
    text = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.02, before_measure_flip_probability=0.02)
    c = CliffordCircuit(text)
    prog, probs, et = c.compile_measurements()
    hp = hip.HipProgram(prog, device=0)
    cs = ChannelSampler(channel_probs=probs, error_transform=et, seed=5)
    B, nf, M = 5000, int(et.shape[0]), int(prog.num_outputs)
    f = cs.sample_packed(B)
    wo = (M + 63) // 64
    conv = c.compile_m2d_converter()
    n_out = conv.num_detectors + conv.num_observables
    rb = (n_out + 7) // 8 + 3
    d_f, d_o, d_e = hp.malloc(f.nbytes), hp.malloc(B * wo * 8), hp.malloc(B * rb)
    try:
        hp.h2d(d_f, f)
        ks = (C.c_uint32 * 2)(0, 7)
        hp.sample_steps_device([d_f.ptr], B, nf, ks, [d_o.ptr])
        hp.pipeline_join(0)
        conv.convert_device(d_o.ptr, B, d_e.ptr, in_row_bytes=8 * wo, in_packed=True, out_row_bytes=rb, out_packed=True,
                            stream=hp.stream_ptr())
        got = tally_pairs_device(d_e.ptr, B, row_bytes=rb, n_cols=n_out, pair_columns="all", device=hp.device, stream=hp.stream_ptr())
        events = np.zeros((B, rb), np.uint8)
        hp.d2h(events, d_e)
    finally:
        for b in (d_f, d_o, d_e):
            b.free()
        hp.close()
    bits = np.unpackbits(events[:, : (n_out + 7) // 8], axis=1, bitorder="little")[:, :n_out].astype(bool)
    np.testing.assert_array_equal(got, numpy_pairs(bits, range(n_out)))
    assert np.diagonal(got).all(), "noise at 2 % should fire every detector"


# ---- the samplers ---------------------------------------------------------------------------------------------------

def c2_maker(noise):
    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    kw = dict(channel_probs=[error_probs(0.03)] * nf, error_transform=np.eye(nf, dtype=np.uint8), noise=noise)
    return lambda: CompiledDetectorSampler(prog, seed=21, **kw)


def clifford_maker(text, noise, measurement=False):
    c = CliffordCircuit(text)

    def mk():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return c.compile_sampler(seed=13, noise=noise) if measurement else c.compile_detector_sampler(seed=13, noise=noise)

    return mk


DISTILL5 = """
    R 0 1 2 3 4
    H 0 1 2
    CX 0 3 1 3 2 4 0 4
    DEPOLARIZE1(0.05) 0 1 2 3 4
    CX 3 1 4 2
    X_ERROR(0.1) 3 4
    M 0 1 2 3 4
"""

FLAGS = [{}, dict(use_detector_reference_sample=True, use_observable_reference_sample=True)]


def masks_for(s):
    """No mask; a mask over direct detectors (host noise: the _DevicePostselect path) and a compiled one; a compiled one."""
    nd, direct = s._num_detectors, s._direct_detector_mask
    out = [None]
    if direct.any():
        m = np.zeros(nd, bool)
        m[np.flatnonzero(direct)[::2]] = True
        m[np.flatnonzero(~direct)[:1]] = True
        out.append(m)
    if (~direct).any():
        m = np.zeros(nd, bool)
        m[np.flatnonzero(~direct)[::3]] = True
        out.append(m)
    return out


def check_detector_count(mk, shots, batch_size, flags, mask, pair_columns):
    """count(pair_columns=...) of a fresh sampler == the tally of sample() of another; then one more batch from both."""
    kw = dict(batch_size=batch_size, postselection_mask=mask, **flags)
    a, b = mk(), mk()
    rows = b.sample(shots, append_observables=True, **kw)
    nd = b._num_detectors
    got = a.count(shots, histogram_columns=(), pair_columns=pair_columns, **kw)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, pair_columns=pair_columns)
    assert got.pair_columns == want.pair_columns and got.pair_counts.dtype == np.int64
    np.testing.assert_array_equal(got.pair_counts, want.pair_counts)
    assert got == want
    np.testing.assert_array_equal(np.diagonal(got.pair_counts), got.column_counts[list(got.pair_columns)])
    if shots:
        assert got.pair_counts.any()
    np.testing.assert_array_equal(a.sample(20_000, append_observables=True, **kw), b.sample(20_000, append_observables=True, **kw))


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("flags", FLAGS)
def test_c2_count_pairs_equal_tally_of_sample(hip, noise, flags):
    """Compiled components: device noise with and without a mask; host noise plain and through _DevicePostselect."""
    mk = c2_maker(noise)
    s = mk()
    n_out = int(s._program.num_outputs)
    shuffled = tuple(int(c) for c in np.random.default_rng(1).permutation(n_out)[: max(2, n_out // 2)])
    masks = masks_for(s)
    assert len(masks) > 1
    for mask in masks:
        for sel in ("all", shuffled):
            check_detector_count(mk, 150_001, 60_000, flags, mask, sel)
    check_detector_count(mk, 0, None, flags, None, "detectors")


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("distance", [3, 5])
def test_surface_code_count_pairs_equal_tally_of_sample(hip, noise, distance):
    """Rotated surface codes: no compiled component, the direct-output path."""
    mk = clifford_maker(rotated_surface_code_memory(distance, distance, after_clifford_depolarization=2e-3,
                                                    before_measure_flip_probability=1e-3), noise)
    s = mk()
    assert not s._program.components
    mask = np.zeros(s._num_detectors, bool)
    mask[::5] = True
    for flags in FLAGS:
        for m, sel in ((None, "all"), (mask, "detectors"), (mask, (s._num_detectors, 3, 0))):
            check_detector_count(mk, 70_001, 30_000, flags, m, sel)
    check_detector_count(mk, 0, None, FLAGS[1], mask, "all")


@pytest.mark.parametrize("noise", ["host", "device"])
def test_measurement_count_pairs(hip, noise):
    mk = clifford_maker(DISTILL5, noise, measurement=True)
    for shots, bs in ((60_001, 16_384), (0, None)):
        a, b = mk(), mk()
        rows = b.sample(shots, batch_size=bs)
        got = a.count(shots, batch_size=bs, pair_columns=(4, 0, 2, 1))
        assert got == tally_rows(rows, num_detectors=b._num_detectors, histogram_columns=(0, 1, 2, 3, 4), pair_columns=(4, 0, 2, 1))
        np.testing.assert_array_equal(a.sample(10_000, batch_size=bs), b.sample(10_000, batch_size=bs))


@pytest.mark.parametrize("noise", ["host", "device"])
def test_default_is_unchanged(hip, noise):
    """No pair_columns: the same counts as pair_columns=(), pair_counts None, and no pair counter is created."""
    mk = c2_maker(noise)
    created = []
    real = HipProgram.pairs_create
    try:
        HipProgram.pairs_create = lambda self, *a, **k: created.append(a) or real(self, *a, **k)
        plain = mk().count(100_001, batch_size=40_000)
        empty = mk().count(100_001, batch_size=40_000, pair_columns=())
        assert not created
        with_pairs = mk().count(100_001, batch_size=40_000, pair_columns="detectors")
        assert len(created) == 1
    finally:
        HipProgram.pairs_create = real
    assert plain == empty and plain.pair_counts is None and plain.pair_columns == ()
    assert (with_pairs.kept, with_pairs.kept_with_observable_flip) == (plain.kept, plain.kept_with_observable_flip)
    np.testing.assert_array_equal(with_pairs.column_counts, plain.column_counts)
    np.testing.assert_array_equal(with_pairs.histogram, plain.histogram)
    p = with_pairs.pair_correlations()
    assert p.shape == (len(with_pairs.pair_columns),) * 2 and np.isnan(np.diagonal(p)).all()
