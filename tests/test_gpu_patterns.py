"""count(pattern_columns=...), count(decoder=...) and the row-table kernels (tsim_rowtab_*) on the device: the kernels
exact against np.unique over widths, row counts, selections, strides, masks and reference rows (never an overflow, never a
collision at a load of 1/4); accumulation, reset, counts past 2^32; the overflow contract; the samplers' count() equal to
the tally of what sample() returns for the same seed and arguments, with the keys left where sample() leaves them; rows of
the measurements -> detection events converter counted where they lie; the lookup decoder against its numpy form."""

import ctypes as C
import warnings

import numpy as np
import pytest

from tsim_amd import _lib, circuits, synth
from tsim_amd.backend import HipProgram
from tsim_amd.channels import ChannelSampler, error_probs
from tsim_amd.circuits import rotated_surface_code_memory
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.counts import tally_patterns_device, tally_rows
from tsim_amd.decode import LookupDecoder
from tsim_amd.sampler import CompiledDetectorSampler

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def numpy_patterns(bits, cols, xor=None, test=None):
    """{packed pattern bytes: count} over the kept rows by np.unique, and the number of kept rows."""
    v = bits ^ xor[None, :] if xor is not None else bits
    if test is not None:
        v = v[~(v & test[None, :]).any(axis=1)]
    if len(v) == 0:
        return {}, 0
    packed = np.packbits(v[:, list(cols)], axis=1, bitorder="little")
    uniq, cnt = np.unique(packed, axis=0, return_counts=True)
    return {u.tobytes(): int(c) for u, c in zip(uniq, cnt)}, len(v)


def packed_rows(bits, row_bytes, rng):
    n, n_cols = bits.shape
    rows = np.zeros((n, row_bytes), np.uint8)
    p = np.packbits(bits, axis=1, bitorder="little")
    rows[:, :p.shape[1]] = p
    if n_cols % 8:  # garbage in the pad bits of the last byte and in the padding bytes: never part of a pattern
        rows[:, p.shape[1] - 1] |= rng.integers(0, 256, n).astype(np.uint8) & np.uint8((0xFF << (n_cols % 8)) & 0xFF)
    rows[:, p.shape[1]:] = rng.integers(0, 256, (n, row_bytes - p.shape[1]))
    return rows


def selection(n_cols, k, rng):
    """k distinct columns in shuffled order, the 64-bit word boundaries and the last column among them where they fit."""
    must = [c for c in dict.fromkeys([n_cols - 1, 0, 63, 64, 127, 128, 1023, 1024, 2047, 2048]) if 0 <= c < n_cols][:k]
    rest = [c for c in rng.permutation(n_cols).tolist() if c not in must][:k - len(must)]
    cols = np.array(must + rest)
    rng.shuffle(cols)
    return tuple(int(c) for c in cols)


def pooled_bits(rng, n, n_cols, pool):
    """n rows drawn from `pool` distinct-ish random rows, 90 % of them replaced by the all-zero row, an all-ones row among them."""
    base = rng.random((pool, n_cols)) < 0.3
    bits = base[rng.integers(0, pool, n)]
    bits[rng.random(n) < 0.9] = False
    bits[rng.integers(0, n)] = True
    return bits


class Table:
    """A row table of the library and device copies of rows and masks (``offset``: the rows' base address mod 16)."""

    def __init__(self, hp, n_cols, cols, capacity):
        self.hp, self.n_cols, self.k = hp, n_cols, len(cols)
        self.bufs = []
        self.h = hp.rowtab_create(n_cols, cols, capacity)

    def up(self, a, offset=0):
        b = self.hp.malloc(max(16, a.nbytes + 32))
        self.bufs.append(b)
        if a.nbytes:
            self.hp.h2d(b.ptr + offset, a)
        return b.ptr + offset

    def mask(self, bits):
        return self.up(np.packbits(bits, bitorder="little")) if bits is not None else 0

    def add(self, d_rows, n, row_bytes, d_xor=0, d_test=0):
        self.hp.rowtab_add_device(self.h, d_rows, n, row_bytes, d_xor=d_xor, d_test=d_test)

    def read(self):
        """({pattern bytes: count}, info)"""
        keys, counts, info = self.hp.rowtab_read(self.h, self.k)
        assert len(keys) == len(counts) == info[1]
        table = {k.tobytes(): int(c) for k, c in zip(keys, counts)}
        assert len(table) == len(keys), "an entry is listed twice"
        return table, dict(zip(("capacity", "entries", "added", "kept", "overflow", "collisions", "launches", "bytes"), info.tolist()))

    def reset(self):
        self.hp.rowtab_reset(self.h)

    def close(self):
        self.hp.rowtab_destroy(self.h)
        for b in self.bufs:
            b.free()


def run_case(hp, bits, cols, row_bytes, offset, rng, xor=None, test=None):
    n, n_cols = bits.shape
    want, kept = numpy_patterns(bits, cols, xor, test)
    t = Table(hp, n_cols, cols, max(64, 4 * len(want)))
    try:
        d_rows = t.up(packed_rows(bits, row_bytes, rng), offset)
        t.add(d_rows, n, row_bytes, t.mask(xor), t.mask(test))
        got, info = t.read()
    finally:
        t.close()
    assert info["overflow"] == 0 and info["collisions"] == 0, info
    assert info["added"] == n and info["kept"] == kept and info["entries"] == len(want) and info["capacity"] >= 4 * len(want)
    assert got == want
    return got


SHAPES = {1: (1000, 1), 63: (70_001, 5000), 64: (30_000, 3000), 65: (70_001, 5000), 200: (50_000, 1000), 2049: (20_000, 500),
          9300: (10_000, 300)}


@pytest.mark.parametrize("n_cols", sorted(SHAPES))
def test_kernels_match_numpy_unique(hp, n_cols):
    """Rows from a pool (duplicates abound; 90 % all-zero rows, an all-ones row); keys "all", a shuffled subset, a single
    column; with and without xor and test; strides tight and padded, even and odd, base addresses aligned and odd."""
    rng = np.random.default_rng(n_cols)
    n, pool = SHAPES[n_cols]
    bits = pooled_bits(rng, n, n_cols, pool)
    used = (n_cols + 7) // 8
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, bool)
    test[rng.choice(n_cols, size=min(n_cols, 3), replace=False)] = True
    layouts = [(used, 0), ((used + 7) // 8 * 8 + 8, 0), (used + 3 + (used % 2), 1), ((used + 3) // 4 * 4, 4)]
    keys = [tuple(range(n_cols)), selection(n_cols, min(n_cols, 150) if n_cols > 2 else n_cols, rng), (n_cols // 2,)]
    if n_cols > 100:
        keys.append(tuple(range(n_cols - 37)))  # a prefix: "detectors"
    for ki, cols in enumerate(keys):
        for i, (use_xor, use_test) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
            row_bytes, offset = layouts[(i + ki) % 4]
            got = run_case(hp, bits, cols, row_bytes, offset, rng, xor if use_xor else None, test if use_test else None)
            assert use_test or sum(got.values()) == n
    if n_cols >= 63:
        assert len(numpy_patterns(bits, keys[0])[0]) > min(pool, 100) // 2


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("n_cols", [40, 65, 2049])
def test_kernels_few_rows(hp, n, n_cols):
    rng = np.random.default_rng(n * n_cols)
    bits = rng.random((n, n_cols)) < 0.4
    bits[0] = True
    xor = rng.random(n_cols) < 0.5
    test = np.zeros(n_cols, bool)
    test[n_cols // 2] = True
    for cols in (tuple(range(n_cols)), selection(n_cols, 33, rng)):
        run_case(hp, bits, cols, (n_cols + 7) // 8 + 1, 1, rng)
        run_case(hp, bits, cols, (n_cols + 7) // 8, 0, rng, xor, test)


def test_high_diversity(hp):
    """Every row its own pattern, and more patterns than a block's cache holds: 64 and 200 random columns."""
    rng = np.random.default_rng(3)
    for n_cols in (64, 200):
        bits = rng.random((40_000, n_cols)) < 0.5
        got = run_case(hp, bits, tuple(range(n_cols)), (n_cols + 7) // 8, 0, rng)
        assert len(got) == 40_000


@pytest.mark.parametrize("n_cols", [30, 200])
def test_counts_accumulate_and_reset(hp, n_cols):
    """Exact keys (30 columns) and fingerprinted ones (200): several adds with different strides, then reset."""
    rng = np.random.default_rng(5)
    n = 70_001
    bits = pooled_bits(rng, n, n_cols, 700)
    other = pooled_bits(rng, 333, n_cols, 50)
    cols = tuple(range(n_cols))
    once, _ = numpy_patterns(bits, cols)
    both, _ = numpy_patterns(np.concatenate([bits, bits, other]), cols)
    used = (n_cols + 7) // 8
    t = Table(hp, n_cols, cols, 8192)
    try:
        d_rows = t.up(packed_rows(bits, used + 1 - used % 2, rng))  # odd stride: byte staging
        d_other = t.up(packed_rows(other, 32, rng))
        got, info = t.read()
        assert got == {} and info["entries"] == 0 and info["bytes"] >= 8192 * 16  # empty after create
        t.add(d_rows, n, used + 1 - used % 2)
        t.add(d_rows, n, used + 1 - used % 2)
        assert t.read()[0] == {k: 2 * v for k, v in once.items()}
        t.add(d_other, 333, 32)  # the counts read so far survive: a further block, of another stride, adds to them
        got, info = t.read()
        assert got == both and info["added"] == 2 * n + 333 == info["kept"]
        t.add(d_rows, 0, used)  # nothing
        assert t.read()[0] == both
        t.reset()
        got, info = t.read()
        assert got == {} and (info["entries"], info["added"], info["kept"], info["overflow"]) == (0, 0, 0, 0)
        t.add(d_rows, n, used + 1 - used % 2)
        got, info = t.read()
        assert got == once and info["collisions"] == 0
        assert info["launches"] == (4 if n_cols <= 63 else 8)  # one launch per add; a second one verifies wide keys
    finally:
        t.close()


@pytest.mark.parametrize("n_cols", [8, 70])
def test_counts_past_32_bits(hp, n_cols):
    """A block of all-ones rows added until the pattern's count exceeds 2^32: the uint64 counters carry."""
    used = (n_cols + 7) // 8
    t = Table(hp, n_cols, tuple(range(n_cols)), 64)
    try:
        n = 1 << 20
        calls = (1 << 32) // n + 1
        d_rows = t.up(np.full((n, used), 0xFF, np.uint8))
        for _ in range(calls):
            t.add(d_rows, n, used)
        got, info = t.read()
        ones = np.packbits(np.ones(n_cols, bool), bitorder="little").tobytes()
        assert n * calls > 1 << 32 and got == {ones: n * calls}, (got, n * calls)
        assert info["kept"] == n * calls and info["overflow"] == 0 and info["collisions"] == 0
    finally:
        t.close()


@pytest.mark.parametrize("n_cols", [40, 100])
def test_overflow_is_defined(hp, n_cols):
    """Capacity 64, thousands of distinct patterns: what is in the table is true and exact, the rest is counted."""
    rng = np.random.default_rng(n_cols)
    n = 50_000
    bits = pooled_bits(rng, n, n_cols, 3000)
    bits[rng.random(n) < 0.5] = rng.random(n_cols) < 0.5  # (one more pattern that dominates)
    cols = tuple(range(n_cols))
    want, kept = numpy_patterns(bits, cols)
    assert len(want) >= 1000
    used = (n_cols + 7) // 8
    t = Table(hp, n_cols, cols, 64)
    try:
        d_rows = t.up(packed_rows(bits, used, rng))
        for rounds in (1, 2):  # (the second add finds the same table: nothing is freed, nothing new fits)
            t.add(d_rows, n, used)
            got, info = t.read()
            assert info["capacity"] == 64 and len(got) == info["entries"] <= 64 and info["collisions"] == 0
            assert all(key in want and got[key] == rounds * want[key] for key in got)
            assert sum(got.values()) + info["overflow"] == info["kept"] == rounds * kept and info["overflow"] > 0
    finally:
        t.close()


def test_add_device_checks_arguments(hp):
    t = Table(hp, 20, (0, 19), 64)
    try:
        d_rows = t.up(np.zeros((4, 3), np.uint8))
        with pytest.raises(ValueError):
            t.add(d_rows, 4, 2)  # row_bytes < ceil(20 / 8)
        with pytest.raises(ValueError):
            t.add(0, 4, 3)       # no rows
        with pytest.raises(ValueError):
            t.add(d_rows, -1, 3)
        got, info = t.read()
        assert info["launches"] == 0 and got == {}
        d_cnt = t.up(np.zeros(3, np.uint64))
        with pytest.raises(_lib.HipBackendError):  # no values loaded yet
            hp.rowtab_decode_device(t.h, d_rows, 4, 3, (19, 20), d_cnt)
        hp.rowtab_load(t.h, np.array([[0], [1]], np.uint8), np.array([0, 1], np.uint64))
        for obs in ((19, 21), (5, 3), (-1, 2)):
            with pytest.raises(ValueError):
                hp.rowtab_decode_device(t.h, d_rows, 4, 3, obs, d_cnt)
        with pytest.raises(ValueError):
            hp.rowtab_decode_device(t.h, d_rows, 4, 3, (19, 20), 0)
        with pytest.raises(ValueError):
            hp.rowtab_load(t.h, np.array([[1], [1]], np.uint8), np.array([0, 1], np.uint64))  # a key twice
        assert t.hp.rowtab_info(t.h)[6] == 0
    finally:
        t.close()
    for cols in ((), (1, 1), (20,), tuple(range(21))):
        with pytest.raises(ValueError):
            hp.rowtab_create(20, cols, 64)
    with pytest.raises(ValueError):
        hp.rowtab_create(20, (0,), 0)


def test_public_tally_patterns_device(hp):
    rng = np.random.default_rng(9)
    n, n_cols = 5000, 70
    bits = pooled_bits(rng, n, n_cols, 40)
    rows = packed_rows(bits, 16, rng)
    d_rows = hp.malloc(rows.nbytes)
    try:
        hp.h2d(d_rows, rows)
        pat, cnt, overflow = tally_patterns_device(d_rows.ptr, n, row_bytes=16, n_cols=n_cols, pattern_columns=(69, 0, 64, 63),
                                                   capacity=256, device=hp.device, stream=hp.stream_ptr())
    finally:
        d_rows.free()
    want = tally_rows(bits, num_detectors=68, pattern_columns=(69, 0, 64, 63))
    assert pat.dtype == np.bool_ and cnt.dtype == np.int64 and overflow == 0
    np.testing.assert_array_equal(pat, want.patterns)
    np.testing.assert_array_equal(cnt, want.pattern_counts)


def test_m2d_rows_are_counted_where_they_lie(hip):
    """sample_steps_device -> convert_device -> the row table on the events in HBM == np.unique of the events."""
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
        pat, cnt, overflow = tally_patterns_device(d_e.ptr, B, row_bytes=rb, n_cols=n_out, pattern_columns="all", capacity=1 << 15,
                                                   device=hp.device, stream=hp.stream_ptr())
        events = np.zeros((B, rb), np.uint8)
        hp.d2h(events, d_e)
    finally:
        for b in (d_f, d_o, d_e):
            b.free()
        hp.close()
    bits = np.unpackbits(events[:, : (n_out + 7) // 8], axis=1, bitorder="little")[:, :n_out].astype(bool)
    want = tally_rows(bits, num_detectors=conv.num_detectors, pattern_columns="all")
    assert overflow == 0 and cnt.sum() == B and len(cnt) > 100, "noise at 2 % should give many patterns"
    np.testing.assert_array_equal(pat, want.patterns)
    np.testing.assert_array_equal(cnt, want.pattern_counts)


# ---- the samplers ---------------------------------------------------------------------------------------------------

def c2_maker(noise, seed=21):
    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    kw = dict(channel_probs=[error_probs(0.03)] * nf, error_transform=np.eye(nf, dtype=np.uint8), noise=noise)
    return lambda: CompiledDetectorSampler(prog, seed=seed, **kw)


def clifford_maker(text, noise, measurement=False, seed=13):
    c = CliffordCircuit(text)

    def mk():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return c.compile_sampler(seed=seed, noise=noise) if measurement else c.compile_detector_sampler(seed=seed, noise=noise)

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


def check_detector_count(mk, shots, batch_size, flags, mask, pattern_columns):
    """count(pattern_columns=...) of a fresh sampler == the tally of sample() of another; then one more batch from both."""
    kw = dict(batch_size=batch_size, postselection_mask=mask, **flags)
    a, b = mk(), mk()
    rows = b.sample(shots, append_observables=True, **kw)
    nd = b._num_detectors
    got = a.count(shots, histogram_columns=(), pattern_columns=pattern_columns, **kw)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, pattern_columns=pattern_columns)
    assert got.pattern_columns == want.pattern_columns and got.pattern_counts.dtype == np.int64 and got.patterns.dtype == np.bool_
    np.testing.assert_array_equal(got.patterns, want.patterns)
    np.testing.assert_array_equal(got.pattern_counts, want.pattern_counts)
    assert got == want
    assert got.pattern_overflow == 0 and got.pattern_counts.sum() == got.kept
    if shots:
        assert len(got.patterns) > 1
    np.testing.assert_array_equal(a.sample(20_000, append_observables=True, **kw), b.sample(20_000, append_observables=True, **kw))


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("flags", FLAGS)
def test_c2_count_patterns_equal_tally_of_sample(hip, noise, flags):
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
def test_surface_code_count_patterns_equal_tally_of_sample(hip, noise, distance):
    """Rotated surface codes: no compiled component, the direct-output path (d = 5: 121 columns, fingerprinted keys)."""
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
def test_measurement_count_patterns(hip, noise):
    mk = clifford_maker(DISTILL5, noise, measurement=True)
    for shots, bs in ((60_001, 16_384), (0, None)):
        a, b = mk(), mk()
        rows = b.sample(shots, batch_size=bs)
        got = a.count(shots, batch_size=bs, pattern_columns=(4, 0, 2, 1))
        assert got == tally_rows(rows, num_detectors=b._num_detectors, histogram_columns=(0, 1, 2, 3, 4), pattern_columns=(4, 0, 2, 1))
        assert a.count(1000, batch_size=bs, pattern_columns="all") == tally_rows(
            b.sample(1000, batch_size=bs), num_detectors=b._num_detectors, histogram_columns=(0, 1, 2, 3, 4), pattern_columns="all")
        np.testing.assert_array_equal(a.sample(10_000, batch_size=bs), b.sample(10_000, batch_size=bs))


@pytest.mark.parametrize("noise", ["host", "device"])
def test_default_is_unchanged(hip, noise):
    """No pattern_columns: the same counts as pattern_columns=(), patterns None, and no row table is created."""
    mk = c2_maker(noise)
    created = []
    real = HipProgram.rowtab_create
    try:
        HipProgram.rowtab_create = lambda self, *a, **k: created.append(a) or real(self, *a, **k)
        plain = mk().count(100_001, batch_size=40_000)
        empty = mk().count(100_001, batch_size=40_000, pattern_columns=())
        assert not created
        with_patterns = mk().count(100_001, batch_size=40_000, pattern_columns="detectors")
        assert len(created) == 1
    finally:
        HipProgram.rowtab_create = real
    assert plain == empty and plain.patterns is None and plain.pattern_counts is None and plain.pattern_columns == ()
    assert plain.pattern_overflow == 0 and plain.decoded_errors is None and plain.decoder_misses is None
    assert (with_patterns.kept, with_patterns.kept_with_observable_flip) == (plain.kept, plain.kept_with_observable_flip)
    np.testing.assert_array_equal(with_patterns.column_counts, plain.column_counts)
    np.testing.assert_array_equal(with_patterns.histogram, plain.histogram)
    assert with_patterns.pattern_counts.sum() == plain.kept


@pytest.mark.parametrize("noise", ["host", "device"])
def test_count_warns_when_patterns_overflow(hip, noise):
    mk = clifford_maker(rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.02, before_measure_flip_probability=0.02), noise)
    rows = mk().sample(70_001, batch_size=30_000, append_observables=True)
    want = tally_rows(rows, num_detectors=24, pattern_columns="all")
    assert len(want.patterns) >= 1000
    truth = {np.packbits(p, bitorder="little").tobytes(): int(c) for p, c in zip(want.patterns, want.pattern_counts)}
    with pytest.warns(RuntimeWarning, match="pattern_capacity=64"):
        got = mk().count(70_001, batch_size=30_000, pattern_columns="all", pattern_capacity=64)
    assert 0 < len(got.patterns) <= 64 and got.pattern_overflow > 0
    assert got.pattern_counts.sum() + got.pattern_overflow == got.kept == want.kept
    assert all(truth[np.packbits(p, bitorder="little").tobytes()] == c for p, c in zip(got.patterns, got.pattern_counts.tolist()))
    assert (np.diff(got.pattern_counts) <= 0).all()


# ---- the lookup decoder -------------------------------------------------------------------------------------------------

def numpy_decode(dec, rows, nd, mask=None):
    """(kept, wrong, unknown) of rows (detectors, then observables) by LookupDecoder.decode / missed."""
    if mask is not None:
        rows = rows[~(rows[:, :nd] & mask).any(axis=1)]
    wrong = (dec.decode(rows[:, :nd]) != rows[:, nd:]).any(axis=1)
    return len(rows), int(wrong.sum()), int(dec.missed(rows[:, :nd]).sum())


def check_decoder_count(mk, dec, shots, batch_size, flags, mask):
    kw = dict(batch_size=batch_size, postselection_mask=mask, **flags)
    a, b = mk(), mk()
    rows = b.sample(shots, append_observables=True, **kw)
    nd = b._num_detectors
    got = a.count(shots, decoder=dec, **kw)
    assert (got.kept, got.decoded_errors, got.decoder_misses) == numpy_decode(dec, rows, nd, mask)
    assert got == tally_rows(rows, num_detectors=nd, postselection_mask=mask, histogram_columns=got.histogram_columns, decoder=dec)
    np.testing.assert_array_equal(a.sample(20_000, append_observables=True, **kw), b.sample(20_000, append_observables=True, **kw))
    return got


@pytest.mark.parametrize("noise", ["host", "device"])
def test_c2_count_decoder_equals_numpy_decode(hip, noise):
    """15 direct detectors, 5 compiled observables; a decoder trained on a few shots, so that unknown syndromes occur."""
    mk = c2_maker(noise)
    train = c2_maker(noise, seed=4)().count(3_000, pattern_columns="all")
    dec = LookupDecoder.from_counts(train)
    assert (dec.num_detectors, dec.num_observables) == (15, 5) and len(dec) > 10
    seen = []
    for flags in FLAGS:
        for mask in masks_for(mk()):
            seen.append(check_decoder_count(mk, dec, 150_001, 60_000, flags, mask))
    assert any(g.decoder_misses > 0 for g in seen)
    both = mk().count(50_000, decoder=dec, pattern_columns="all", pair_columns="detectors")  # every counter in one call
    alone = mk().count(50_000, decoder=dec)
    assert (both.decoded_errors, both.decoder_misses, both.kept) == (alone.decoded_errors, alone.decoder_misses, alone.kept)
    assert both.pattern_counts.sum() == both.kept and both.pair_counts is not None


@pytest.mark.parametrize("noise", ["host", "device"])
def test_noiseless_circuit_decodes_without_errors(hip, noise):
    mk = clifford_maker(rotated_surface_code_memory(3, 3), noise)
    train = mk().count(10_000, pattern_columns="all")
    assert len(train.patterns) == 1 and train.pattern_counts.tolist() == [10_000]
    dec = LookupDecoder.from_counts(train)
    got = clifford_maker(rotated_surface_code_memory(3, 3), noise, seed=99)().count(100_001, batch_size=40_000, decoder=dec)
    assert (got.kept, got.decoded_errors, got.decoder_misses) == (100_001, 0, 0)


@pytest.mark.parametrize("noise", ["host", "device"])
def test_surface_code_decoder_trained_on_another_seed(hip, noise):
    """d = 3 at p = 2e-3: a table trained on one seed lowers the logical error rate of another seed's shots."""
    text = rotated_surface_code_memory(3, 3, after_clifford_depolarization=2e-3, before_measure_flip_probability=1e-3)
    train = clifford_maker(text, noise, seed=1)().count(1_000_000, pattern_columns="all")
    assert train.pattern_overflow == 0 and train.pattern_counts.sum() == 1_000_000
    dec = LookupDecoder.from_counts(train)
    mk = clifford_maker(text, noise, seed=2)
    mask = np.zeros(24, bool)
    mask[::7] = True
    for flags in FLAGS:
        for m in (None, mask):
            got = check_decoder_count(mk, dec, 200_001, 70_000, flags, m)
            assert got.decoded_errors <= got.kept_with_observable_flip
    assert 0 < got.decoded_errors < got.kept_with_observable_flip
