"""Pattern counts and the lookup decoder without a device: tally_rows(pattern_columns=...) against a direct dictionary
count (ordering, masks, selections, empty input, capacity), the validation, ShotCounts.__eq__, the library's argument
checks, LookupDecoder (from_counts with ties, decode, missed), and count(pattern_columns=...) / count(decoder=...) on the
paths that never touch a device."""

import ctypes as C
from collections import Counter

import numpy as np
import pytest

import tsim_amd.sampler as sampler_module
from oracle import oracle_np as O
from tsim_amd import _lib
from tsim_amd.channels import error_probs
from tsim_amd.counts import ShotCounts, check_pattern_columns, tally_patterns_device, tally_rows
from tsim_amd.decode import LookupDecoder
from tsim_amd.program import CompiledComponent, make_program, scalar_graphs_from_terms
from tsim_amd.sampler import CompiledDetectorSampler, CompiledMeasurementSampler


def dictionary_count(rows, cols, nd, mask=None):
    """{packed pattern bytes: count} over the kept rows, and the expected order: count descending, bytes ascending."""
    if mask is not None:
        rows = rows[~(rows[:, :nd] & mask).any(axis=1)]
    tab = Counter(np.packbits(r[list(cols)], bitorder="little").tobytes() for r in rows)
    order = sorted(tab, key=lambda k: (-tab[k], k))
    return tab, order


def assert_patterns(got: ShotCounts, rows, cols, nd, mask=None):
    tab, order = dictionary_count(rows, cols, nd, mask)
    k = len(cols)
    assert got.pattern_columns == tuple(cols)
    assert got.patterns.dtype == np.bool_ and got.patterns.shape == (len(order), k)
    assert got.pattern_counts.dtype == np.int64 and got.pattern_counts.shape == (len(order),)
    keys = [np.packbits(p, bitorder="little").tobytes() for p in got.patterns]
    assert keys == order
    assert got.pattern_counts.tolist() == [tab[key] for key in order]
    assert got.pattern_overflow == 0 and int(got.pattern_counts.sum()) == got.kept


@pytest.mark.parametrize("seed", range(4))
def test_tally_rows_patterns_match_a_dictionary_count(seed):
    rng = np.random.default_rng(seed)
    n, n_cols, nd = 600, 11, 8
    pool = rng.random((12, n_cols)) < 0.4
    rows = pool[rng.integers(0, 12, n)]
    rows[rng.random(n) < 0.5] = False
    mask = np.zeros(nd, bool)
    mask[[1, 6]] = True
    shuffled = tuple(int(c) for c in rng.permutation(n_cols)[:7])
    for m in (None, mask):
        for sel, cols in (("all", tuple(range(n_cols))), ("detectors", tuple(range(nd))), (shuffled, shuffled), ((9,), (9,))):
            got = tally_rows(rows, num_detectors=nd, postselection_mask=m, pattern_columns=sel)
            assert_patterns(got, rows, cols, nd, m)
    # a reference row XORed in by the caller, as count(use_*_reference_sample=True) does it
    ref = rng.random(n_cols) < 0.5
    assert_patterns(tally_rows(rows ^ ref, num_detectors=nd, postselection_mask=mask, pattern_columns="all"), rows ^ ref,
                    tuple(range(n_cols)), nd, mask)


def test_ordering_rule():
    """count descending; equal counts by the little-endian packed bytes ascending: column 0 is the lowest bit of byte 0."""
    rows = np.array([[0, 1, 0]] * 3 + [[1, 0, 0]] * 3 + [[0, 0, 1]] * 5 + [[1, 1, 0]] * 3 + [[0, 0, 0]], bool)
    got = tally_rows(rows, num_detectors=3, pattern_columns="all")
    assert got.patterns.astype(int).tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 0]]
    assert got.pattern_counts.tolist() == [5, 3, 3, 3, 1]
    # more than one byte: byte 0 decides before byte 1
    wide = np.zeros((4, 10), bool)
    wide[0, 9] = wide[1, 9] = True      # bytes (0, 2)
    wide[2, 0] = wide[3, 0] = True      # bytes (1, 0)
    got = tally_rows(wide, num_detectors=10, pattern_columns="all")
    assert got.patterns[0, 9] and got.patterns[1, 0] and got.pattern_counts.tolist() == [2, 2]
    # the order of the selection is the order of the pattern's bits
    got = tally_rows(wide, num_detectors=10, pattern_columns=(9, 0))
    assert got.patterns.astype(int).tolist() == [[1, 0], [0, 1]]


def test_empty_input_and_no_kept_rows():
    got = tally_rows(np.zeros((0, 5), bool), num_detectors=3, pattern_columns="all")
    assert got.patterns.shape == (0, 5) and got.pattern_counts.shape == (0,) and got.pattern_overflow == 0
    rows = np.ones((7, 5), bool)
    got = tally_rows(rows, num_detectors=3, postselection_mask=np.array([True, False, False]), pattern_columns=(4, 1))
    assert got.kept == 0 and got.patterns.shape == (0, 2) and got.pattern_counts.dtype == np.int64
    plain = tally_rows(rows, num_detectors=3)
    assert plain.patterns is None and plain.pattern_counts is None and plain.pattern_columns == () and plain.pattern_overflow == 0
    assert plain.decoded_errors is None and plain.decoder_misses is None
    assert plain == tally_rows(rows, num_detectors=3, pattern_columns=())


def test_host_capacity_admits_patterns_in_order_of_first_appearance():
    rows = np.array([[1, 0], [0, 1], [1, 0], [1, 1], [0, 1], [0, 0], [1, 1]], bool)
    got = tally_rows(rows, num_detectors=2, pattern_columns="all", pattern_capacity=2)
    assert got.patterns.astype(int).tolist() == [[1, 0], [0, 1]] and got.pattern_counts.tolist() == [2, 2]
    assert got.pattern_overflow == 3 and got.pattern_counts.sum() + got.pattern_overflow == got.kept
    for bad in (0, -1, 1.5, (1 << 30) + 1):
        with pytest.raises(ValueError):
            tally_rows(rows, num_detectors=2, pattern_columns="all", pattern_capacity=bad)


def test_check_pattern_columns():
    assert check_pattern_columns(None, 9, 7) == () and check_pattern_columns((), 9, 7) == ()
    assert check_pattern_columns("all", 9, 7) == tuple(range(9)) and check_pattern_columns("detectors", 9, 7) == tuple(range(7))
    assert check_pattern_columns(np.array([8, 0, 3]), 9, 7) == (8, 0, 3)
    assert check_pattern_columns("all", 10000, 9000) == tuple(range(10000))  # no cap on the width
    assert len(check_pattern_columns(list(range(5000)), 6000, 10)) == 5000
    for bad in ([9], [-1], [1, 1], "observables", np.zeros((2, 2), np.int64), [0.5]):
        with pytest.raises(ValueError):
            check_pattern_columns(bad, 9, 7)


def test_shot_counts_equality_sees_the_new_fields():
    base = (10, 4, 1, np.array([1, 2, 3, 0, 1]), 3, (3, 4), np.array([2, 1, 0, 1]), (), None)
    pat, cnt = np.array([[0, 0], [1, 0]], bool), np.array([3, 1])
    a = ShotCounts(*base, (0, 1), pat, cnt, 0)
    assert a == ShotCounts(*base, (0, 1), pat.copy(), cnt.copy(), 0)
    assert a != ShotCounts(*base)
    assert a != ShotCounts(*base, (1, 0), pat, cnt, 0)
    assert a != ShotCounts(*base, (0, 1), pat[::-1], cnt, 0)
    assert a != ShotCounts(*base, (0, 1), pat, np.array([2, 2]), 0)
    assert a != ShotCounts(*base, (0, 1), pat, cnt, 1)
    assert a != ShotCounts(*base, (0, 1), pat, cnt, 0, 2, 0)
    assert ShotCounts(*base, (0, 1), pat, cnt, 0, 2, 1) == ShotCounts(*base, (0, 1), pat, cnt, 0, 2, 1)
    assert ShotCounts(*base, (0, 1), pat, cnt, 0, 2, 1) != ShotCounts(*base, (0, 1), pat, cnt, 0, 2, 0)


# ---- the library without a device ------------------------------------------------------------------------------------

def test_rowtab_checks_before_any_device_call():
    lib = _lib.load()

    def create(n_cols, cols, n_key=None, capacity=64, out=True):
        a = np.asarray(cols, np.int32)
        h = C.c_void_p()
        rc = lib.tsim_rowtab_create(0, n_cols, a.ctypes.data_as(C.c_void_p) if a.size else None, len(a) if n_key is None else n_key,
                                    capacity, C.byref(h) if out else None)
        assert h.value is None
        return rc

    for rc in (create(8, [], 0), create(8, [0], -1), create(8, list(range(9))),          # n_key outside 1 .. n_cols
               create(8, [0, 3, 0]), create(8, [7, 7]),                                   # duplicates
               create(8, [8]), create(8, [-1]), create(8, [1, 2, 100]),                    # not a column
               create(0, [0]), create(8, [], 3), create(8, [0], out=False),                # no columns, NULL list, NULL out
               create(8, [0], capacity=0), create(8, [0], capacity=(1 << 30) + 1)):        # capacity outside 1 .. 2^30
        assert rc == -22
        assert _lib.last_error()
    n = C.c_int64(-1)
    assert lib.tsim_rowtab_add_device(None, None, 0, 1, None, None, None) == -22
    assert lib.tsim_rowtab_read(None, None, None, 0, C.byref(n), None) == -22
    assert lib.tsim_rowtab_reset(None, None) == -22
    assert lib.tsim_rowtab_info(None, None) == -22
    assert lib.tsim_rowtab_load(None, None, None, 0) == -22
    assert lib.tsim_rowtab_decode_device(None, None, 0, 1, None, None, 0, 0, None, None) == -22
    lib.tsim_rowtab_destroy(None)


def test_tally_patterns_device_checks_arguments_on_the_host():
    for kw in (dict(n=-1), dict(n_cols=0), dict(row_bytes=1, n_cols=9), dict(pattern_columns=[8]), dict(pattern_columns=[1, 1]),
               dict(pattern_columns=()), dict(capacity=0)):
        args = dict(n=5, row_bytes=2, n_cols=8, pattern_columns=[0, 1])
        args.update(kw)
        n = args.pop("n")
        with pytest.raises(ValueError):
            tally_patterns_device(0, n, **args)


# ---- the lookup decoder -----------------------------------------------------------------------------------------------

def test_decoder_from_counts_picks_the_likeliest_observables_and_breaks_ties():
    # 2 detectors, 2 observables; columns: d0 d1 o0 o1
    rows = np.array([[0, 0, 0, 0]] * 9 + [[0, 0, 1, 0]] * 2        # syndrome 00: no flip wins
                    + [[1, 0, 1, 0]] * 4 + [[1, 0, 0, 0]] * 3       # syndrome 10: o0 wins
                    + [[0, 1, 0, 1]] * 2 + [[0, 1, 1, 0]] * 2       # syndrome 01: a tie, value 1 (o0) < value 2 (o1)
                    + [[1, 1, 1, 1]] * 1, bool)                     # syndrome 11: seen once
    train = tally_rows(rows, num_detectors=2, pattern_columns="all")
    dec = LookupDecoder.from_counts(train)
    assert len(dec) == 4 and (dec.num_detectors, dec.num_observables) == (2, 2)
    table = {tuple(s): tuple(p) for s, p in zip(dec.syndromes.astype(int).tolist(), dec.predictions.astype(int).tolist())}
    assert table == {(0, 0): (0, 0), (1, 0): (1, 0), (0, 1): (1, 0), (1, 1): (1, 1)}
    dets = np.array([[0, 1], [1, 1], [0, 0], [1, 0], [0, 1]], bool)
    assert dec.decode(dets).astype(int).tolist() == [[1, 0], [1, 1], [0, 0], [1, 0], [1, 0]]
    assert not dec.missed(dets).any()
    keys, values = dec.table()
    assert keys.shape == (4, 1) and values.dtype == np.uint64
    assert {int(k[0]): int(v) for k, v in zip(keys, values)} == {0: 0, 1: 1, 2: 1, 3: 3}
    # the numbers count(decoder=...) reports, on the host
    got = tally_rows(rows, num_detectors=2, decoder=dec)
    assert got.decoded_errors == 2 + 3 + 2 and got.decoder_misses == 0


def test_decoder_unknown_syndromes_predict_no_flip():
    dec = LookupDecoder(np.array([[1, 0, 0], [0, 0, 0]], bool), np.array([[1], [0]], bool))
    dets = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 1]], bool)
    assert dec.decode(dets).astype(int).tolist() == [[1], [0], [0], [0]]
    assert dec.missed(dets).tolist() == [False, True, False, True]
    assert dec.decode(np.zeros((0, 3), bool)).shape == (0, 1) and dec.missed(np.zeros((0, 3), bool)).shape == (0,)
    rows = np.concatenate([dets, np.array([[1], [1], [1], [0]], bool)], axis=1)
    got = tally_rows(rows, num_detectors=3, decoder=dec)
    assert (got.decoded_errors, got.decoder_misses) == (2, 2)
    masked = tally_rows(rows, num_detectors=3, decoder=dec, postselection_mask=np.array([False, True, False]))
    assert (masked.kept, masked.decoded_errors, masked.decoder_misses) == (2, 1, 0)


def test_decoder_validation():
    with pytest.raises(ValueError):
        LookupDecoder(np.zeros((2, 3), bool), np.zeros((2, 1), bool))  # the same syndrome twice
    with pytest.raises(ValueError):
        LookupDecoder(np.zeros((1, 3), bool), np.zeros((2, 1), bool))
    with pytest.raises(ValueError):
        LookupDecoder(np.zeros((1, 3), bool), np.zeros((1, 65), bool))
    dec = LookupDecoder(np.zeros((1, 3), bool), np.zeros((1, 1), bool))
    with pytest.raises(ValueError):
        dec.decode(np.zeros((4, 2), bool))
    rows = np.zeros((5, 4), bool)
    with pytest.raises(ValueError):
        LookupDecoder.from_counts(tally_rows(rows, num_detectors=3))                                # no patterns
    with pytest.raises(ValueError):
        LookupDecoder.from_counts(tally_rows(rows, num_detectors=3, pattern_columns="detectors"))   # not every column
    with pytest.raises(ValueError):
        tally_rows(rows, num_detectors=2, decoder=dec)                                              # 3 + 1 against 2 + 2
    empty = LookupDecoder.from_counts(tally_rows(np.zeros((0, 4), bool), num_detectors=3, pattern_columns="all"))
    assert len(empty) == 0 and empty.missed(np.zeros((2, 3), bool)).all()


def test_decoder_wide_syndromes_and_many_observables():
    rng = np.random.default_rng(2)
    nd, n_obs = 130, 64
    pool = rng.random((40, nd + n_obs)) < 0.3
    rows = pool[rng.integers(0, 40, 3000)]
    dec = LookupDecoder.from_counts(tally_rows(rows, num_detectors=nd, pattern_columns="all"))
    assert np.array_equal(dec.decode(pool[:, :nd]), pool[:, nd:])  # distinct random syndromes: each saw one observable pattern
    assert dec.table()[1].dtype == np.uint64 and dec.table()[0].shape == (len(dec), 17)
    assert int(dec.table()[1][0]) == int(np.packbits(dec.predictions[0], bitorder="little").view("<u8")[0])


# ---- samplers that never touch a device ---------------------------------------------------------------------------------

def oracle_sample_program(program, f_params, key):
    return O.sample_program(program, np.asarray(f_params), key)


@pytest.fixture
def oracle_seam(monkeypatch):
    monkeypatch.setattr(sampler_module, "sample_program", oracle_sample_program)


def random_bit_component(output_index, f_index=None):
    F = 0 if f_index is None else 1
    lv0 = scalar_graphs_from_terms(F, [dict()])
    lv1 = scalar_graphs_from_terms(F + 1, [dict(power2=-1)])
    fsel = np.zeros(0, np.int32) if f_index is None else np.asarray([f_index], np.int32)
    return CompiledComponent((output_index,), fsel, (lv0, lv1))


def det_sampler(seed=0):
    comps = [random_bit_component(2, f_index=0), random_bit_component(3)]
    prog = make_program(comps, [(0, 0, True), (1, 1, False), (4, 2, True)], 5, 3)
    return CompiledDetectorSampler(prog, channel_probs=[error_probs(0.3), error_probs(0.2), error_probs(0.4)],
                                   error_transform=np.eye(3, dtype=np.uint8), seed=seed)


def test_count_zero_shots_without_a_device(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was used")

    s = det_sampler()
    monkeypatch.setattr(s, "_hip", no_device)
    key, nkey = s._key, s._noise_key
    for sel, k in (("all", 5), ("detectors", 3), ((4, 0), 2)):
        got = s.count(0, pattern_columns=sel)
        assert got.patterns.shape == (0, k) and got.pattern_counts.shape == (0,) and got.pattern_overflow == 0
        assert len(got.pattern_columns) == k and got.decoded_errors is None
    plain = s.count(0)
    assert plain.patterns is None and plain.pattern_columns == ()
    dec = LookupDecoder(np.zeros((1, 3), bool), np.zeros((1, 2), bool))
    got = s.count(0, decoder=dec)
    assert (got.decoded_errors, got.decoder_misses) == (0, 0)
    for bad in ([5], [1, 1], [-1], "observables", np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            s.count(10, pattern_columns=bad)
    with pytest.raises(ValueError):
        s.count(10, pattern_columns="all", pattern_capacity=0)
    with pytest.raises(ValueError):
        s.count(10, decoder=LookupDecoder(np.zeros((1, 2), bool), np.zeros((1, 3), bool)))
    assert s._key == key and s._noise_key == nkey


@pytest.mark.parametrize("flags", [{}, dict(use_detector_reference_sample=True, use_observable_reference_sample=True)])
@pytest.mark.parametrize("mask", [None, np.array([False, True, False])])
@pytest.mark.parametrize("sel", ["all", "detectors", (4, 0, 2)])
def test_seam_count_pattern_columns(oracle_seam, flags, mask, sel):
    kw = dict(batch_size=16, postselection_mask=mask, **flags)
    a, b = det_sampler(seed=7), det_sampler(seed=7)
    rows = b.sample(100, append_observables=True, **kw)
    got = a.count(100, pattern_columns=sel, **kw)
    assert got == tally_rows(rows, num_detectors=3, postselection_mask=mask, histogram_columns=(3, 4), pattern_columns=sel)
    assert got.pattern_counts.sum() == got.kept and len(got.patterns) > 1
    np.testing.assert_array_equal(a.sample(40, batch_size=16, append_observables=True), b.sample(40, batch_size=16, append_observables=True))


def test_seam_count_decoder_and_overflow_warning(oracle_seam):
    train = det_sampler(seed=3).count(400, batch_size=64, pattern_columns="all")
    dec = LookupDecoder.from_counts(train)
    rows = det_sampler(seed=8).sample(300, batch_size=64, append_observables=True)
    got = det_sampler(seed=8).count(300, batch_size=64, decoder=dec)
    assert got.decoded_errors == int((dec.decode(rows[:, :3]) != rows[:, 3:]).any(axis=1).sum())
    assert got.decoder_misses == int(dec.missed(rows[:, :3]).sum())
    assert got.decoded_errors <= got.kept_with_observable_flip + got.decoder_misses
    with pytest.warns(RuntimeWarning, match="pattern_capacity=2"):
        small = det_sampler(seed=8).count(300, batch_size=64, pattern_columns="all", pattern_capacity=2)
    assert len(small.patterns) == 2 and small.pattern_overflow > 0 and small.pattern_counts.sum() + small.pattern_overflow == small.kept


def test_seam_measurement_count_pattern_columns(oracle_seam):
    prog = make_program([random_bit_component(0), random_bit_component(1, f_index=0), random_bit_component(2)], [], 3, 0)
    mk = lambda: CompiledMeasurementSampler(prog, channel_probs=[error_probs(0.3)],  # noqa: E731
                                            error_transform=np.array([[1]], np.uint8), seed=5)
    rows = mk().sample(77, batch_size=20)
    got = mk().count(77, batch_size=20, pattern_columns="all")
    assert got == tally_rows(rows, num_detectors=0, histogram_columns=(0, 1, 2), pattern_columns=(0, 1, 2))
    assert mk().count(77, batch_size=20).patterns is None
