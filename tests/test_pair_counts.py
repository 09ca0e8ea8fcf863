"""Pair counts on the CPU: the numpy statement (``tally_rows(pair_columns=...)``) against the direct product, batches,
ShotCounts equality, the selection's checks, the C entry point's argument errors without a device, the p_ij arithmetic
on exact moments, and the seam-replaced samplers, whose count(pair_columns=...) is the tally of sample()."""

import ctypes as C

import numpy as np
import pytest

import tsim_amd.sampler as sampler_module
from oracle import oracle_np as O
from tsim_amd import _lib, counts
from tsim_amd.channels import error_probs
from tsim_amd.counts import ShotCounts, check_pair_columns, pair_correlations_from_moments, tally_pairs_device, tally_rows
from tsim_amd.program import CompiledComponent, make_program, scalar_graphs_from_terms
from tsim_amd.sampler import CompiledDetectorSampler, CompiledMeasurementSampler


def direct_product(rows, cols, nd, mask=None, xor=None):
    v = rows ^ xor[None, :] if xor is not None else rows
    if mask is not None:
        v = v[~(v[:, :nd] & mask).any(axis=1)]
    B = v[:, list(cols)]
    return B.T.astype(np.int64) @ B.astype(np.int64)


# ---- the numpy statement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_tally_rows_pair_counts_match_the_direct_product(seed):
    rng = np.random.default_rng(seed)
    n, n_cols, nd = 500, 37, 30
    rows = rng.random((n, n_cols)) < 0.25
    ref = rng.random(n_cols) < 0.3  # a reference sample XORed in, as sample(use_*_reference_sample=True) does
    mask = rng.random(nd) < 0.1
    shuffled = tuple(int(c) for c in rng.permutation(n_cols)[:19])
    for data in (rows, rows ^ ref[None, :]):
        for m in (None, mask):
            for sel, cols in (("all", range(n_cols)), ("detectors", range(nd)), (shuffled, shuffled), ([n_cols - 1], [n_cols - 1])):
                got = tally_rows(data, num_detectors=nd, postselection_mask=m, pair_columns=sel)
                assert got.pair_columns == tuple(cols)
                assert got.pair_counts.dtype == np.int64 and got.pair_counts.shape == (len(got.pair_columns),) * 2
                np.testing.assert_array_equal(got.pair_counts, direct_product(data, cols, nd, m))
                np.testing.assert_array_equal(got.pair_counts, got.pair_counts.T)
                np.testing.assert_array_equal(np.diagonal(got.pair_counts), got.column_counts[list(cols)])
                assert got.pair_counts.max(initial=0) <= got.kept


def test_tally_rows_without_pair_columns_is_unchanged():
    rows = np.random.default_rng(1).random((50, 6)) < 0.5
    for sel in ((), None):
        got = tally_rows(rows, num_detectors=4, pair_columns=sel)
        assert got.pair_columns == () and got.pair_counts is None
        assert got == tally_rows(rows, num_detectors=4)


def test_host_tally_batches_accumulate():
    rng = np.random.default_rng(3)
    rows = rng.random((1000, 20)) < 0.3
    mask = np.zeros(15, bool)
    mask[[2, 9]] = True
    pc = (19, 0, 7, 15, 3)
    whole = counts._HostTally(20, 15, mask, (), pc)
    whole.add(rows)
    parts = counts._HostTally(20, 15, mask, (), pc)
    for lo, hi in ((0, 1), (1, 64), (64, 64), (64, 700), (700, 1000)):
        parts.add(rows[lo:hi])
    assert parts.result() == whole.result()
    np.testing.assert_array_equal(parts.result().pair_counts, direct_product(rows, pc, 15, mask))
    empty = counts._HostTally(20, 15, None, (), pc).result()
    assert empty.pair_counts.shape == (5, 5) and not empty.pair_counts.any()


def test_shot_counts_equality_sees_the_pair_counts():
    base = (10, 4, 1, np.array([1, 2, 3, 0, 1]), 3, (3, 4), np.array([2, 1, 0, 1]))
    seven = ShotCounts(*base)
    assert seven == ShotCounts(*base) and seven.pair_columns == () and seven.pair_counts is None
    p = np.array([[2, 1], [1, 3]])
    a = ShotCounts(*base, (1, 2), p)
    assert a == ShotCounts(*base, (1, 2), p.copy())
    assert a != ShotCounts(*base, (1, 2), np.array([[2, 0], [0, 3]]))
    assert a != ShotCounts(*base, (2, 1), p)
    assert a != seven and seven != a
    with pytest.raises(ValueError):
        seven.pair_correlations()


def test_check_pair_columns():
    assert check_pair_columns(None, 9, 7) == () and check_pair_columns((), 9, 7) == ()
    assert check_pair_columns("all", 9, 7) == tuple(range(9))
    assert check_pair_columns("detectors", 9, 7) == tuple(range(7))
    assert check_pair_columns(np.array([8, 0, 3]), 9, 7) == (8, 0, 3)
    assert check_pair_columns(range(4096), 5000, 10) == tuple(range(4096))
    for bad, n_cols in (([1, 1], 9), ([0, 9], 9), ([-1], 9), (list(range(4097)), 5000), (np.zeros((2, 2), np.int64), 9), ([0.5], 9),
                        ("some", 9)):
        with pytest.raises(ValueError):
            check_pair_columns(bad, n_cols, 7)
    with pytest.raises(ValueError, match="4097"):
        check_pair_columns(range(4097), 5000, 7)
    with pytest.raises(ValueError, match="5000"):
        check_pair_columns("all", 5000, 7)
    with pytest.raises(ValueError, match="4097"):
        check_pair_columns("detectors", 5000, 4097)


# ---- the library without a device ------------------------------------------------------------------------------

def test_pairs_create_checks_before_any_device_call():
    lib = _lib.load()

    def create(n_cols, cols, n_pair=None, out=True):
        a = np.asarray(cols, np.int32)
        h = C.c_void_p()
        rc = lib.tsim_pairs_create(0, n_cols, a.ctypes.data_as(C.c_void_p) if a.size else None, len(a) if n_pair is None else n_pair,
                                   C.byref(h) if out else None)
        assert h.value is None
        return rc

    for rc in (create(8, [], 0), create(8, [0], -1), create(5000, list(range(4097))),  # n_pair outside 1 .. 4096
               create(8, [0, 3, 0]), create(8, [7, 7]),                                 # duplicates
               create(8, [8]), create(8, [-1]), create(8, [1, 2, 100]),                  # not a column
               create(0, [0]), create(8, [], 3), create(8, [0], out=False)):             # no columns at all, NULL list, NULL out
        assert rc == -22
        assert _lib.last_error()
    assert lib.tsim_pairs_add_device(None, None, 0, 1, None, None, None) == -22
    assert lib.tsim_pairs_read(None, None, None) == -22
    assert lib.tsim_pairs_reset(None, None) == -22
    assert lib.tsim_pairs_info(None, None) == -22
    lib.tsim_pairs_destroy(None)


def test_tally_pairs_device_checks_arguments_on_the_host():
    for kw in (dict(n=-1), dict(n_cols=0), dict(row_bytes=1, n_cols=9), dict(pair_columns=[8]), dict(pair_columns=[1, 1]),
               dict(pair_columns=()), dict(pair_columns=list(range(4097)), n_cols=40000, row_bytes=5000)):
        args = dict(n=5, row_bytes=2, n_cols=8, pair_columns=[0, 1])
        args.update(kw)
        n = args.pop("n")
        with pytest.raises(ValueError):
            tally_pairs_device(0, n, **args)


# ---- the p_ij estimator ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pa,pb,pc", [(0.0, 0.0, 0.01), (0.01, 0.02, 0.005), (0.1, 0.2, 0.05), (0.3, 0.05, 0.2), (0.02, 0.02, 0.0),
                                      (0.001, 0.4, 1e-4)])
def test_moment_function_returns_the_shared_mechanism(pa, pb, pc):
    """x_i = a ^ c, x_j = b ^ c with independent a, b, c: the exact moments give p_c back."""
    odd = lambda p, q: p * (1 - q) + q * (1 - p)  # noqa: E731 - P(u ^ v = 1)
    xi, xj = odd(pa, pc), odd(pb, pc)
    # x_i x_j = 1: c = 0 and a = b = 1, or c = 1 and a = b = 0
    xij = (1 - pc) * pa * pb + pc * (1 - pa) * (1 - pb)
    p = pair_correlations_from_moments([xi, xj], [[xi, xij], [xij, xj]])
    assert p.shape == (2, 2) and p.dtype == np.float64
    assert np.isnan(p[0, 0]) and np.isnan(p[1, 1])
    assert abs(p[0, 1] - pc) <= 1e-12 and abs(p[1, 0] - pc) <= 1e-12


def test_moment_function_nan_cases():
    # perfectly correlated at 1/2: covariance 1/4, denominator 1 - 2 (1/2 + 1/2 - 1) = 1, radicand 0 -> not positive
    assert np.isnan(pair_correlations_from_moments([0.5, 0.5], [[0.5, 0.5], [0.5, 0.5]])[0, 1])
    # radicand negative: column 0 set only where column 1 is - covariance 0.12 over a denominator of 0.4
    xi, xj, xij = 0.3, 0.6, 0.3
    assert 1 - 2 * (xi + xj - 2 * xij) > 0 and 0.25 - (xij - xi * xj) / (1 - 2 * (xi + xj - 2 * xij)) < 0
    p = pair_correlations_from_moments([xi, xj], [[xi, xij], [xij, xj]])
    assert np.isnan(p[0, 1]) and np.isnan(p[1, 0])
    # denominator not positive: anticorrelated at 1/2
    assert np.isnan(pair_correlations_from_moments([0.5, 0.5], [[0.5, 0.0], [0.0, 0.5]])[0, 1])
    # independent columns: 0
    assert pair_correlations_from_moments([0.1, 0.3], [[0.1, 0.03], [0.03, 0.3]])[0, 1] == pytest.approx(0.0, abs=1e-15)
    with pytest.raises(ValueError):
        pair_correlations_from_moments([0.1, 0.2], [[0.1]])


def test_pair_correlations_of_counts():
    rng = np.random.default_rng(11)
    n = 200_000
    a, b, c = rng.random(n) < 0.05, rng.random(n) < 0.08, rng.random(n) < 0.03
    rows = np.stack([a ^ c, b ^ c, rng.random(n) < 0.1], axis=1)
    got = tally_rows(rows, num_detectors=3, pair_columns="all")
    p = got.pair_correlations()
    x = np.diagonal(got.pair_counts) / got.kept
    np.testing.assert_array_equal(p, pair_correlations_from_moments(x, got.pair_counts / got.kept))
    assert np.isnan(np.diagonal(p)).all() and np.array_equal(p[0, 1], p[1, 0])
    assert abs(p[0, 1] - 0.03) < 5e-3 and abs(p[0, 2]) < 5e-3
    none_kept = tally_rows(rows[:10], num_detectors=3, postselection_mask=np.ones(3, bool), pair_columns="all")
    if none_kept.kept == 0:
        assert np.isnan(none_kept.pair_correlations()).all()


# ---- the seam-replaced samplers ------------------------------------------------------------------------------------

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


@pytest.mark.parametrize("flags", [{}, dict(use_detector_reference_sample=True, use_observable_reference_sample=True)])
@pytest.mark.parametrize("mask", [None, np.array([False, True, False])])
@pytest.mark.parametrize("sel", ["all", "detectors", (4, 0, 2)])
def test_seam_count_pair_columns(oracle_seam, flags, mask, sel):
    kw = dict(batch_size=16, postselection_mask=mask, **flags)
    a, b = det_sampler(seed=7), det_sampler(seed=7)
    rows = b.sample(100, append_observables=True, **kw)
    got = a.count(100, pair_columns=sel, **kw)
    assert got == tally_rows(rows, num_detectors=3, postselection_mask=mask, histogram_columns=(3, 4), pair_columns=sel)
    assert got.pair_counts is not None and got.pair_counts.any()
    np.testing.assert_array_equal(a.sample(40, batch_size=16, append_observables=True), b.sample(40, batch_size=16, append_observables=True))
    zero = det_sampler(seed=7).count(0, pair_columns=sel, **kw)
    assert zero.pair_columns == got.pair_columns and not zero.pair_counts.any()


def test_seam_measurement_count_pair_columns(oracle_seam):
    prog = make_program([random_bit_component(0), random_bit_component(1, f_index=0), random_bit_component(2)], [], 3, 0)
    mk = lambda: CompiledMeasurementSampler(prog, channel_probs=[error_probs(0.3)],  # noqa: E731
                                            error_transform=np.array([[1]], np.uint8), seed=5)
    rows = mk().sample(77, batch_size=20)
    got = mk().count(77, batch_size=20, pair_columns="all")
    assert got == tally_rows(rows, num_detectors=0, histogram_columns=(0, 1, 2), pair_columns=(0, 1, 2))
    assert mk().count(77, batch_size=20).pair_counts is None


def test_count_rejects_bad_pair_columns_before_any_device_call(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was used")

    s = det_sampler()
    monkeypatch.setattr(s, "_hip", no_device)
    key, nkey = s._key, s._noise_key
    for bad in ([5], [1, 1], [-1], "observables", np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            s.count(10, pair_columns=bad)
    assert s._key == key and s._noise_key == nkey
