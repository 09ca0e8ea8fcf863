"""count() on the CPU: argument checks before any device call, ShotCounts, the numpy statement of the tally, the C entry
point's own checks, and the seam-replaced samplers (``tsim_amd.sampler.sample_program`` bound to the numpy oracle),
whose count() must equal the tally of what sample() returns."""

import ctypes as C
import math

import numpy as np
import pytest

import tsim_amd.sampler as sampler_module
from oracle import oracle_np as O
from tsim_amd import _lib, counts
from tsim_amd.channels import error_probs
from tsim_amd.counts import ShotCounts, counters_length, tally_rows, tally_rows_device
from tsim_amd.program import CompiledComponent, make_program, scalar_graphs_from_terms
from tsim_amd.sampler import CompiledDetectorSampler, CompiledMeasurementSampler


def oracle_sample_program(program, f_params, key):
    return O.sample_program(program, np.asarray(f_params), key)


def random_bit_component(output_index, f_index=None):
    F = 0 if f_index is None else 1
    lv0 = scalar_graphs_from_terms(F, [dict()])
    lv1 = scalar_graphs_from_terms(F + 1, [dict(power2=-1)])
    fsel = np.zeros(0, np.int32) if f_index is None else np.asarray([f_index], np.int32)
    return CompiledComponent((output_index,), fsel, (lv0, lv1))


def det_sampler(seed=0, flip=False, p=0.3):
    """det0 = f0 (direct, optionally flipped), det1 = f1 (direct), det2 a compiled random bit depending on f0, obs0 a
    compiled random bit, obs1 = f2 (direct, flipped)."""
    comps = [random_bit_component(2, f_index=0), random_bit_component(3)]
    prog = make_program(comps, [(0, 0, flip), (1, 1, False), (4, 2, True)], 5, 3)
    return CompiledDetectorSampler(prog, channel_probs=[error_probs(p), error_probs(0.2), error_probs(0.4)],
                                   error_transform=np.eye(3, dtype=np.uint8), seed=seed)


def no_device(*_a, **_k):
    raise AssertionError("the device was used")


# ---- argument checks ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs", [
    dict(shots=-1),
    dict(shots=10, batch_size=0),
    dict(shots=10, postselection_mask=np.zeros(2, bool)),
    dict(shots=10, postselection_mask=np.zeros((3, 1), bool)),
    dict(shots=10, histogram_columns=[5]),
    dict(shots=10, histogram_columns=[-1]),
    dict(shots=10, histogram_columns=[1, 1]),
    dict(shots=10, histogram_columns=list(range(17))),
    dict(shots=10, histogram_columns=[0.5]),
])
def test_count_rejects_bad_arguments_before_any_device_call(monkeypatch, kwargs):
    s = det_sampler()
    monkeypatch.setattr(s, "_hip", no_device)
    key, nkey = s._key, s._noise_key
    with pytest.raises(ValueError):
        s.count(**kwargs)
    assert s._key == key and s._noise_key == nkey


def test_measurement_count_rejects_bad_arguments(monkeypatch):
    prog = make_program([random_bit_component(0), random_bit_component(1)], [], 2, 0)
    s = CompiledMeasurementSampler(prog, channel_probs=[], error_transform=np.zeros((0, 0), np.uint8), seed=1)
    monkeypatch.setattr(s, "_hip", no_device)
    for kw in (dict(shots=-3), dict(shots=4, histogram_columns=[2]), dict(shots=4, histogram_columns=[0, 0])):
        with pytest.raises(ValueError):
            s.count(**kw)


def test_tally_rows_device_checks_arguments_on_the_host():
    for kw in (dict(n=-1), dict(n_cols=0), dict(row_bytes=1, n_cols=9), dict(observables=(3, 2)), dict(observables=(0, 99)),
               dict(histogram_columns=[8]), dict(histogram_columns=[1, 1])):
        args = dict(n=5, row_bytes=2, n_cols=8, d_counts=0)
        args.update(kw)
        n = args.pop("n")
        with pytest.raises(ValueError):
            tally_rows_device(0, n, **args)
    tally_rows_device(0, 0, row_bytes=1, n_cols=8, d_counts=0)  # n == 0: nothing to do, nothing called


def test_c_entry_point_checks_before_any_launch():
    lib = _lib.load()
    counters = np.zeros(counters_length(8, 1), np.uint64)
    p = counters.ctypes.data_as(C.c_void_p)
    hc = np.array([1, 1], np.int32)
    fake = C.c_void_p(0x1000)
    bad = [
        (0, fake, -1, 1, 8, None, None, 0, 0, None, 0, p, None),
        (0, fake, 4, 0, 8, None, None, 0, 0, None, 0, p, None),   # row_bytes < ceil(n_cols / 8)
        (0, fake, 4, 1, 0, None, None, 0, 0, None, 0, p, None),   # n_cols = 0
        (0, fake, 4, 1, 8, None, None, 5, 4, None, 0, p, None),   # observables backwards
        (0, fake, 4, 1, 8, None, None, 0, 0, hc.ctypes.data_as(C.c_void_p), 2, p, None),  # duplicate column
        (0, fake, 4, 1, 8, None, None, 0, 0, None, 17, p, None),  # too many columns
        (0, fake, 4, 1, 8, None, None, 0, 0, None, 0, None, None),  # no counters
        (0, None, 4, 1, 8, None, None, 0, 0, None, 0, p, None),   # no rows
    ]
    for args in bad:
        assert lib.tsim_tally_rows_device(*args) == -22
        assert _lib.last_error()
    assert lib.tsim_tally_rows_device(0, None, 0, 1, 8, None, None, 0, 8, None, 0, p, None) == 0


# ---- ShotCounts and the numpy statement ----------------------------------------------------------------------

def test_shot_counts_properties():
    c = ShotCounts(10, 4, 1, np.array([1, 2, 3, 0, 1]), 3, (3, 4), np.array([2, 1, 0, 1]))
    assert c.detector_counts.tolist() == [1, 2, 3]
    assert c.observable_counts.tolist() == [0, 1]
    assert c.kept_fraction == 0.4
    assert math.isnan(ShotCounts(0, 0, 0, np.zeros(5), 3, (), np.zeros(1)).kept_fraction)
    same = ShotCounts(10, 4, 1, np.array([1, 2, 3, 0, 1]), 3, (3, 4), np.array([2, 1, 0, 1]))
    assert c == same and not c != same
    assert c != ShotCounts(10, 4, 1, np.array([1, 2, 3, 0, 2]), 3, (3, 4), np.array([2, 1, 0, 1]))
    raw = np.array([4, 1, 1, 2, 3, 0, 1, 2, 1, 0, 1], np.uint64)
    assert ShotCounts.from_counters(raw, shots=10, n_cols=5, num_detectors=3, histogram_columns=(3, 4)) == same
    with pytest.raises(ValueError):
        ShotCounts.from_counters(raw[:-1], shots=10, n_cols=5, num_detectors=3, histogram_columns=(3, 4))


def brute_force(rows, nd, mask, hist):
    kept = obs = 0
    cols = np.zeros(rows.shape[1], np.int64)
    bins = np.zeros(1 << len(hist), np.int64)
    for r in rows:
        if mask is not None and any(r[j] and mask[j] for j in range(nd)):
            continue
        kept += 1
        obs += bool(r[nd:].any())
        cols += r
        bins[sum(int(r[c]) << i for i, c in enumerate(hist))] += 1
    return kept, obs, cols, bins


@pytest.mark.parametrize("seed", range(4))
def test_tally_rows_matches_a_loop(seed):
    rng = np.random.default_rng(seed)
    n, n_cols = int(rng.integers(0, 300)), int(rng.integers(1, 40))
    nd = int(rng.integers(0, n_cols + 1))
    rows = rng.random((n, n_cols)) < 0.2
    mask = (rng.random(nd) < 0.3) if seed % 2 else None
    hist = tuple(int(c) for c in rng.choice(n_cols, size=min(n_cols, int(rng.integers(0, 6))), replace=False))
    got = tally_rows(rows, num_detectors=nd, postselection_mask=mask, histogram_columns=hist)
    kept, obs, cols, bins = brute_force(rows, nd, mask, hist)
    assert (got.shots, got.kept, got.kept_with_observable_flip) == (n, kept, obs)
    assert got.column_counts.tolist() == cols.tolist() and got.histogram.tolist() == bins.tolist()
    assert got.histogram.sum() == kept


# ---- the seam-replaced samplers: count() is the tally of sample() ---------------------------------------------

@pytest.fixture
def oracle_seam(monkeypatch):
    monkeypatch.setattr(sampler_module, "sample_program", oracle_sample_program)


FLAGS = [{}, dict(use_detector_reference_sample=True), dict(use_observable_reference_sample=True),
         dict(use_detector_reference_sample=True, use_observable_reference_sample=True)]
MASKS = [None, np.array([True, False, False]), np.array([False, False, True]), np.array([True, True, True])]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("mask_i", range(len(MASKS)))
@pytest.mark.parametrize("shots,batch_size", [(0, None), (37, 8), (50, None)])
def test_seam_count_equals_tally_of_sample(oracle_seam, flags, mask_i, shots, batch_size):
    mask = MASKS[mask_i]
    kw = dict(batch_size=batch_size, postselection_mask=mask, **flags)
    rows = det_sampler(seed=7, flip=True).sample(shots, append_observables=True, **kw)
    want = tally_rows(rows, num_detectors=3, postselection_mask=mask, histogram_columns=(3, 4))
    got = det_sampler(seed=7, flip=True).count(shots, **kw)
    assert got == want
    assert got.histogram_columns == (3, 4)  # the observables, by default
    if shots and mask is None:
        assert got.kept == shots


def test_seam_count_histogram_columns_and_key_continuity(oracle_seam):
    kw = dict(batch_size=16, postselection_mask=np.array([False, True, False]), use_detector_reference_sample=True)
    a, b = det_sampler(seed=3), det_sampler(seed=3)
    got = a.count(100, histogram_columns=[4, 0, 2], **kw)
    rows = b.sample(100, append_observables=True, **kw)
    assert got == tally_rows(rows, num_detectors=3, postselection_mask=kw["postselection_mask"], histogram_columns=(4, 0, 2))
    # the keys stand where sample() left them: the next call agrees row for row
    np.testing.assert_array_equal(a.sample(40, batch_size=16, append_observables=True),
                                  b.sample(40, batch_size=16, append_observables=True))


def test_seam_measurement_count(oracle_seam):
    prog = make_program([random_bit_component(0), random_bit_component(1, f_index=0), random_bit_component(2)], [], 3, 0)
    mk = lambda: CompiledMeasurementSampler(prog, channel_probs=[error_probs(0.3)],  # noqa: E731
                                            error_transform=np.array([[1]], np.uint8), seed=5)
    rows = mk().sample(77, batch_size=20)
    got = mk().count(77, batch_size=20)
    assert got == tally_rows(rows, num_detectors=0, histogram_columns=(0, 1, 2))
    assert got.kept == 77 and got.histogram.sum() == 77


def test_count_without_components_on_host(oracle_seam):
    """A program with no compiled component (direct outputs only) - the Clifford-only surface codes - tallied on the host
    path when the seam is replaced."""
    prog = make_program([], [(0, 0, False), (1, 1, True), (2, 2, False)], 3, 2)
    mk = lambda: CompiledDetectorSampler(prog, channel_probs=[error_probs(0.3)] * 3,  # noqa: E731
                                         error_transform=np.eye(3, dtype=np.uint8), seed=2)
    for kw in ({}, dict(postselection_mask=np.array([True, False]), use_detector_reference_sample=True)):
        rows = mk().sample(64, append_observables=True, **kw)
        assert mk().count(64, **kw) == tally_rows(rows, num_detectors=2, postselection_mask=kw.get("postselection_mask"),
                                                  histogram_columns=(2,))


def test_default_histogram_columns():
    assert counts.default_histogram_columns(3, 5) == (3, 4)
    assert counts.default_histogram_columns(3, 3) == ()
    assert counts.default_histogram_columns(0, 17) == ()
    assert counts.default_histogram_columns(0, 16) == tuple(range(16))
