"""count() and the tally kernel (tsim_tally_rows_device) on the device: the kernel bit-exact against numpy over widths,
strides, masks, histograms and counter carries; the samplers' count() equal to the tally of what sample() returns for
the same seed and arguments, with the keys left where sample() leaves them."""

import warnings

import numpy as np
import pytest

from tsim_amd import synth
from tsim_amd.backend import HipProgram
from tsim_amd.channels import error_probs
from tsim_amd.circuits import rotated_surface_code_memory
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.counts import ShotCounts, counters_length, tally_rows, tally_rows_device
from tsim_amd.sampler import CompiledDetectorSampler

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def numpy_tally(bits, xor, test, obs, hist):
    v = bits ^ xor[None, :] if xor is not None else bits
    keep = ~(v & test[None, :]).any(axis=1) if test is not None else np.ones(len(v), bool)
    k = v[keep]
    idx = np.zeros(len(k), np.int64)
    for i, c in enumerate(hist):
        idx |= k[:, c].astype(np.int64) << i
    out = np.zeros(counters_length(bits.shape[1], len(hist)), np.uint64)
    out[0] = keep.sum()
    out[1] = k[:, obs[0]:obs[1]].any(axis=1).sum()
    out[2:2 + bits.shape[1]] = k.sum(axis=0)
    out[2 + bits.shape[1]:] = np.bincount(idx, minlength=1 << len(hist))
    return out


def device_tally(hp, rows_bytes, n, row_bytes, n_cols, *, xor=None, test=None, obs=(0, 0), hist=(), prefill=None, calls=1):
    bufs = []

    def up(a):
        b = hp.malloc(max(16, a.nbytes + 16))
        bufs.append(b)
        if a.nbytes:
            hp.h2d(b, a)
        return b

    try:
        d_rows = up(rows_bytes)
        d_xor = up(np.packbits(xor, bitorder="little")) if xor is not None else None
        d_test = up(np.packbits(test, bitorder="little")) if test is not None else None
        init = np.zeros(counters_length(n_cols, len(hist)), np.uint64) if prefill is None else prefill
        d_c = up(init)
        for _ in range(calls):
            hp.tally_rows_device(d_rows.ptr, n, row_bytes, n_cols, d_c.ptr, d_xor=d_xor.ptr if d_xor else 0,
                                 d_test=d_test.ptr if d_test else 0, observables=obs, histogram_columns=hist)
        out = np.zeros_like(init)
        hp.d2h(out, d_c)
        return out
    finally:
        for b in bufs:
            b.free()


def packed_rows(bits, row_bytes, rng):
    n, n_cols = bits.shape
    rows = np.zeros((n, row_bytes), np.uint8)
    p = np.packbits(bits, axis=1, bitorder="little")
    rows[:, :p.shape[1]] = p
    if n_cols % 8:  # garbage in the pad bits of the last byte and in the padding bytes: never counted
        rows[:, p.shape[1] - 1] |= rng.integers(0, 256, n).astype(np.uint8) & np.uint8((0xFF << (n_cols % 8)) & 0xFF)
    rows[:, p.shape[1]:] = rng.integers(0, 256, (n, row_bytes - p.shape[1]))
    return rows


def hist_columns(n_cols, k):
    """k distinct columns around the 64-bit word boundaries (and the last column)."""
    cand = []
    for c in [0, 63, 64, 1, 127, 128, 62, 65, 2047, 2048, 5, 4095, 4096, 9, 191, 192, 8000, 200, 13]:
        if c < n_cols and c not in cand:
            cand.append(c)
    if n_cols - 1 not in cand:
        cand.insert(1, n_cols - 1)
    for c in range(n_cols):
        if len(cand) >= k:
            break
        if c not in cand:
            cand.append(c)
    return tuple(cand[:k])


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 2047, 2048, 2049, 9300])
@pytest.mark.parametrize("padded", [False, True])
def test_kernel_matches_numpy(hp, n_cols, padded):
    rng = np.random.default_rng(n_cols + padded)
    n = 1000
    bits = rng.random((n, n_cols)) < 0.3
    bits[rng.random(n) < 0.3] = False  # all-zero rows
    used = (n_cols + 7) // 8
    row_bytes = (used + 7) // 8 * 8 + (8 if padded else 0) if padded else used
    rows = packed_rows(bits, row_bytes, rng)
    nd = max(0, n_cols - 3)
    obs = (nd, n_cols)
    xor = rng.random(n_cols) < 0.2
    test = np.zeros(n_cols, bool)
    test[rng.choice(n_cols, size=min(n_cols, 3), replace=False)] = True
    for use_xor in (False, True):
        for use_test in (False, True):
            for k in (0, 1, 5, 16):
                if k > n_cols:
                    continue
                hist = hist_columns(n_cols, k)
                x, t = (xor if use_xor else None), (test if use_test else None)
                got = device_tally(hp, rows, n, row_bytes, n_cols, xor=x, test=t, obs=obs, hist=hist)
                np.testing.assert_array_equal(got, numpy_tally(bits, x, t, obs, hist), err_msg=f"xor={use_xor} test={use_test} k={k}")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1_000_003])
def test_kernel_row_counts(hp, n):
    rng = np.random.default_rng(n)
    n_cols = 130
    bits = rng.random((n, n_cols)) < 0.05
    rows = packed_rows(bits, 24, rng)
    test = np.zeros(n_cols, bool)
    test[[3, 70]] = True
    hist = (127, 128, 129, 0, 64)
    got = device_tally(hp, rows, n, 24, n_cols, test=test, obs=(120, 130), hist=hist)
    np.testing.assert_array_equal(got, numpy_tally(bits, None, test, (120, 130), hist))


def test_all_zero_rows_land_in_one_bin(hp):
    """10^6 + 3 empty rows: every lane of every wave in bin 0 (the contention case), 16 columns (bins in global memory)
    and 5 columns (bins in LDS)."""
    n, n_cols = 1_000_003, 64
    rows = np.zeros((n, 8), np.uint8)
    for hist in (tuple(range(16)), (0, 7, 8, 62, 63)):
        got = device_tally(hp, rows, n, 8, n_cols, obs=(60, 64), hist=hist)
        assert got[0] == n and got[1] == 0 and not got[2:2 + n_cols].any()
        assert got[2 + n_cols] == n and not got[3 + n_cols:].any()


def test_counters_accumulate_and_carry(hp):
    rng = np.random.default_rng(5)
    n, n_cols = 70_001, 200
    bits = rng.random((n, n_cols)) < 0.5
    rows = packed_rows(bits, 25, rng)  # odd stride: byte staging
    hist = (0, 100, 199)
    once = numpy_tally(bits, None, None, (190, 200), hist)
    twice = device_tally(hp, rows, n, 25, n_cols, obs=(190, 200), hist=hist, calls=2)
    np.testing.assert_array_equal(twice, 2 * once)
    for base in (np.uint64(2**32 - 7), np.uint64(2**63 - 11)):
        pre = np.full(counters_length(n_cols, len(hist)), base, np.uint64)
        got = device_tally(hp, rows, n, 25, n_cols, obs=(190, 200), hist=hist, prefill=pre)
        np.testing.assert_array_equal(got, pre + once)


def test_public_tally_rows_device(hp):
    rng = np.random.default_rng(9)
    n, n_cols = 5000, 70
    bits = rng.random((n, n_cols)) < 0.1
    rows = packed_rows(bits, 16, rng)
    d_rows, d_c = hp.malloc(rows.nbytes), hp.malloc(8 * counters_length(n_cols, 2))
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_c, np.zeros(counters_length(n_cols, 2), np.uint64))
        tally_rows_device(d_rows.ptr, n, row_bytes=16, n_cols=n_cols, d_counts=d_c.ptr, observables=(68, 70),
                          histogram_columns=(68, 69), device=hp.device, stream=hp.stream_ptr())
        out = np.zeros(counters_length(n_cols, 2), np.uint64)
        hp.d2h(out, d_c)
    finally:
        d_rows.free()
        d_c.free()
    got = ShotCounts.from_counters(out, shots=n, n_cols=n_cols, num_detectors=68, histogram_columns=(68, 69))
    assert got == tally_rows(bits, num_detectors=68, histogram_columns=(68, 69))


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


DEPENDENT = """
    R 0 1 2
    X 2
    X_ERROR(0.2) 0
    X_ERROR(0.3) 1
    M 0 1 2
    DETECTOR rec[-3]
    DETECTOR rec[-2]
    DETECTOR rec[-3] rec[-2]
    DETECTOR rec[-1]
    DETECTOR rec[-3] rec[-2] rec[-1]
    OBSERVABLE_INCLUDE(1) rec[-3]
"""

DISTILL5 = """
    R 0 1 2 3 4
    H 0 1 2
    CX 0 3 1 3 2 4 0 4
    DEPOLARIZE1(0.05) 0 1 2 3 4
    CX 3 1 4 2
    X_ERROR(0.1) 3 4
    M 0 1 2 3 4
"""

FLAGS = [{}, dict(use_detector_reference_sample=True), dict(use_observable_reference_sample=True),
         dict(use_detector_reference_sample=True, use_observable_reference_sample=True)]


def masks_for(s):
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


def check_detector_count(mk, shots, batch_size, flags, mask, hist=None):
    kw = dict(batch_size=batch_size, postselection_mask=mask, **flags)
    a, b = mk(), mk()
    rows = b.sample(shots, append_observables=True, **kw)
    nd = b._num_detectors
    got = a.count(shots, histogram_columns=hist, **kw)
    from tsim_amd.counts import default_histogram_columns

    hc = default_histogram_columns(nd, rows.shape[1]) if hist is None else tuple(hist)
    want = tally_rows(rows, num_detectors=nd, postselection_mask=mask, histogram_columns=hc)
    assert got == want, (got, want)
    return a, b


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("flags", FLAGS)
def test_c2_count_equals_tally_of_sample(hip, noise, flags):
    mk = c2_maker(noise)
    for mask in masks_for(mk()):
        check_detector_count(mk, 250_001, 100_000, flags, mask)
    check_detector_count(mk, 0, None, flags, None)


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("flags", [FLAGS[0], FLAGS[3]])
def test_surface_code_count_equals_tally_of_sample(hip, noise, flags):
    """d = 5 rotated surface code: no compiled component, the direct-output path."""
    mk = clifford_maker(rotated_surface_code_memory(5, 5, after_clifford_depolarization=2e-3, before_measure_flip_probability=1e-3),
                        noise)
    s = mk()
    assert not s._program.components
    mask = np.zeros(s._num_detectors, bool)
    mask[::5] = True
    for m in (None, mask):
        check_detector_count(mk, 70_001, 30_000, flags, m, hist=[0, 63, 64, 65, s._num_detectors])
    check_detector_count(mk, 0, None, flags, mask)


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("flags", FLAGS)
def test_dependent_detectors_count_equals_tally_of_sample(hip, noise, flags):
    mk = clifford_maker(DEPENDENT, noise)
    s = mk()
    assert s._program.components
    for mask in masks_for(s):
        check_detector_count(mk, 40_003, 16_384, flags, mask, hist=[0, 2, 4, 5])
    check_detector_count(mk, 0, 16_384, flags, None)


@pytest.mark.parametrize("noise", ["host", "device"])
def test_measurement_count_histogram_of_five_measurements(hip, noise):
    mk = clifford_maker(DISTILL5, noise, measurement=True)
    for shots, bs in ((60_001, 16_384), (0, None)):
        s = mk()
        rows = s.sample(shots, batch_size=bs)
        got = mk().count(shots, batch_size=bs, histogram_columns=range(5))
        assert rows.shape[1] == 5 and got.histogram_columns == (0, 1, 2, 3, 4)
        assert got == tally_rows(rows, num_detectors=s._num_detectors, histogram_columns=(0, 1, 2, 3, 4))


@pytest.mark.parametrize("noise", ["host", "device"])
def test_keys_continue_after_count(hip, noise):
    """count(); sample() gives the second call's rows of sample(); sample() - on the plain, reference and masked paths."""
    mk = c2_maker(noise)
    s = mk()
    mask = masks_for(s)[1]
    for kw in ({}, dict(use_detector_reference_sample=True), dict(postselection_mask=mask, use_observable_reference_sample=True)):
        a, b = mk(), mk()
        a.count(120_001, batch_size=50_000, **kw)
        b.sample(120_001, batch_size=50_000, append_observables=True, **kw)
        np.testing.assert_array_equal(a.sample(30_000, batch_size=50_000, append_observables=True, **kw),
                                      b.sample(30_000, batch_size=50_000, append_observables=True, **kw))
