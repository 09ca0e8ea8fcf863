"""``tally_rows(..., decoder=, corrected=True)`` without a device: the numpy statement of corrected observables
(``tsim_amd.counts``) against rows corrected by hand, its invariants against the uncorrected tally, a lookup decoder with several
observables, and what is refused."""

import dataclasses

import numpy as np
import pytest

from test_unionfind import memory

from tsim_amd import faults
from tsim_amd.counts import ShotCounts, tally_rows
from tsim_amd.decode import LookupDecoder, UnionFindDecoder

_CACHE: dict = {}


def d3_rows():
    """``(decoder, rows)``: d = 3 memory at p = 0.02, 4133 rows of ``fault_rows_host`` under key (1, 2)."""
    if not _CACHE:
        c = memory(3, 0.02)
        _CACHE["d3"] = (UnionFindDecoder.from_circuit(c), faults.fault_rows_host(c.compile_faults(), 0, 4133, (1, 2)).view(np.bool_))
    return _CACHE["d3"]


def corrected_by_hand(dec, rows, mask):
    """The rows whose kept shots had ``obs ^= dec.decode(dets)`` applied."""
    nd = dec.num_detectors
    out = rows.copy()
    keep = np.ones(len(rows), np.bool_) if mask is None else ~(rows[:, :nd] & mask).any(axis=1)
    out[keep, nd:] ^= dec.decode(rows[keep, :nd])
    return out


@pytest.mark.parametrize("masked", [False, True])
def test_corrected_equals_the_tally_of_rows_corrected_by_hand(masked):
    uf, rows = d3_rows()
    nd = uf.num_detectors
    mask = None
    if masked:
        mask = np.zeros(nd, np.bool_)
        mask[[0, 13]] = True
    kw = dict(num_detectors=nd, postselection_mask=mask, histogram_columns=(nd,), pair_columns=(2, nd), pattern_columns=(5, nd))
    before = rows.copy()
    got = tally_rows(rows, decoder=uf, corrected=True, **kw)
    assert np.array_equal(rows, before), "the caller's rows are not changed"
    plain = tally_rows(rows, decoder=uf, **kw)
    by_hand = tally_rows(corrected_by_hand(uf, rows, mask), **kw)
    assert got.corrected and not plain.corrected
    # everything but the decoder's own counts is the tally of the corrected rows
    assert dataclasses.replace(got, decoded_errors=None, decoder_misses=None, corrected=False) == by_hand
    # the invariants against the same call without corrected
    assert 0 < plain.decoded_errors < plain.kept_with_observable_flip, "the case is not vacuous"
    assert got.kept_with_observable_flip == got.decoded_errors == plain.decoded_errors
    assert (got.kept, got.decoder_misses) == (plain.kept, plain.decoder_misses)
    assert np.array_equal(got.detector_counts, plain.detector_counts)
    assert int(got.observable_counts[0]) == got.decoded_errors  # (one observable: still flipped = decoded wrongly)
    assert int(got.histogram[1]) == got.decoded_errors and int(got.histogram[0]) == got.kept - got.decoded_errors
    assert (0 < got.kept < len(rows)) == masked


def test_soft_output_counts_do_not_change():
    uf, rows = d3_rows()
    soft = uf.with_soft_output("largest_cluster", 16)
    nd = uf.num_detectors
    plain = tally_rows(rows, num_detectors=nd, decoder=soft)
    got = tally_rows(rows, num_detectors=nd, decoder=soft, corrected=True)
    assert got.soft_output == "largest_cluster" and np.array_equal(got.soft_kept, plain.soft_kept)
    assert np.array_equal(got.soft_errors, plain.soft_errors) and int(got.soft_errors.sum()) == got.kept_with_observable_flip


def test_lookup_decoder_with_three_observables():
    """Synthetic rows: 6 detectors and 3 observables that are noisy functions of them; trained on one half by
    ``tally_rows(pattern_columns="all")``, applied to the other half."""
    rng = np.random.default_rng(3)
    n, nd, n_obs = 6000, 6, 3
    dets = rng.random((n, nd)) < 0.25
    obs = np.stack([dets[:, 0] ^ dets[:, 1], dets[:, 2] & dets[:, 3], dets[:, 4] | dets[:, 5]], axis=1) ^ (rng.random((n, n_obs)) < 0.1)
    rows = np.concatenate([dets, obs], axis=1)
    train, apply = rows[: n // 2], rows[n // 2:]
    dec = LookupDecoder.from_counts(tally_rows(train, num_detectors=nd, pattern_columns="all"))
    assert dec.num_observables == 3
    hc = tuple(range(nd, nd + n_obs))
    got = tally_rows(apply, num_detectors=nd, decoder=dec, corrected=True, histogram_columns=hc)
    left = apply[:, nd:] ^ dec.decode(apply[:, :nd])  # the residual flips, in numpy
    assert np.array_equal(got.observable_counts, left.sum(axis=0))
    assert np.array_equal(got.histogram, np.bincount((left * (1 << np.arange(n_obs))).sum(axis=1), minlength=8))
    assert got.kept == len(apply) and int(got.histogram[0]) == got.kept - got.decoded_errors
    assert got.decoded_errors == int(left.any(axis=1).sum()) > 0 and len(set(got.observable_counts.tolist())) > 1


def test_corrected_without_a_decoder_raises():
    _, rows = d3_rows()
    with pytest.raises(ValueError, match="decoder"):
        tally_rows(rows, num_detectors=24, corrected=True)


def test_counts_with_different_corrected_compare_unequal():
    a = ShotCounts(4, 4, 1, np.array([1, 1]), 1, (), np.array([4]))
    assert a.corrected is False and a == dataclasses.replace(a)
    assert a != dataclasses.replace(a, corrected=True)
    assert dataclasses.fields(ShotCounts)[-1].name == "corrected"
