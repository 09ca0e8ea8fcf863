"""Corrected observables on the GPU: ``count(decoder=..., corrected=True)`` of every decoder against the numpy statement
(``tally_rows(..., corrected=True)``) of the same seeded ``sample()``, the default path next to it, and ``decode_file``:
recorded shots to a predictions file, bit for bit against ``decode``."""

import os

import numpy as np
import pytest

from test_unionfind import memory
from test_unionfind_erasure import erasure_memory
from test_unionfind_windowed import long_memory

from tsim_amd import faults, shotdata, synth
from tsim_amd.backend import HipProgram
from tsim_amd.counts import tally_rows
from tsim_amd.decode import DecodeFileResult, LookupDecoder, UnionFindDecoder, WindowedUnionFindDecoder

pytestmark = pytest.mark.gpu

SHOTS = 20000
_ROWS: dict = {}


@pytest.fixture(scope="module")
def hp(hip):
    return HipProgram(synth.kat_h_m())


def d3():
    """``(circuit, its sample(20000) under seed 5 by method="faults")``, computed once and left unchanged."""
    if "d3" not in _ROWS:
        c = memory(3, 0.01)
        rows = c.compile_detector_sampler(seed=5, method="faults").sample(SHOTS, append_observables=True)
        rows.setflags(write=False)
        _ROWS["d3"] = (c, rows)
    return _ROWS["d3"]


def check(c, dec, rows=None, *, seed=5, mask=None, **sampler_kw):
    """``count(corrected=True)`` of a fresh sampler == the numpy statement over ``sample()`` of another fresh sampler with the
    same seed; returns both results of the device (corrected, plain)."""
    nd = dec.num_detectors
    if rows is None:
        rows = c.compile_detector_sampler(seed=seed, **sampler_kw).sample(SHOTS, append_observables=True)
    kw = {} if mask is None else dict(postselection_mask=mask)
    got = c.compile_detector_sampler(seed=seed, **sampler_kw).count(SHOTS, decoder=dec, corrected=True, **kw)
    want = tally_rows(rows, num_detectors=nd, decoder=dec, corrected=True, histogram_columns=tuple(range(nd, rows.shape[1])), **kw)
    print(f"kept {got.kept}, decoded errors {got.decoded_errors}, misses {got.decoder_misses}, observables left {got.observable_counts.tolist()}")
    assert got == want
    assert got.corrected and got.kept_with_observable_flip == got.decoded_errors
    return got


def detector_mask(nd: int, *cols) -> np.ndarray:
    mask = np.zeros(nd, np.bool_)
    mask[list(cols)] = True
    return mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("weights", [None, "probability"])
def test_union_find_plain_and_weighted(hip, weights, masked):
    c, rows = d3()
    uf = UnionFindDecoder.from_circuit(c, weights=weights)
    mask = detector_mask(uf.num_detectors, 0, 13) if masked else None
    got = check(c, uf, rows, mask=mask, method="faults")
    plain = c.compile_detector_sampler(seed=5, method="faults").count(SHOTS, decoder=uf, **({} if mask is None else dict(postselection_mask=mask)))
    # corrected=False is what tally_rows gives today, and only the observables' side differs between the two
    assert plain == tally_rows(rows, num_detectors=uf.num_detectors, decoder=uf, postselection_mask=mask, histogram_columns=(uf.num_detectors,))
    assert not plain.corrected and plain != got
    assert 0 < plain.decoded_errors < plain.kept_with_observable_flip and (0 < got.kept < SHOTS) == masked
    assert (got.kept, got.decoded_errors, got.decoder_misses) == (plain.kept, plain.decoded_errors, plain.decoder_misses)
    assert np.array_equal(got.detector_counts, plain.detector_counts)
    assert int(got.observable_counts[0]) == got.decoded_errors == int(got.histogram[1])


def test_union_find_with_a_soft_output(hip):
    c, rows = d3()
    soft = UnionFindDecoder.from_circuit(c).with_soft_output("largest_cluster", 16)
    got = check(c, soft, rows, method="faults")
    assert got.soft_output == "largest_cluster" and int(got.soft_kept.sum()) == got.kept and int(got.soft_errors.sum()) == got.decoded_errors > 0


def test_union_find_with_heralds(hip):
    c = erasure_memory(3, 3)
    uf = UnionFindDecoder.from_circuit(c, heralds=True)
    assert uf.info()["n_heralds"] == 144
    mask = detector_mask(uf.num_detectors, int(uf.graph.herald_det[7]), int(uf.graph.node_det[13]))   # a herald column and a node column
    got = check(c, uf, seed=21, mask=mask, method="faults")
    assert 0 < got.kept < SHOTS and got.decoded_errors > 0


def test_windowed_union_find(hip):
    """d = 3, 12 rounds; commit / window of 2 / 4 rounds (a round is 8 detector columns)."""
    c = long_memory(3, 12, 2e-3)
    w = WindowedUnionFindDecoder.from_circuit(c, 16, 32)
    assert w.info()["n_windows"] == 5
    got = check(c, w, seed=21, mask=detector_mask(w.num_detectors, 0, 70), method="faults")
    assert 0 < got.kept < SHOTS and got.decoded_errors > 0


def test_lookup_decoder_on_the_default_sampler(hip):
    c = memory(3, 0.01)
    dec = LookupDecoder.from_counts(c.compile_detector_sampler(seed=8).count(SHOTS, pattern_columns="all"))
    got = check(c, dec, seed=9)
    assert got.decoder_misses > 0 and 0 < got.decoded_errors < got.kept


# ---- decode_file ---------------------------------------------------------------------------------------------------------------

def recorded():
    """``(decoder, rows)``: 5000 + 13 rows of d = 3 memory at p = 0.02 (``fault_rows_host`` under key (1, 2))."""
    if "file" not in _ROWS:
        c = memory(3, 0.02)
        _ROWS["file"] = (UnionFindDecoder.from_circuit(c), faults.fault_rows_host(c.compile_faults(), 0, 5013, (1, 2)).view(np.bool_))
    return _ROWS["file"]


@pytest.mark.parametrize("appended", [False, True])
@pytest.mark.parametrize("in_format", ["b8", "dets"])
def test_decode_file_bit_for_bit(hp, tmp_path, in_format, appended):
    uf, rows = recorded()
    nd, n_obs = uf.num_detectors, uf.num_observables
    data = rows if appended else rows[:, :nd]
    src = tmp_path / f"events.{in_format}"
    shotdata.write_shot_data_file(data=np.ascontiguousarray(data), path=src, format=in_format, num_detectors=nd,
                                  num_observables=n_obs if appended else 0)
    want = uf.decode(rows[:, :nd])
    wrong = int((want != rows[:, nd:]).any(axis=1).sum())
    assert 0 < wrong < len(rows) and want.any()
    for out_format in ("01", "r8"):
        dst = tmp_path / f"predictions.{out_format}"
        res = uf.decode_file(detection_events_filepath=src, detection_events_format=in_format, predictions_filepath=dst,
                             predictions_format=out_format, observables_appended=appended, hp=hp)
        assert res == DecodeFileResult(len(rows), len(rows), wrong if appended else None, int(uf.missed(rows[:, :nd]).sum()))
        got = shotdata.read_shot_data_file(path=dst, format=out_format, num_observables=n_obs)
        assert got.shape == want.shape and np.array_equal(got, want)


def test_decode_file_in_pieces_and_by_the_other_decoders(hp, tmp_path, monkeypatch):
    """A file read in several pieces (a small chunk size), into ``ptb64`` and ``dets``; the lookup decoder's method."""
    uf, rows = recorded()
    nd, n_obs = uf.num_detectors, uf.num_observables
    rows = rows[:4992]  # (ptb64: a multiple of 64)
    src = tmp_path / "events.01"
    shotdata.write_shot_data_file(data=np.ascontiguousarray(rows), path=src, format="01")
    monkeypatch.setattr(shotdata, "CHUNK_BYTES", 20000)
    uniq, first = np.unique(rows[:2000, :nd], axis=0, return_index=True)
    look = LookupDecoder(uniq, rows[first, nd:])
    for dec, out_format in ((uf, "ptb64"), (uf, "dets"), (look, "b8")):
        dst = tmp_path / f"predictions.{out_format}"
        res = dec.decode_file(detection_events_filepath=src, detection_events_format="01", predictions_filepath=dst,
                              predictions_format=out_format, observables_appended=True, hp=hp)
        want = dec.decode(rows[:, :nd])
        assert res == DecodeFileResult(len(rows), len(rows), int((want != rows[:, nd:]).any(axis=1).sum()), int(dec.missed(rows[:, :nd]).sum()))
        assert np.array_equal(shotdata.read_shot_data_file(path=dst, format=out_format, num_observables=n_obs), want)
    assert res.decoder_misses > 0


def test_decode_file_of_an_empty_file(hip, tmp_path):
    """No rows: an empty predictions file and zeros; ``hp`` left to the default."""
    uf, _ = recorded()
    src, dst = tmp_path / "events.b8", tmp_path / "predictions.01"
    src.write_bytes(b"")
    res = uf.decode_file(detection_events_filepath=src, detection_events_format="b8", predictions_filepath=dst, predictions_format="01",
                         observables_appended=True)
    assert res == DecodeFileResult(0, 0, 0, 0) and os.path.getsize(dst) == 0
    res = uf.decode_file(detection_events_filepath=src, detection_events_format="b8", predictions_filepath=dst, predictions_format="01")
    assert res == DecodeFileResult(0, 0, None, 0) and os.path.getsize(dst) == 0
