"""Where finished device rows go (``tsim_amd.sampler``: bools, the compacted ``bit_packed`` prefix, kernel-written
``bit_packed`` rows, arranged column blocks, the sinks of ``count()`` and ``sample_write()``), at the smallest shapes
that take every branch of the two pipelines: more batches than lanes with and without a partial last batch (host
noise), a first, a middle and a last group and a single batch (device noise).  Everything is compared bit for bit with
what numpy makes of the plain bool rows of an identically seeded twin."""

import functools

import numpy as np
import pytest

from tsim_amd import synth
from tsim_amd.channels import error_probs
from tsim_amd.counts import default_histogram_columns, tally_rows
from tsim_amd.sampler import CompiledDetectorSampler

pytestmark = pytest.mark.gpu

DET, OBS = "use_detector_reference_sample", "use_observable_reference_sample"
BIG = "device_groups"
SHAPES = {  # noise, shots, batch_size
    "host_exact": ("host", 2_600, 200),     # 13 batches on 8 lanes, exact cover: a riding reference row grows the plan
    "host_partial": ("host", 2_501, 200),   # a partial last batch
    BIG: ("device", 5 * 2**20 + 3, 2**20),  # groups of 1, 4 and 1 batches (smaller batches are merged)
    "device_one": ("device", 2_501, None),  # one batch
}
ARRANGED = {
    "prepend": dict(prepend_observables=True),
    "prepend_append": dict(prepend_observables=True, append_observables=True),
    "separate_packed": dict(separate_observables=True, bit_packed=True),
    "det_ref": {DET: True},
    "obs_ref_append_packed": {OBS: True, "append_observables": True, "bit_packed": True},
    "both_refs_separate": {DET: True, OBS: True, "separate_observables": True},
}
DELIVERIES = {"bools": {}, "packed_prefix": dict(bit_packed=True), "packed_prefix_append": dict(bit_packed=True, append_observables=True), **ARRANGED}
REFS = {"plain": {}, "det_ref": {DET: True}, "both_refs": {DET: True, OBS: True}}


def maker(noise):
    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    kw = dict(channel_probs=[error_probs(0.02)] * nf, error_transform=np.eye(nf, dtype=np.uint8), noise=noise)
    return lambda: CompiledDetectorSampler(prog, seed=33, **kw)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """``(rows, rows beside a reference sample, the reference sample)`` of the shape: the plain bool rows, read-only."""
    noise, shots, bs = SHAPES[shape]
    mk = maker(noise)
    out = (mk()._sample_batches(shots, bs),) + tuple(mk()._sample_batches(shots, bs, compute_reference=True))
    for a in out:
        a.setflags(write=False)
    assert out[2].any()
    return out


def flipped(shape, flags):
    """The full-width rows ``sample(**flags)`` is made of: the plain rows, the reference bits XORed in where asked."""
    plain, beside_ref, ref = reference(shape)
    if not (flags.get(DET) or flags.get(OBS)):
        return plain
    nd = maker("host")()._num_detectors
    flip = np.zeros(len(ref), dtype=np.bool_)
    if flags.get(DET):
        flip[:nd] = ref[:nd]
    if flags.get(OBS):
        flip[nd:] = ref[nd:]
    return beside_ref ^ flip


def expected(rows, nd, flags):
    """The reference's numpy epilogue (sampler.py:850-868, 665-669) over full-width rows."""
    det, obs = rows[:, :nd], rows[:, nd:]
    if flags.get("separate_observables"):
        want = (det, obs)
    elif flags.get("prepend_observables"):
        want = (np.concatenate([obs, det] + ([obs] if flags.get("append_observables") else []), axis=1),)
    else:
        want = (rows if flags.get("append_observables") else det,)
    return tuple(np.packbits(w, axis=1, bitorder="little") for w in want) if flags.get("bit_packed") else want


def request(shape, flags):
    noise, shots, bs = SHAPES[shape]
    if shape == BIG:  # (bytes, not bools, at five million shots)
        flags = dict(flags, bit_packed=True)
    return maker(noise), shots, dict(flags, batch_size=bs)


def unique_cases():
    seen, out = set(), []
    for shape in SHAPES:
        for name, flags in DELIVERIES.items():
            key = (shape, tuple(sorted(request(shape, flags)[2].items(), key=str)))
            if key not in seen:
                seen.add(key)
                out.append((shape, name))
    return out


@pytest.mark.parametrize("shape,delivery", unique_cases())
def test_delivery_equals_the_numpy_epilogue(hip, shape, delivery):
    mk, shots, kw = request(shape, DELIVERIES[delivery])
    s = mk()
    got = s.sample(shots, **kw)
    got = got if isinstance(got, tuple) else (got,)
    want = expected(flipped(shape, kw), s._num_detectors, kw)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


def direct_mask(s):
    mask = np.zeros(s._num_detectors, dtype=bool)
    mask[np.flatnonzero(s._direct_detector_mask)[::3]] = True
    return mask


@pytest.mark.parametrize("refs", ["plain", "both_refs"])
@pytest.mark.parametrize("shape", [BIG, "device_one"])
def test_device_noise_postselection_blanks_the_plain_rows(hip, shape, refs):
    """Device noise samples every row and blanks the discarded ones (sampler.py:532-540): their direct detector columns
    stay, reference bits only there; the survivors are the plain rows with the reference bits."""
    mk, shots, kw = request(shape, REFS[refs])
    s = mk()
    nd, direct, mask = s._num_detectors, s._direct_detector_mask, direct_mask(s)
    plain, beside_ref, ref = reference(shape)
    rows = (beside_ref if REFS[refs] else plain).copy()
    test = rows[:, :nd] ^ ref[:nd] if kw.get(DET) else rows[:, :nd]
    gone = (test & mask).any(axis=1)
    assert 0.02 < gone.mean() < 0.98
    keep = np.zeros(rows.shape[1], dtype=bool)
    keep[:nd] = direct
    rows[gone] &= keep
    if kw.get(DET):
        rows[:, :nd] ^= np.where(gone[:, None], ref[:nd] & direct, ref[:nd])
    if kw.get(OBS):
        rows[~gone, nd:] ^= ref[nd:]
    forms = [dict(bit_packed=True, append_observables=True), dict(bit_packed=True)] + ([] if shape == BIG else [dict(append_observables=True)])
    for form in forms:
        got = mk().sample(shots, postselection_mask=mask, **dict(kw, **form))
        np.testing.assert_array_equal(got, expected(rows, nd, dict(kw, **form))[0], err_msg=str(form))


@pytest.mark.parametrize("refs", ["plain", "both_refs"])
@pytest.mark.parametrize("shape", ["host_exact", "host_partial"])
def test_host_noise_postselection_packed_prefix_equals_the_bools(hip, shape, refs):
    """Host noise compacts the survivors into batches of their own (other keys than the plain rows'): the ``bit_packed``
    prefix forms, made on the device, are held to the bool rows, and the discarded rows to their blank form."""
    mk, shots, kw = request(shape, REFS[refs])
    s = mk()
    nd, direct, mask = s._num_detectors, s._direct_detector_mask, direct_mask(s)
    bools = mk().sample(shots, postselection_mask=mask, append_observables=True, **kw)
    gone = (bools[:, :nd] & mask).any(axis=1)
    assert 0.02 < gone.mean() < 0.98
    assert not bools[gone][:, nd:].any() and not bools[gone][:, :nd][:, ~direct].any()
    for form in (dict(append_observables=True), {}):
        got = mk().sample(shots, postselection_mask=mask, bit_packed=True, **dict(kw, **form))
        np.testing.assert_array_equal(got, expected(bools, nd, dict(form, bit_packed=True))[0], err_msg=str(form))


@pytest.mark.parametrize("refs", sorted(REFS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_count_equals_the_tally_of_the_rows(hip, shape, refs):
    """``count()``: the sink, without and with the riding reference row."""
    noise, shots, bs = SHAPES[shape]
    s = maker(noise)()
    rows = flipped(shape, REFS[refs])
    nd = s._num_detectors
    got = s.count(shots, batch_size=bs, **REFS[refs])
    assert got == tally_rows(rows, num_detectors=nd, histogram_columns=default_histogram_columns(nd, rows.shape[1]))


@pytest.mark.parametrize("refs", sorted(REFS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sample_write_equals_the_encoded_rows(hip, tmp_path, shape, refs):
    """``sample_write(format="01")``: one line of ``0`` / ``1`` per shot, detectors then observables."""
    noise, shots, bs = SHAPES[shape]
    path = tmp_path / "rows.01"
    maker(noise)().sample_write(shots, filepath=path, format="01", batch_size=bs, append_observables=True, **REFS[refs])
    rows = flipped(shape, REFS[refs])
    text = np.full((shots, rows.shape[1] + 1), ord("\n"), dtype=np.uint8)
    text[:, :-1] = rows + np.uint8(ord("0"))
    got = np.fromfile(path, dtype=np.uint8)
    assert got.size == text.size
    np.testing.assert_array_equal(got.reshape(text.shape), text)


@pytest.mark.parametrize("noise", ["host", "device"])
def test_sampling_goes_on_after_release(hip, noise):
    """``release()`` gives every cached device buffer back; the next request allocates again and the keys go on."""
    shots, bs = (2_501, 200) if noise == "host" else (2_501, None)
    a, b = maker(noise)(), maker(noise)()
    first = a.sample(shots, batch_size=bs, append_observables=True)
    a.release()
    assert not a._bufs
    np.testing.assert_array_equal(first, b.sample(shots, batch_size=bs, append_observables=True))
    for flags in (dict(bit_packed=True), {DET: True, "prepend_observables": True}):
        np.testing.assert_array_equal(a.sample(shots, batch_size=bs, **flags), b.sample(shots, batch_size=bs, **flags))
    a.release()
    b.release()
