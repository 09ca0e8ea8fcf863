"""stim's shot-data formats without a device: the numpy statement against the worked examples, and argument checks that
must fail before any device call."""

import numpy as np
import pytest

import shotdata_np as S
from tsim_amd import shotdata
from tsim_amd.channels import error_probs
from tsim_amd.m2d import CompiledMeasurementsToDetectionEventsConverter
from tsim_amd.program import CompiledComponent, make_program, scalar_graphs_from_terms
from tsim_amd.sampler import CompiledDetectorSampler, CompiledMeasurementSampler

N = 10
A = np.zeros(N, bool)
B = np.zeros(N, bool)
B[[2, 3]] = True
C = np.zeros(N, bool)
C[[0, 9]] = True


def one(n, cols=()):
    r = np.zeros((1, n), bool)
    r[0, list(cols)] = True
    return r


@pytest.mark.parametrize("fmt,want", [
    ("01", [b"0000000000\n", b"0011000000\n", b"1000000001\n"]),
    ("b8", [bytes([0, 0]), bytes([0x0C, 0]), bytes([1, 2])]),
    ("r8", [bytes([10]), bytes([2, 0, 6]), bytes([0, 8, 0])]),
    ("hits", [b"\n", b"2,3\n", b"0,9\n"]),
    ("dets", [b"shot\n", b"shot D2 D3\n", b"shot D0 L2\n"]),
])
def test_worked_examples(fmt, want):
    sec = (0, 7, 3)
    for row, w in zip((A, B, C), want):
        assert S.encode(fmt, row[None], sec) == w
        assert np.array_equal(S.decode(fmt, w, N, sec), row[None])
    assert S.encode("dets", C[None], (10, 0, 0)) == b"shot M0 M9\n"


def test_r8_long_runs():
    assert S.encode("r8", one(300)) == bytes([255, 45])
    assert S.encode("r8", one(255)) == bytes([255, 0])
    assert S.encode("r8", one(256, [255])) == bytes([255, 0, 0])
    for rows in (one(300), one(255), one(256, [255])):
        assert np.array_equal(S.decode("r8", S.encode("r8", rows), rows.shape[1]), rows)


def test_ptb64_example():
    rows = np.zeros((64, N), bool)
    rows[0], rows[63] = C, B
    data = S.encode("ptb64", rows)
    assert len(data) == 80
    words = np.frombuffer(data, "<u8")
    want = np.zeros(10, np.uint64)
    want[0] = 1
    want[2] = want[3] = np.uint64(1 << 63)
    want[9] = 1
    assert np.array_equal(words, want)
    assert np.array_equal(S.decode("ptb64", data, N), rows)


def test_zero_width_rows():
    rows = np.zeros((3, 0), bool)
    assert S.encode("01", rows) == b"\n" * 3
    assert S.encode("r8", rows) == bytes([0, 0, 0])
    assert S.encode("hits", rows) == b"\n" * 3
    assert S.encode("dets", rows, (0, 0, 0)) == b"shot\n" * 3


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("n", [1, 7, 9, 64, 65, 300])
def test_oracle_round_trip(fmt, n):
    rng = np.random.default_rng(n)
    rows = rng.random((64, n)) < 0.2
    sec = (n // 3, n - n // 3 - n // 5, n // 5)
    assert np.array_equal(S.decode(fmt, S.encode(fmt, rows, sec), n, sec), rows)


# ---- argument checks before any device call ----------------------------------------------------------------------

def no_device(*_a, **_k):
    raise AssertionError("the device was used")


def random_bit_component(output_index):
    lv0 = scalar_graphs_from_terms(0, [dict()])
    lv1 = scalar_graphs_from_terms(1, [dict(power2=-1)])
    return CompiledComponent((output_index,), np.zeros(0, np.int32), (lv0, lv1))


def det_sampler():
    prog = make_program([random_bit_component(2), random_bit_component(3)], [(0, 0, False), (1, 1, False), (4, 2, True)], 5, 3)
    return CompiledDetectorSampler(prog, channel_probs=[error_probs(0.3), error_probs(0.2), error_probs(0.4)],
                                   error_transform=np.eye(3, dtype=np.uint8), seed=0)


@pytest.mark.parametrize("kwargs", [
    dict(format="07"),
    dict(format=8),
    dict(format="ptb64", shots=100),
    dict(format="b8", obs_out_filepath="x.obs", obs_out_format="bad"),
    dict(format="01", obs_out_filepath="x.obs", obs_out_format="ptb64", shots=100),
    dict(format="01", obs_out_filepath="x.obs", append_observables=True),
    dict(format="01", obs_out_filepath="x.obs", prepend_observables=True),
    dict(format="dets", prepend_observables=True),
    dict(format="01", shots=-1),
    dict(format="01", batch_size=0),
])
def test_sample_write_rejects_bad_arguments_before_any_device_call(monkeypatch, tmp_path, kwargs):
    s = det_sampler()
    monkeypatch.setattr(s, "_hip", no_device)
    monkeypatch.setattr(shotdata, "codec", no_device)
    key, nkey = s._key, s._noise_key
    kw = dict(shots=128, filepath=tmp_path / "out")
    kw.update(kwargs)
    with pytest.raises(ValueError):
        s.sample_write(**kw)
    assert s._key == key and s._noise_key == nkey
    assert not (tmp_path / "out").exists()


def test_measurement_sample_write_rejects_bad_arguments(monkeypatch, tmp_path):
    prog = make_program([random_bit_component(0), random_bit_component(1)], [], 2, 0)
    s = CompiledMeasurementSampler(prog, channel_probs=[], error_transform=np.zeros((0, 0), np.uint8), seed=1)
    monkeypatch.setattr(s, "_hip", no_device)
    monkeypatch.setattr(shotdata, "codec", no_device)
    for kw in (dict(shots=10, format="ptb64"), dict(shots=10, format="x"), dict(shots=-1)):
        with pytest.raises(ValueError):
            s.sample_write(filepath=tmp_path / "m", **kw)


@pytest.mark.parametrize("call", [
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 4), bool), path=p, format="bad"),
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 4), np.int32), path=p, format="01"),
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 4), np.float32), path=p, format="01"),
    lambda p: shotdata.write_shot_data_file(data=np.zeros(3, bool), path=p, format="01"),
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 4), bool), path=p, format="ptb64"),
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 4), bool), path=p, format="dets", num_detectors=3),
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 4), bool), path=p, format="01", num_detectors=-1),
    lambda p: shotdata.write_shot_data_file(data=np.zeros((3, 2), np.uint8), path=p, format="01", num_measurements=20),
    lambda p: shotdata.read_shot_data_file(path=p, format="bad", num_measurements=3),
    lambda p: shotdata.read_shot_data_file(path=p, format="b8"),
    lambda p: shotdata.read_shot_data_file(path=p, format="ptb64"),
    lambda p: shotdata.read_shot_data_file(path=p, format="01", num_detectors=-2),
])
def test_file_functions_reject_bad_arguments_before_any_device_call(monkeypatch, tmp_path, call):
    monkeypatch.setattr(shotdata, "codec", no_device)
    with pytest.raises(ValueError):
        call(tmp_path / "f")


def test_convert_file_rejects_bad_arguments_before_any_device_call(monkeypatch, tmp_path):
    conv = CompiledMeasurementsToDetectionEventsConverter([[0], [0, 1]], [0, 1], num_measurements=2, num_detectors=1)
    monkeypatch.setattr(conv, "_handle", no_device)
    monkeypatch.setattr(shotdata, "codec", no_device)
    kw = dict(measurements_filepath=tmp_path / "m", detection_events_filepath=tmp_path / "d")
    with pytest.raises(NotImplementedError):
        conv.convert_file(sweep_bits_filepath=tmp_path / "s", **kw)
    for bad in (dict(measurements_format="x"), dict(detection_events_format="x"), dict(obs_out_filepath=tmp_path / "o", obs_out_format="x"),
                dict(obs_out_filepath=tmp_path / "o", append_observables=True)):
        with pytest.raises(ValueError):
            conv.convert_file(**kw, **bad)
