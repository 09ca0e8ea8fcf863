"""stim's shot-data formats on the MI355X: the device codec against the numpy statement (tests/shotdata_np.py), file round
trips and faults, sample_write against sample(), convert_file against convert()."""

import warnings

import numpy as np
import pytest

import shotdata_np as S
from tsim_amd import circuits, shotdata, synth
from tsim_amd.channels import error_probs
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.sampler import CompiledDetectorSampler

pytestmark = pytest.mark.gpu

WIDTHS = [0, 1, 7, 8, 9, 63, 64, 65, 254, 255, 256, 300, 1000, 10000]
DENSITIES = [0.0, 1e-3, 0.5, 1.0]


class Dev:
    """Device memory from the codec's staging slots, for the duration of a test."""

    def __init__(self):
        self.c = shotdata.codec(0)
        self.slots = []

    def buf(self, nbytes):
        s = self.c.take_slot()
        self.slots.append(s)
        return self.c.staging(s, nbytes, pinned=False)

    def up(self, data: bytes):
        d = self.buf(len(data) + 16)
        if data:
            h = np.frombuffer(data, np.uint8).copy()
            self.c.copy(d, h.ctypes.data, len(data))
            self.c.sync()
        return d

    def down(self, d, nbytes):
        h = np.empty(nbytes, np.uint8)
        if nbytes:
            self.c.copy(h.ctypes.data, d, nbytes)
        self.c.sync()
        return h.tobytes()

    def close(self):
        for s in self.slots:
            self.c.give_slot(s)
        self.slots = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def rows_for(n, p, B, seed):
    rng = np.random.default_rng(seed)
    return rng.random((B, n)) < p


def sections_for(fmt, n):
    return (n // 4, n - n // 4 - n // 3, n // 3) if fmt == "dets" else None


@pytest.mark.parametrize("stride", ["odd", "aligned"])
@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("n", WIDTHS)
def test_device_encode_and_decode_match_the_oracle(dev, fmt, n, stride):
    B = 128 if fmt == "ptb64" else 131  # not a multiple of a block
    if n == 10000:
        B = 64
    sec = sections_for(fmt, n)
    for k, p in enumerate(DENSITIES):
        rows = rows_for(n, p, B, seed=n * 7 + k)
        # padded rows with garbage in the pad bits and pad bytes
        used = (n + 7) // 8
        rb = used + 5 if stride == "odd" else (used + 7) // 8 * 8 + 8  # (aligned: the 8-byte row loads)
        raw = np.random.default_rng(k).integers(0, 256, size=(B, rb), dtype=np.uint8)
        raw[:, :used] = np.packbits(rows.view(np.uint8), axis=1, bitorder="little") if n else raw[:, :0]
        if n % 8:
            raw[:, used - 1] |= np.uint8(0xFF << (n % 8) & 0xFF)
        want = S.encode(fmt, rows, sec)
        d_rows = dev.up(raw.tobytes())
        cap = len(want) + 64
        d_out = dev.buf(cap)
        kw = dict(zip(("num_measurements", "num_detectors", "num_observables"), sec)) if sec else {}
        got_n = shotdata.encode_rows_device(d_rows, B, row_bytes=rb, n_bits=n, format=fmt, d_out=d_out, out_capacity=cap, **kw)
        assert got_n == len(want)
        assert dev.down(d_out, got_n) == want, (fmt, n, p)
        if n == 0 and fmt in ("b8", "ptb64"):
            dev.close()
            continue
        d_in = dev.up(want)
        d_dec = dev.buf(B * used + 16)
        r, used_bytes, fault, _kind = shotdata.decode_bytes_device(d_in, len(want), final=True, n_bits=n, format=fmt, d_rows=d_dec,
                                                                   row_bytes=used, max_rows=B, **kw)
        assert (r, used_bytes, fault) == (B, len(want), -1), (fmt, n, p)
        got = np.frombuffer(dev.down(d_dec, B * used), np.uint8).reshape(B, used)
        assert np.array_equal(got, np.packbits(rows.view(np.uint8), axis=1, bitorder="little")), (fmt, n, p)
        dev.close()


def test_padded_uint64_rows_use_the_compaction(dev):
    n, B = 130, 200
    rows = rows_for(n, 0.3, B, 5)
    raw = np.zeros((B, 24), np.uint8)
    raw[:, :17] = np.packbits(rows.view(np.uint8), axis=1, bitorder="little")
    raw[:, 16] |= 0xFC  # garbage past column 129
    raw[:, 17:] = 0xA5
    d_rows, d_out = dev.up(raw.tobytes()), dev.buf(B * 17)
    assert shotdata.encode_rows_device(d_rows, B, row_bytes=24, n_bits=n, format="b8", d_out=d_out, out_capacity=B * 17) == B * 17
    assert dev.down(d_out, B * 17) == S.encode("b8", rows)


def test_encode_reports_a_short_buffer(dev):
    rows = rows_for(50, 0.5, 70, 1)
    want = S.encode("hits", rows)
    d_rows = dev.up(np.packbits(rows.view(np.uint8), axis=1, bitorder="little").tobytes())
    d_out = dev.up(b"\xab" * len(want))
    assert shotdata.encode_rows_device(d_rows, 70, row_bytes=7, n_bits=50, format="hits", d_out=d_out, out_capacity=10) == len(want)
    assert dev.down(d_out, len(want)) == b"\xab" * len(want)  # nothing was written


def test_fixed_formats_encode_in_pieces(dev, tmp_path, monkeypatch):
    """A writer encodes a call's rows in pieces of about CHUNK_BYTES of 01 text: the file is the same."""
    monkeypatch.setattr(shotdata, "CHUNK_BYTES", 100)
    rows = rows_for(70, 0.2, 640, 3)
    for fmt in S.FORMATS:
        sec = (0, 70, 0)
        w = shotdata.ShotWriter(tmp_path / "p", fmt, 70, sec)
        w.write_packed(np.packbits(rows.view(np.uint8), axis=1, bitorder="little"))
        w.close()
        assert (tmp_path / "p").read_bytes() == S.encode(fmt, rows, sec), fmt


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("chunk", [3, 17, 64, 1000, None])
def test_file_round_trip_independent_of_chunk_size(tmp_path, monkeypatch, fmt, chunk):
    if chunk is not None:
        monkeypatch.setattr(shotdata, "CHUNK_BYTES", chunk)
    for n, B, p in ((10, 192, 0.3), (300, 128, 0.01), (65, 64, 0.9)):
        rows = rows_for(n, p, B, n)
        sec = sections_for(fmt, n) or (0, n, 0)
        kw = dict(zip(("num_measurements", "num_detectors", "num_observables"), sec))
        path = tmp_path / f"x.{fmt}"
        shotdata.write_shot_data_file(data=rows, path=path, format=fmt, **kw)
        assert path.read_bytes() == S.encode(fmt, rows, sec)
        assert np.array_equal(shotdata.read_shot_data_file(path=path, format=fmt, **kw), rows)
        packed = shotdata.read_shot_data_file(path=path, format=fmt, bit_packed=True, **kw)
        assert np.array_equal(packed, np.packbits(rows.view(np.uint8), axis=1, bitorder="little"))
        shotdata.write_shot_data_file(data=packed, path=path, format=fmt, **kw)
        assert path.read_bytes() == S.encode(fmt, rows, sec)


@pytest.mark.parametrize("fmt,data,n,sec,offset", [
    ("01", b"0011\n", 4, None, None),
    ("01", b"0012\n", 4, None, 3),
    ("01", b"001\n0000\n", 4, None, 3),
    ("01", b"00110\n", 4, None, 4),
    ("01", b"0011\n00", 4, None, 7),
    ("b8", b"\x01\x02\x03", 10, None, 3),
    ("ptb64", b"\x00" * 12, 1, None, 12),
    ("r8", bytes([2, 9]), 10, None, 1),
    ("r8", bytes([255]), 10, None, 0),
    ("r8", bytes([10, 3]), 10, None, 2),
    ("hits", b"1,2\n3,x\n", 10, None, 6),
    ("hits", b"1,12\n", 10, None, 2),
    ("hits", b"1,,2\n", 10, None, 2),
    ("hits", b"\n,1\n", 10, None, 1),
    ("dets", b"shot D1 L3\n", 6, (0, 3, 3), 8),
    ("dets", b"shot D1 X0\n", 6, (0, 3, 3), 8),
    ("dets", b"shot 1\n", 6, (0, 3, 3), 5),
    ("dets", b"shot D1\nsho D2\n", 6, (0, 3, 3), 11),
    ("dets", b"shot M0\n", 6, (0, 3, 3), 5),
])
def test_faults_name_the_byte_offset(tmp_path, monkeypatch, fmt, data, n, sec, offset):
    sec = sec or (0, n, 0)
    kw = dict(zip(("num_measurements", "num_detectors", "num_observables"), sec))
    path = tmp_path / "bad"
    path.write_bytes(data)
    for chunk in (4, 1 << 20):
        monkeypatch.setattr(shotdata, "CHUNK_BYTES", chunk)
        if offset is None:
            shotdata.read_shot_data_file(path=path, format=fmt, **kw)
            continue
        with pytest.raises(ValueError, match=f"byte offset {offset}\\b") as e:
            shotdata.read_shot_data_file(path=path, format=fmt, **kw)
        assert str(path) in str(e.value)


def test_reader_leniency(tmp_path):
    p = tmp_path / "t"
    p.write_bytes(b"3,1,3\n\n0")
    want = np.zeros((3, 5), bool)
    want[0, [1, 3]] = True
    want[2, 0] = True
    assert np.array_equal(shotdata.read_shot_data_file(path=p, format="hits", num_measurements=5), want)
    p.write_bytes(b"shot  D3   D1 D3\nshot\nshot D0")
    assert np.array_equal(shotdata.read_shot_data_file(path=p, format="dets", num_detectors=5), want)
    p.write_bytes(b"01\n10")
    assert shotdata.read_shot_data_file(path=p, format="01", num_measurements=2).tolist() == [[False, True], [True, False]]


# ---- sample_write ---------------------------------------------------------------------------------------------------

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


SURFACE = circuits.rotated_surface_code_memory(3, 3)
NO_COMPONENTS = """
    R 0 1 2
    X_ERROR(0.2) 0
    X_ERROR(0.3) 1
    M 0 1 2
    DETECTOR rec[-3]
    DETECTOR rec[-2]
    OBSERVABLE_INCLUDE(0) rec[-3] rec[-2]
"""

FLAGS = [
    dict(),
    dict(append_observables=True),
    dict(prepend_observables=True),
    dict(prepend_observables=True, append_observables=True),
    dict(append_observables=True, use_detector_reference_sample=True, use_observable_reference_sample=True),
    dict(separate=True),
]


def expected_files(s, shots, fmt, flags, batch_size, tmp_path):
    kw = {k: v for k, v in flags.items() if k != "separate"}
    res = s.sample(shots, batch_size=batch_size, separate_observables=flags.get("separate", False), **kw)
    nd = s._num_detectors
    if flags.get("separate"):
        det, obs = res
        return S.encode(fmt, det, (0, det.shape[1], 0)), S.encode("hits", obs)
    n = res.shape[1]
    return S.encode(fmt, res, (0, nd, n - nd) if fmt == "dets" else None), None


@pytest.mark.parametrize("maker", [
    pytest.param(lambda noise: c2_maker(noise), id="c2"),
    pytest.param(lambda noise: clifford_maker(SURFACE, noise), id="surface"),
    pytest.param(lambda noise: clifford_maker(NO_COMPONENTS, noise), id="no-components"),
])
@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_sample_write_equals_encoded_sample(tmp_path, maker, noise, fmt):
    mk = maker(noise)
    shots = 320
    for flags in (FLAGS if fmt in ("01", "ptb64") else FLAGS[1::3]):
        if fmt == "dets" and flags.get("prepend_observables"):
            continue
        for batch_size in (None, 100):
            a, b = mk(), mk()
            want, want_obs = expected_files(a, shots, fmt, flags, batch_size, tmp_path)
            path, obs_path = tmp_path / "out", tmp_path / "obs"
            kw = {k: v for k, v in flags.items() if k != "separate"}
            if flags.get("separate"):
                kw.update(obs_out_filepath=obs_path, obs_out_format="hits")
            b.sample_write(shots, filepath=path, format=fmt, batch_size=batch_size, **kw)
            assert path.read_bytes() == want, (flags, batch_size)
            if want_obs is not None:
                assert obs_path.read_bytes() == want_obs
            assert np.array_equal(a.sample(64, append_observables=True), b.sample(64, append_observables=True))  # the keys agree


def test_measurement_sample_write(tmp_path):
    for noise in ("host", "device"):
        mk = clifford_maker(SURFACE, noise, measurement=True)
        a, b = mk(), mk()
        want = a.sample(256, batch_size=100)
        n = want.shape[1]
        for fmt in S.FORMATS:
            for chunk in (None, 200):  # 200: the writer encodes 64 rows at a time
                b2 = mk()
                if chunk:
                    shotdata.CHUNK_BYTES, saved = chunk, shotdata.CHUNK_BYTES
                try:
                    b2.sample_write(256, filepath=tmp_path / "m", format=fmt, batch_size=100)
                finally:
                    if chunk:
                        shotdata.CHUNK_BYTES = saved
                assert (tmp_path / "m").read_bytes() == S.encode(fmt, want, (n, 0, 0)), (fmt, chunk)
        b.sample_write(256, filepath=tmp_path / "m", format="r8", batch_size=100)
        assert np.array_equal(a.sample(64), b.sample(64))


# ---- convert_file ---------------------------------------------------------------------------------------------------

def test_convert_file_equals_encoded_convert(tmp_path):
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        meas = c.compile_sampler(seed=5).sample(192)
    conv = c.compile_m2d_converter()
    M, nd, no = conv.num_measurements, conv.num_detectors, conv.num_observables
    det_app = conv.convert(measurements=meas, append_observables=True)
    det, obs = conv.convert(measurements=meas, separate_observables=True)
    for fin in S.FORMATS:
        mpath = tmp_path / f"m.{fin}"
        mpath.write_bytes(S.encode(fin, meas, (M, 0, 0)))
        for fout in S.FORMATS:
            out, opath = tmp_path / "d", tmp_path / "o"
            conv.convert_file(measurements_filepath=mpath, measurements_format=fin, detection_events_filepath=out,
                              detection_events_format=fout, append_observables=True)
            assert out.read_bytes() == S.encode(fout, det_app, (0, nd, no)), (fin, fout)
            conv.convert_file(measurements_filepath=mpath, measurements_format=fin, detection_events_filepath=out,
                              detection_events_format=fout, obs_out_filepath=opath, obs_out_format=fout)
            assert out.read_bytes() == S.encode(fout, det, (0, nd, 0)), (fin, fout)
            assert opath.read_bytes() == S.encode(fout, obs, (0, 0, no)), (fin, fout)


def test_convert_file_in_small_chunks(tmp_path, monkeypatch):
    """Decoded chunks of a few rows: the ptb64 output carries partial groups from chunk to chunk."""
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        meas = c.compile_sampler(seed=6).sample(256)
    conv = c.compile_m2d_converter()
    M, nd, no = conv.num_measurements, conv.num_detectors, conv.num_observables
    det, obs = conv.convert(measurements=meas, separate_observables=True)
    monkeypatch.setattr(shotdata, "CHUNK_BYTES", 150)
    for fin in ("01", "r8", "dets"):
        mpath = tmp_path / f"m.{fin}"
        mpath.write_bytes(S.encode(fin, meas, (M, 0, 0)))
        for fout in ("ptb64", "hits"):
            conv.convert_file(measurements_filepath=mpath, measurements_format=fin, detection_events_filepath=tmp_path / "d",
                              detection_events_format=fout, obs_out_filepath=tmp_path / "o", obs_out_format="ptb64")
            assert (tmp_path / "d").read_bytes() == S.encode(fout, det), (fin, fout)
            assert (tmp_path / "o").read_bytes() == S.encode("ptb64", obs), (fin, fout)


def test_a_failed_close_releases_every_writer(tmp_path):
    """ptb64 output of a row count that is not a multiple of 64 raises at close; every staging slot comes back."""
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        meas = c.compile_sampler(seed=7).sample(100)
    conv = c.compile_m2d_converter()
    mpath = tmp_path / "m.01"
    mpath.write_bytes(S.encode("01", meas))
    codec = shotdata.codec(0)
    free = len(codec._free)
    for _ in range(3):
        with pytest.raises(ValueError, match="multiple of 64"):
            conv.convert_file(measurements_filepath=mpath, detection_events_filepath=tmp_path / "d", detection_events_format="ptb64",
                              obs_out_filepath=tmp_path / "o", obs_out_format="ptb64")
        assert len(codec._free) == free
