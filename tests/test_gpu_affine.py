"""The affine measurement sampler on the device (tsim_affine_*, csrc/tsim_affine.hip.h): the kernel's bytes against the
numpy statement ``affine.affine_rows_host`` for synthetic handles, and the sampler's paths on circuits."""

import ctypes as C

import numpy as np
import pytest

from tsim_amd import _lib, affine, circuits, counts, shotdata, synth
from tsim_amd.clifford import CliffordCircuit

from test_affine import B_SET, FIRST_SHOTS, random_csr

pytestmark = pytest.mark.gpu

KEY = (0x243F6A88, 0x85A308D3)


def pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(np.asarray(bits).astype(np.uint8), axis=1, bitorder="little")


@pytest.fixture(scope="module")
def hp(hip):
    prog = hip.HipProgram(synth.kat_h_m(), device=0)  # device buffers and a stream
    yield prog
    prog.close()


class Case:
    """A synthetic handle, its f rows on the device at a padded stride, and the host statement's rows for one launch."""

    def __init__(self, hp, num_f, n_random, n_out, B_max, seed):
        self.hp, self.num_f, self.n_random, self.n_out = hp, num_f, n_random, n_out
        self.row_ptr, self.cols, self.flip = random_csr(num_f, n_random, n_out, seed)
        self.h = affine.AffineHandle(num_f, n_random, self.row_ptr, self.cols, self.flip)
        rng = np.random.default_rng(seed + 1)
        self.f_rb = 8 * ((num_f + 63) // 64) + 8  # larger than used
        self.f_host = rng.integers(0, 256, (B_max, self.f_rb)).astype(np.uint8)  # garbage in the pad bits and past them
        self.d_f = hp.malloc(max(1, self.f_host.nbytes))
        hp.h2d(self.d_f, self.f_host)

    def want(self, B, first_shot, key=KEY):
        return affine.affine_rows_host(self.flip, self.row_ptr, self.cols, self.num_f, self.n_random,
                                       self.f_host if self.num_f else None, B, first_shot, key)

    def launch(self, B, first_shot, out_packed, col0, n_cols, *, slack=5, key=KEY, row0=0):
        """One launch into a 0xA5-filled buffer: ``(used bytes per row, the rows with their slack)``."""
        used = (n_cols + 7) // 8 if out_packed else n_cols
        rb = used + slack
        got = np.full((B, rb), 0xA5, np.uint8)
        d_out = self.hp.malloc(got.nbytes)
        self.hp.h2d(d_out, got)
        self.h.sample_device(self.d_f.ptr + row0 * self.f_rb if self.num_f else 0, B, d_out.ptr, key=key, first_shot=first_shot,
                             f_row_bytes=self.f_rb, out_row_bytes=rb, out_packed=out_packed, col0=col0, n_cols=n_cols,
                             stream=self.hp.stream_ptr())
        self.hp.synchronize()
        self.hp.d2h(got, d_out)
        d_out.free()
        return used, got

    def close(self):
        self.d_f.free()
        self.h.close()


# every value of num_f {0, 1, 63, 64, 65, 700}, n_random {0, 1, 64, 65, 600} and n_out {1, 7, 8, 9, 64, 65, 513, 1300}
SIZES = [(0, 1, 1), (1, 0, 7), (0, 0, 9), (63, 64, 8), (64, 65, 9), (65, 600, 64), (700, 0, 65), (0, 600, 513), (700, 600, 1300),
         (1, 1, 1300), (64, 64, 64), (63, 1, 513), (65, 65, 65)]


@pytest.mark.parametrize("num_f,n_random,n_out", SIZES)
def test_kernel_matches_host_statement(hp, num_f, n_random, n_out):
    case = Case(hp, num_f, n_random, n_out, max(B_SET), seed=7 * num_f + 3 * n_random + n_out)
    lens = np.diff(case.row_ptr)
    if num_f + n_random and n_out >= 3:
        assert lens.min() == 0 and lens.max() <= 40
    i = 0
    for first_shot in FIRST_SHOTS:
        whole = {}
        for B in B_SET:
            whole[B] = case.want(B, first_shot)
            for out_packed in (False, True):
                # all outputs, or a sub-range that starts and ends inside a byte of the packed row
                col0, n_cols = (0, n_out) if (i % 2 == 0 or n_out < 4) else (3, n_out - 4)
                i += 1
                used, got = case.launch(B, first_shot, out_packed, col0, n_cols)
                w = whole[B][:, col0:col0 + n_cols]
                assert np.array_equal(got[:, :used], pack(w) if out_packed else w), (first_shot, B, out_packed, col0)
                assert (got[:, used:] == 0xA5).all()  # bytes past a row's outputs are not written
    # rows exactly as wide as their outputs (the contiguous store path for rows of at most 64 bytes)
    for out_packed in (False, True):
        used, got = case.launch(200, 64, out_packed, 0, n_out, slack=0)
        w = case.want(200, 64)
        assert np.array_equal(got, pack(w) if out_packed else w)
    case.close()


@pytest.mark.parametrize("num_f,n_random,n_out", [(65, 65, 65), (700, 600, 1300)])
def test_a_launch_cut_in_two_equals_one_launch(hp, num_f, n_random, n_out):
    case = Case(hp, num_f, n_random, n_out, 200, seed=11)
    _, one = case.launch(200, 0, True, 0, n_out, slack=0)
    _, a = case.launch(128, 0, True, 0, n_out, slack=0)
    _, b = case.launch(72, 128, True, 0, n_out, slack=0, row0=128)
    assert np.array_equal(np.concatenate([a, b]), one)
    assert np.array_equal(one, pack(case.want(200, 0)))
    _, other = case.launch(200, 0, True, 0, n_out, slack=0, key=(KEY[0], KEY[1] + 1))
    assert n_random == 0 or not np.array_equal(other, one)
    case.close()


@pytest.mark.parametrize("num_f,n_random,n_out", [(5000, 4000, 300), (2050, 6000, 70)])
def test_columns_in_windows(hp, num_f, n_random, n_out):
    """More masks than one wave's LDS holds: windows of columns; the window that holds the last f columns also holds the
    first random symbols."""
    case = Case(hp, num_f, n_random, n_out, 130, seed=num_f)
    info = case.h.info()
    win = info["window"]
    assert info["n_windows"] > 1 and (num_f // win) * win < num_f < (num_f // win + 1) * win <= num_f + n_random
    assert (info["num_f"], info["n_random"], info["n_out"], info["nnz"]) == (num_f, n_random, n_out, len(case.cols))
    for first_shot in (0, 64 * (2**20 + 3)):
        want = case.want(130, first_shot)
        for out_packed in (False, True):
            used, got = case.launch(130, first_shot, out_packed, 0, n_out)
            assert np.array_equal(got[:, :used], pack(want) if out_packed else want)
            assert (got[:, used:] == 0xA5).all()
    used, got = case.launch(130, 0, True, 5, n_out - 9)
    assert np.array_equal(got[:, :used], pack(case.want(130, 0)[:, 5:n_out - 4])) and (got[:, used:] == 0xA5).all()
    case.close()


def test_argument_errors_come_before_any_launch(hp):
    lib = _lib.load()
    rp = np.array([0, 1, 2], np.int32)
    cols = np.array([0, 3], np.int32)
    flip = np.zeros(2, np.uint8)
    h = C.c_void_p()

    def create(num_f, n_random, n_out, rp_, cols_, flip_):
        return lib.tsim_affine_create(0, num_f, n_random, n_out, _lib.ptr(rp_), _lib.ptr(cols_), _lib.ptr(flip_), C.byref(h))

    assert create(2, 1, 2, rp, cols, flip) == -22 and b"cols[1] = 3" in lib.tsim_last_error()  # columns are 0 .. 2
    assert create(2, 2, 2, np.array([0, 2, 1], np.int32), cols, flip) == -22 and b"decreases" in lib.tsim_last_error()
    assert create(2, 2, 2, None, cols, flip) == -22 and create(2, 2, 2, rp, None, flip) == -22 and create(2, 2, 2, rp, cols, None) == -22
    assert create(-1, 2, 2, rp, cols, flip) == -22
    assert lib.tsim_affine_create(0, 2, 2, 2, _lib.ptr(rp), _lib.ptr(cols), _lib.ptr(flip), None) == -22
    with pytest.raises(ValueError):
        affine.AffineHandle(2, 1, rp, cols, flip)
    good = affine.AffineHandle(9, 2, rp, cols, flip)
    d = hp.malloc(4096)
    ok = dict(key=KEY, first_shot=0, f_row_bytes=8, out_row_bytes=1, out_packed=True, stream=hp.stream_ptr())
    good.sample_device(d.ptr, 64, d.ptr + 2048, **ok)
    hp.synchronize()
    for change, match in ((dict(first_shot=32), "multiple of 64"), (dict(first_shot=-64), "multiple of 64"),
                          (dict(f_row_bytes=1), "f_row_bytes"), (dict(out_row_bytes=0), "out_row_bytes"),
                          (dict(out_packed=False, out_row_bytes=1), "out_row_bytes"), (dict(col0=1, n_cols=2), "outputs"),
                          (dict(first_shot=2**38), "2\\^38")):
        with pytest.raises(ValueError, match=match):
            good.sample_device(d.ptr, 64, d.ptr + 2048, **{**ok, **change})
    with pytest.raises(ValueError, match="NULL"):
        good.sample_device(0, 64, d.ptr + 2048, **ok)
    with pytest.raises(ValueError, match="NULL"):
        good.sample_device(d.ptr, 64, 0, **ok)
    with pytest.raises(ValueError, match="negative"):
        good.sample_device(d.ptr, -1, d.ptr + 2048, **ok)
    good.sample_device(d.ptr, 64, d.ptr + 2048, **{**ok, "first_shot": 2**38 - 64})  # the last tile there is
    hp.synchronize()
    no_f = affine.AffineHandle(0, 2, np.array([0, 1], np.int32), np.array([1], np.int32), np.ones(1, np.uint8))
    no_f.sample_device(0, 64, d.ptr, key=KEY, f_row_bytes=0, out_row_bytes=1, out_packed=False, stream=hp.stream_ptr())  # no f rows
    got = np.zeros(64, np.uint8)
    hp.synchronize()
    hp.d2h(got, d.ptr)
    assert np.array_equal(got, affine.affine_rows_host([1], [0, 1], [1], 0, 2, None, 64, 0, KEY)[:, 0])
    d.free()
    good.close()
    no_f.close()


# ---- the sampler ------------------------------------------------------------------------------------------------------

def memory(d: int) -> str:
    return circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=0.01, before_round_data_depolarization=0.01,
                                                before_measure_flip_probability=0.01)


CIRCUITS = {"d3": memory(3), "d5": memory(5), "m1100": "H 0\n" + "M(0.01) 0\n" * 1100}
_compiled = {}


def circuit(name: str) -> CliffordCircuit:
    if name not in _compiled:
        _compiled[name] = CliffordCircuit(CIRCUITS[name])
        _compiled[name].compile_affine_measurements()
    return _compiled[name]


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_sampler_paths(hip, tmp_path, name, noise):
    c = circuit(name)
    M = c.num_measurements
    shots, bs = 2500, 1000  # three chunks of 1024, 1024, 452 rows
    mk = lambda: c.compile_sampler(seed=9, method="affine", noise=noise)  # noqa: E731
    rows = mk().sample(shots, batch_size=bs)
    assert rows.dtype == np.bool_ and rows.shape == (shots, M)
    if noise == "host":  # the host statement fed the same f rows and the same key
        s = mk()
        f = s._channel_sampler.sample_packed(shots)
        form = c.compile_affine_measurements()
        want = affine.affine_rows_host(form["flip"], form["row_ptr"], form["cols"], form["num_f"], form["n_random"], f, shots, 0,
                                       s._next_key())
        assert np.array_equal(rows, want.view(np.bool_))
        assert np.array_equal(mk().sample(shots), rows)  # ... whatever the batch size
    elif name == "m1100":  # a coin, re-read 1100 times with 1 % flips
        assert 0.4 < rows[:, 0].mean() < 0.6 and 0.005 < (rows ^ rows[:, :1])[:, 1:].mean() < 0.02
    assert np.array_equal(mk().sample(shots, bs, True), pack(rows))
    got = mk().count(shots, batch_size=bs, pair_columns="all", pattern_columns="all")
    assert got == counts.tally_rows(rows, num_detectors=0, histogram_columns=got.histogram_columns, pair_columns="all", pattern_columns="all")
    assert got.shots == got.kept == shots and np.array_equal(got.column_counts, rows.sum(axis=0))
    for fmt in ("b8", "r8"):
        path = tmp_path / f"{name}.{fmt}"
        mk().sample_write(shots, filepath=path, format=fmt, batch_size=bs)
        back = shotdata.read_shot_data_file(path=path, format=fmt, num_measurements=M)
        assert np.array_equal(back, rows), fmt


@pytest.mark.parametrize("name", ["d3", "d5"])
def test_convert_device_chained_behind_the_kernel(hip, hp, name):
    """The sampler's padded uint64 rows -> convert_device, both on one stream == the host conversion of the same rows."""
    c = circuit(name)
    s = c.compile_sampler(seed=4, method="affine")
    conv = c.compile_m2d_converter()
    M, n_out = c.num_measurements, conv.num_detectors + conv.num_observables
    wo, rb = (M + 63) // 64, (n_out + 7) // 8
    seen = {}

    def sink(d_rows, row_bytes, r0, r1, stream):
        assert row_bytes == 8 * wo
        d_e = s._hip().malloc((r1 - r0) * rb)
        conv.convert_device(d_rows, r1 - r0, d_e.ptr, in_row_bytes=row_bytes, in_packed=True, out_row_bytes=rb, out_packed=True,
                            stream=stream)
        s._hip().stream_synchronize(stream)
        rows, ev = np.zeros((r1 - r0, row_bytes), np.uint8), np.zeros((r1 - r0, rb), np.uint8)
        s._hip().d2h(rows, d_rows)
        s._hip().d2h(ev, d_e.ptr)
        d_e.free()
        seen[r0] = (rows, ev)

    s._direct_device(3000, 1024, sink=sink)
    assert sorted(seen) == [0, 1024, 2048]
    rows = np.concatenate([seen[k][0] for k in sorted(seen)])
    events = np.concatenate([seen[k][1] for k in sorted(seen)])
    assert not np.unpackbits(rows, axis=1, bitorder="little")[:, M:].any()  # zero pad bits up to the uint64 words' end
    assert np.array_equal(rows[:, :(M + 7) // 8], pack(c.compile_sampler(seed=4, method="affine").sample(3000)))
    bits = np.unpackbits(rows, axis=1, bitorder="little")[:, :M]
    row_ptr, cols, ref = conv.csr()
    want = np.stack([(bits[:, cols[row_ptr[j]:row_ptr[j + 1]]].sum(axis=1) & 1) ^ ref[j] for j in range(n_out)], axis=1)
    assert np.array_equal(events, pack(want)) and events.any()
    assert np.array_equal(events, conv.convert(measurements=rows[:, :(M + 7) // 8], bit_packed=True, append_observables=True))


@pytest.mark.parametrize("noise", ["host", "device"])
def test_noiseless_d5_rows_convert_to_zeros(hip, noise):
    c = CliffordCircuit(circuits.rotated_surface_code_memory(5, 5))
    rows = c.compile_sampler(seed=6, method="affine", noise=noise).sample(4000)
    assert (rows.any(axis=0) & ~rows.all(axis=0)).sum() > 20, "the records should carry random outcomes"
    assert not c.compile_m2d_converter().convert(measurements=rows, append_observables=True).any()


# ---- the same law as the default method (statistical: two samples of one distribution) -----------------------------------

STATISTICAL = {
    "bell": "H 0\nCX 0 1\nDEPOLARIZE2(0.05) 0 1\nX_ERROR(0.02) 0\nM(0.01) 0 1\nM 0 1",
    "bases": "RX 0\nRX 0\nM 0\nRX 0\nM 0\nR 0\nM 0",
    "d3": memory(3),
}


@pytest.mark.parametrize("name", sorted(STATISTICAL))
def test_same_law_as_the_default_method(hip, name):
    """Column means and pair means of N = 2^18 shots of each method: |difference| <= 5 sigma of the difference of two
    binomial means, sigma^2 = 2 p (1 - p) / N at the pooled p (exact agreement where both are constant)."""
    c = CliffordCircuit(STATISTICAL[name])
    N = 2**18
    a = c.compile_sampler(seed=31, method="affine").count(N, pair_columns="all")
    b = c.compile_sampler(seed=32).count(N, pair_columns="all")
    assert a.shots == b.shots == N
    for got, want in ((a.column_counts / N, b.column_counts / N), (a.pair_counts / N, b.pair_counts / N)):
        p = (got + want) / 2
        sigma = np.sqrt(2 * p * (1 - p) / N)
        assert (np.abs(got - want) <= 5 * sigma + 1e-12).all(), np.max(np.abs(got - want) / np.maximum(sigma, 1e-12))
    assert (a.column_counts > 0).any()
