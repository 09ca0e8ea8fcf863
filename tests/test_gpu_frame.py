"""The Pauli-frame sampler on the device (tsim_frame_*, csrc/tsim_frame.hip.h): the kernels' bytes against the numpy statement
``frame.frame_rows_host`` - always the oracle, bit for bit - and the samplers' surface on circuits."""

import numpy as np
import pytest

import shotdata_np
from test_frame import FEEDBACK, KEY, SIZES, random_circuit

from tsim_amd import circuits, counts, frame, shotdata, synth
from tsim_amd.clifford import CliffordCircuit

pytestmark = pytest.mark.gpu

MAX_SHOT = 1 << 38


def pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(np.asarray(bits).astype(np.uint8), axis=1, bitorder="little")


@pytest.fixture(scope="module")
def hp(hip):
    prog = hip.HipProgram(synth.kat_h_m(), device=0)  # device buffers and a stream
    yield prog
    prog.close()


class _NoTableau:
    """The frame operations do not depend on the tableau (a 10240-qubit one takes 400 MB): constants and a fresh symbol for
    every third measurement stand in for it where only the kernels are compared with the host statement."""

    def __init__(self):
        self.n_random, self.calls = 0, 0

    def h(self, a): pass  # noqa: E704
    def s(self, a): pass  # noqa: E704
    def cx(self, a, b): pass  # noqa: E704
    def pauli(self, a, px, pz): pass  # noqa: E704
    def pauli_if(self, a, sym_mask, px=1, pz=0): pass  # noqa: E704

    def measure_z(self, a):
        self.calls += 1
        if self.calls % 3 == 0:
            self.n_random += 1
            return 0, 1 << (self.n_random - 1)
        return self.calls & 1, 0


def form_of(text: str, kind: str = "measurements", *, n_qubits: int | None = None) -> frame.FrameForm:
    """``n_qubits``: that many circuit qubits, walked without a tableau."""
    c = CliffordCircuit(text)
    if n_qubits is None:
        return c.compile_frame(kind)
    rec = frame._FrameRecorder(n_qubits, tableau=_NoTableau())
    c._walk(rec)
    return frame.build_form(rec, kind)


class Case:
    """A handle and one launch into a 0xA5-filled buffer with slack bytes."""

    def __init__(self, hp, form):
        self.hp, self.form = hp, form
        self.h = frame.FrameHandle(form)
        self.n_out = form.n_out

    def want(self, B, first_shot, key=KEY):
        return frame.frame_rows_host(self.form, B, first_shot, key)

    def launch(self, B, first_shot, out_packed, col0, n_cols, *, slack=5, key=KEY):
        used = (n_cols + 7) // 8 if out_packed else n_cols
        rb = used + slack
        got = np.full((B, rb), 0xA5, np.uint8)
        d_out = self.hp.malloc(max(1, got.nbytes))
        self.hp.h2d(d_out, got)
        self.h.sample_device(B, d_out.ptr, key=key, first_shot=first_shot, out_row_bytes=rb, out_packed=out_packed, col0=col0,
                             n_cols=n_cols, stream=self.hp.stream_ptr())
        self.hp.synchronize()
        self.hp.d2h(got, d_out)
        d_out.free()
        return used, got

    def check(self, B, first_shot, whole, i):
        """Both layouts; all outputs, or a sub-range that starts and ends inside a byte of the packed row."""
        n_out = self.n_out
        for out_packed in (False, True):
            col0, n_cols = (0, n_out) if (i % 2 == 0 or n_out < 12) else (3, n_out - 8)
            i += 1
            used, got = self.launch(B, first_shot, out_packed, col0, n_cols)
            w = whole[:B, col0:col0 + n_cols]
            assert np.array_equal(got[:, :used], pack(w) if out_packed else w), (first_shot, B, out_packed, col0)
            assert (got[:, used:] == 0xA5).all()  # bytes past a row's outputs are not written
        return i

    def close(self):
        self.h.close()


def sweep(case: Case):
    """B in {1, 63, 64, 65, 64 T + 1, 3 x 64 T} x first_shot in {0, 64, 64 T, the last multiple of 64 that leaves room}."""
    T = case.h.info()["T"]
    Bs = (1, 63, 64, 65, 64 * T + 1, 3 * 64 * T)
    i = 0
    for first_shot in (0, 64, 64 * T, (MAX_SHOT - max(Bs)) // 64 * 64):
        whole = case.want(max(Bs), first_shot)
        for B in Bs:
            i = case.check(B, first_shot, whole, i)
    # rows exactly as wide as their outputs (the contiguous store path for rows of at most 64 bytes), up to the last shot
    whole = case.want(200, MAX_SHOT - 256)
    for out_packed in (False, True):
        _, got = case.launch(200, MAX_SHOT - 256, out_packed, 0, case.n_out, slack=0)
        assert np.array_equal(got, pack(whole) if out_packed else whole)


# qubit counts (the auxiliary qubit included) at which T changes: 16 bytes per qubit and word in 160 KiB
BOUNDARIES = [(320, 32), (321, 16), (640, 16), (641, 8), (1280, 8), (1281, 4), (2560, 4), (2561, 2), (5120, 2), (5121, 1), (10240, 1)]


@pytest.mark.parametrize("nq,T", [(2, 32), (3, 32)] + BOUNDARIES)
def test_kernel_matches_host_statement_at_every_tile_size(hp, nq, T):
    """``nq`` - 1 circuit qubits (1, 2, and one on each side of every boundary of T, up to the largest a handle takes) under
    about a hundred random operations."""
    n = nq - 1
    form = form_of(random_circuit(n, 100 if nq == 10240 else 40, seed=nq), n_qubits=n if n > 70 else None)
    assert form.n_qubits == nq or (n <= 2 and form.n_qubits == 3)  # (MPAD's 0 / 1 count as qubit numbers)
    case = Case(hp, form)
    info = case.h.info()
    assert info["T"] == T and info["lds_bytes"] == 16 * form.n_qubits * T <= 160 * 1024 and info["max_qubits"] == 10240
    assert (info["n_qubits"], info["n_records"], info["n_hidden"], info["n_out"]) == (form.n_qubits, form.n_records, form.n_hidden,
                                                                                     form.n_out)
    sweep(case)
    case.close()


RECORDS = {
    0: "H 0\nX_ERROR(0.5) 0",
    1: "X_ERROR(0.5) 0\nM 0",
    65: "H 0\n" + "M(0.1) 0\n" * 65,
    2100: "H 0 1\n" + "M(0.01) 0 1\n" * 1050,
    # more column masks than one wave's LDS holds (7640): the output stage windows
    7700: "H 0 1\n" + ("X_ERROR(0.2) 0\nM 0 1\nM(0.05) 0 1\n" + "M 0 1\n" * 8) * 385,
}


@pytest.mark.parametrize("n_rec", sorted(RECORDS))
def test_record_counts(hp, n_rec):
    form = form_of(RECORDS[n_rec])
    assert form.n_records == form.n_out == n_rec
    case = Case(hp, form)
    info = case.h.info()
    assert (info["n_windows"] > 1) == (n_rec == 7700)
    if n_rec == 0:
        used, got = case.launch(70, 64, True, 0, 0)
        assert used == 0 and (got == 0xA5).all()
    else:
        i = 0
        for first_shot, B in ((0, 65), (64 * (2**20 + 3), 130)):
            whole = case.want(B, first_shot)
            i = case.check(B, first_shot, whole, i + 1)  # (a sub-range, then all outputs)
            i = case.check(B, first_shot, whole, i + 1)
    case.close()


def test_batches_of_one_item_and_of_hundreds(hp):
    single = form_of("H 0\nS 0\nX_ERROR(0.3) 0\nH 0\nM 0\nCX rec[-1] 0\nH 0\nZ_ERROR(0.2) 0\nH 0\nM 0")
    case = Case(hp, single)
    assert case.h.info()["max_batch_items"] == 1 and case.h.info()["n_batches"] == single.n_batches == single.n_ops
    sweep(case)
    case.close()
    qs = list(range(600))
    pairs = " ".join(f"{a} {a + 1}" for a in qs[::2])
    text = (f"H {' '.join(map(str, qs[::2]))}\nCX {pairs}\nDEPOLARIZE2(0.2) {pairs}\nX_ERROR(0.1) {' '.join(map(str, qs))}\n"
            f"M(0.05) {' '.join(map(str, qs))}\nCX rec[-1] 0 rec[-2] 5\nMR {' '.join(map(str, qs[:50]))}")
    wide = form_of(text, n_qubits=600)
    case = Case(hp, wide)
    info = case.h.info()
    assert info["max_batch_items"] == 600 and info["n_batches"] < 16 and info["T"] == 16
    sizes = np.diff(wide.batch_ptr)
    assert sorted(sizes.tolist())[-4:] == [300, 600, 600, 600]  # DEPOLARIZE2 / CX+H..., X_ERROR, MEASURE, its flips
    sweep(case)
    case.close()


@pytest.mark.parametrize("n_qubits,n_ops", SIZES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_operation_and_channel_kind(hp, n_qubits, n_ops, seed):
    """The random circuits of test_frame (every gate, channel kind and fire probability 0, 1 and in between), both forms."""
    c = CliffordCircuit(random_circuit(n_qubits, n_ops, 1000 * n_qubits + seed))
    for kind in ("measurements", "detectors"):
        form = c.compile_frame(kind)
        if not form.n_out:
            continue
        case = Case(hp, form)
        first_shot = 64 * (seed - 1)
        case.check(200, first_shot, case.want(200, first_shot), seed)
        case.close()


@pytest.mark.parametrize("n_qubits", [5, 70])
def test_a_request_cut_in_two_equals_one_launch(hp, n_qubits):
    case = Case(hp, form_of(random_circuit(n_qubits, 60, 1000 * n_qubits + 2)))
    n_out = case.n_out
    _, one = case.launch(200, 0, True, 0, n_out, slack=0)
    _, a = case.launch(128, 0, True, 0, n_out, slack=0)
    _, b = case.launch(72, 128, True, 0, n_out, slack=0)
    assert np.array_equal(np.concatenate([a, b]), one)
    assert np.array_equal(one, pack(case.want(200, 0)))
    _, other = case.launch(200, 0, True, 0, n_out, slack=0, key=(KEY[0], KEY[1] + 1))
    assert not np.array_equal(other, one)
    case.close()


def test_a_launch_larger_than_the_scratch(hp):
    """7700 records leave room for 4352 words in the 256 MiB of flip words: 278 658 shots are two launches inside the call."""
    form = form_of(RECORDS[7700])
    case = Case(hp, form)
    words = case.h.info()["max_words"]
    assert words == (256 << 20) // (8 * 7700) // 32 * 32 == 4352
    B, col0, n_cols = 64 * words + 130, 3803, 61
    _, got = case.launch(B, 64, True, col0, n_cols, slack=0)
    seam = 64 * words  # the rows on both sides of the seam, and the first ones
    assert np.array_equal(got[seam - 128:seam + 128], pack(frame.frame_rows_host(form, 256, 64 + seam - 128, KEY)[:, col0:col0 + n_cols]))
    assert np.array_equal(got[:100], pack(case.want(100, 64)[:, col0:col0 + n_cols]))
    case.close()


def test_argument_errors_come_before_any_launch(hp):
    good = frame.FrameHandle(form_of("H 0\nM(0.1) 0 1"))
    d = hp.malloc(4096)
    ok = dict(key=KEY, first_shot=0, out_row_bytes=1, out_packed=True, stream=hp.stream_ptr())
    good.sample_device(64, d.ptr, **ok)
    hp.synchronize()
    for change, match in ((dict(first_shot=32), "multiple of 64"), (dict(first_shot=-64), "multiple of 64"),
                          (dict(out_row_bytes=0), "out_row_bytes"), (dict(out_packed=False, out_row_bytes=1), "out_row_bytes"),
                          (dict(col0=1, n_cols=2), "outputs"), (dict(first_shot=2**38), "2\\^38")):
        with pytest.raises(ValueError, match=match):
            good.sample_device(64, d.ptr, **{**ok, **change})
    with pytest.raises(ValueError, match="NULL"):
        good.sample_device(64, 0, **ok)
    with pytest.raises(ValueError, match="negative"):
        good.sample_device(-1, d.ptr, **ok)
    good.sample_device(64, d.ptr, **{**ok, "first_shot": 2**38 - 64})  # the last word there is
    hp.synchronize()
    d.free()
    good.close()


# ---- the samplers -----------------------------------------------------------------------------------------------------

D3 = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.01, before_round_data_depolarization=0.01,
                                          before_measure_flip_probability=0.01)
CIRCUITS = {"d3": D3, "feedback": FEEDBACK}
SHOTS, BS = 2500, 1000  # three chunks of 1024, 1024, 452 rows
_rows: dict = {}


def host_rows(name: str, kind: str, seed: int) -> np.ndarray:
    """What the host-statement sampler gives for the seed: computed once, shared, left unchanged."""
    if (name, kind, seed) not in _rows:
        c = CliffordCircuit(CIRCUITS[name])
        s = c.compile_sampler(seed=seed, method="frame") if kind == "measurements" else c.compile_detector_sampler(seed=seed, method="frame")
        rows = frame.frame_rows_host(s._form, SHOTS, 0, s._next_key()).view(np.bool_)
        rows.setflags(write=False)
        _rows[name, kind, seed] = rows
    return _rows[name, kind, seed]


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_measurement_sampler(hip, tmp_path, name, noise):
    c = CliffordCircuit(CIRCUITS[name])
    M = c.num_measurements
    rows = host_rows(name, "measurements", 9)
    mk = lambda: c.compile_sampler(seed=9, method="frame", noise=noise)  # noqa: E731
    got = mk().sample(SHOTS, batch_size=BS)
    assert got.dtype == np.bool_ and np.array_equal(got, rows) and rows.any()
    assert np.array_equal(mk().sample(SHOTS), rows)
    assert np.array_equal(mk().sample(SHOTS, BS, True), pack(rows))
    s = mk()
    assert np.array_equal(s.sample(640), rows[:640]) and not np.array_equal(s.sample(640), rows[:640])  # one key per request
    got = mk().count(SHOTS, batch_size=BS, pair_columns="all", pattern_columns="all")
    assert got == counts.tally_rows(rows, num_detectors=0, histogram_columns=got.histogram_columns, pair_columns="all",
                                    pattern_columns="all")
    assert got.shots == got.kept == SHOTS and np.array_equal(got.column_counts, rows.sum(axis=0))
    for fmt in ("b8", "dets"):
        path = tmp_path / f"{name}.{fmt}"
        mk().sample_write(SHOTS, filepath=path, format=fmt, batch_size=BS)
        assert np.array_equal(shotdata_np.decode(fmt, path.read_bytes(), M, (M, 0, 0)), rows), fmt
        assert np.array_equal(shotdata.read_shot_data_file(path=path, format=fmt, num_measurements=M), rows), fmt


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_detector_sampler(hip, tmp_path, name):
    c = CliffordCircuit(CIRCUITS[name])
    rows = host_rows(name, "detectors", 8)
    mk = lambda: c.compile_detector_sampler(seed=8, method="frame")  # noqa: E731
    nd, n_out = mk().num_detectors, rows.shape[1]
    det, obs = rows[:, :nd], rows[:, nd:]
    ref = mk()._compute_reference_sample()
    assert rows.any() and n_out - nd == mk().num_observables == 1
    # every layout and keyword combination
    for packed in (False, True):
        out = (lambda a: pack(a)) if packed else (lambda a: a)
        kw = dict(batch_size=BS, bit_packed=packed)
        assert np.array_equal(mk().sample(SHOTS, **kw), out(det))
        assert np.array_equal(mk().sample(SHOTS, append_observables=True, **kw), out(rows))
        assert np.array_equal(mk().sample(SHOTS, prepend_observables=True, **kw), out(np.concatenate([obs, det], axis=1)))
        assert np.array_equal(mk().sample(SHOTS, prepend_observables=True, append_observables=True, **kw),
                              out(np.concatenate([obs, det, obs], axis=1)))
        a, b = mk().sample(SHOTS, separate_observables=True, **kw)
        assert np.array_equal(a, out(det)) and np.array_equal(b, out(obs))
        flipped = mk().sample(SHOTS, append_observables=True, use_detector_reference_sample=True,
                              use_observable_reference_sample=True, **kw)
        assert np.array_equal(flipped, out(rows ^ ref))
        mask = np.zeros(nd, np.bool_)
        mask[:1] = True
        assert np.array_equal(mk().sample(SHOTS, postselection_mask=mask, **kw), out(det))
    assert np.array_equal(mk().sample(SHOTS), det)  # whatever the batch size
    # count(): plain, post-selected, pairs, patterns
    mask = np.zeros(nd, np.bool_)
    mask[0] = True
    for kw in (dict(), dict(postselection_mask=mask), dict(pair_columns="all"), dict(pattern_columns="detectors"),
               dict(postselection_mask=mask, pair_columns="detectors", pattern_columns="all",
                    use_detector_reference_sample=True, use_observable_reference_sample=True)):
        got = mk().count(SHOTS, batch_size=BS, **kw)
        tkw = {k: v for k, v in kw.items() if not k.startswith("use_")}
        base = rows ^ ref if "use_detector_reference_sample" in kw else rows
        assert got == counts.tally_rows(base, num_detectors=nd, histogram_columns=got.histogram_columns, **tkw), kw
        assert got.shots == SHOTS and got.kept == (SHOTS if "postselection_mask" not in kw else int((~base[:, 0]).sum()))
    # sample_write(): b8 and dets decode back to the rows
    for fmt in ("b8", "dets"):
        path, opath = tmp_path / f"{name}.{fmt}", tmp_path / f"{name}.obs.{fmt}"
        mk().sample_write(SHOTS, filepath=path, format=fmt, append_observables=True, batch_size=BS)
        assert np.array_equal(shotdata_np.decode(fmt, path.read_bytes(), n_out, (0, nd, n_out - nd)), rows), fmt
        mk().sample_write(SHOTS, filepath=path, format=fmt, obs_out_filepath=opath, obs_out_format=fmt, batch_size=BS)
        assert np.array_equal(shotdata_np.decode(fmt, path.read_bytes(), nd, (0, nd, 0)), det), fmt
        assert np.array_equal(shotdata_np.decode(fmt, opath.read_bytes(), n_out - nd, (0, 0, n_out - nd)), obs), fmt
    # the records of the measurement sampler, converted, are the detector sampler's rows for the same seed
    meas = c.compile_sampler(seed=8, method="frame").sample(SHOTS)
    assert np.array_equal(c.compile_m2d_converter().convert(measurements=meas, append_observables=True), rows)


def test_gauge_detector_on_the_device(hip):
    c = CliffordCircuit("R 0\nH 0\nM 0\nDETECTOR rec[-1]")
    s = c.compile_detector_sampler(seed=1, method="frame")
    key = c.compile_detector_sampler(seed=1, method="frame")._next_key()
    rows = s.sample(300)
    assert np.array_equal(rows, frame.frame_rows_host(s._form, 300, 0, key).view(np.bool_)) and 100 < rows.sum() < 200
