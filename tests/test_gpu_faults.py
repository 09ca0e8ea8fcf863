"""The fault-driven detector sampler on the device (tsim_faults_*, csrc/tsim_faults.hip.h): the kernel's bytes against the
numpy statement ``faults.fault_rows_host`` - always the oracle, bit for bit - and the sampler's surface on a circuit."""

import numpy as np
import pytest

import shotdata_np
from test_frame import KEY

from tsim_amd import circuits, counts, faults, synth
from tsim_amd.channels import correlated_error_probs, error_probs, pauli_channel_1_probs
from tsim_amd.clifford import CliffordCircuit, pauli_channel_2_probs

pytestmark = pytest.mark.gpu

MAX_SHOT = 1 << 38
K = faults.K_GAP
DEP2 = lambda p: pauli_channel_2_probs(*([p / 15] * 15))  # noqa: E731


def pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(np.asarray(bits).astype(np.uint8), axis=1, bitorder="little")


@pytest.fixture(scope="module")
def hp(hip):
    prog = hip.HipProgram(synth.kat_h_m(), device=0)  # device buffers and a stream
    yield prog
    prog.close()


def synth_form(n_out: int, classes, seed: int, *, fan: int = 3, hot: int | None = None) -> faults.FaultForm:
    """A form from arrays: ``classes`` = ``[(outcome vector, sites)]``, the sites of the classes interleaved so that class-
    major order differs from channel order.  Every error bit flips 0 .. ``fan`` outputs drawn at random (about one list in
    four is empty; ``hot``: drawn among the first ``hot`` outputs only, so that many sites share a column and flips cancel
    inside a shot); the constants are random."""
    rng = np.random.default_rng(seed)
    left = [n for _, n in classes]
    chans = []
    while any(left):
        for i, (probs, _) in enumerate(classes):
            take = min(left[i], 1 + int(rng.integers(3)))
            chans += [np.asarray(probs, np.float64)] * take
            left[i] -= take
    masks, e = [0] * n_out, 0
    for probs in chans:
        for _ in range(int(np.log2(len(probs)))):
            n = int(rng.integers(0, fan + 2)) - 1  # -1 and 0: an empty list
            for j in (rng.choice(hot or n_out, size=min(max(n, 0), hot or n_out), replace=False) if n_out else ()):
                masks[int(j)] |= 1 << e
            e += 1
    return faults.build_form(chans, e, masks, rng.integers(0, 2, size=n_out), max(0, n_out - 2))


class Case:
    """A handle and one launch into a 0xA5-filled buffer with slack bytes."""

    def __init__(self, hp, form):
        self.hp, self.form = hp, form
        self.h = faults.FaultHandle(form)
        self.n_out = form.n_out

    def want(self, B, first_shot, key=KEY):
        return faults.fault_rows_host(self.form, first_shot, B, key)

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
        """Both layouts; all outputs, or a sub-range that starts and ends inside a byte of the packed row; the row stride a
        multiple of four bytes (dword stores) or not."""
        n_out = self.n_out
        for out_packed in (False, True):
            col0, n_cols = (0, n_out) if (i % 2 == 0 or n_out < 12) else (3, n_out - 8)
            used = (n_cols + 7) // 8 if out_packed else n_cols
            slack = (-used % 4 if i % 4 < 2 else 5) + (4 if i % 3 == 0 else 0)
            i += 1
            used, got = self.launch(B, first_shot, out_packed, col0, n_cols, slack=slack)
            w = whole[:B, col0:col0 + n_cols]
            assert np.array_equal(got[:, :used], pack(w) if out_packed else w), (first_shot, B, out_packed, col0, slack)
            assert (got[:, used:] == 0xA5).all()  # bytes past a row's outputs are not written
        return i

    def sweep(self, Bs=(1, 63, 65, 200), first_shots=(0, 64 * 7)):
        i = 0
        for first_shot in first_shots:
            whole = self.want(max(Bs), first_shot)
            for B in Bs:
                i = self.check(B, first_shot, whole, i)
                i = self.check(B, first_shot, whole, i)
        return whole

    def close(self):
        self.h.close()


MIXED = [(error_probs(0.3), 5), (DEP2(0.5), 3), (pauli_channel_1_probs(0.1, 0.2, 0.05), 4), (error_probs(1.0), 2)]


@pytest.mark.parametrize("n_out", [1, 31, 32, 33, 64, 65])
def test_column_counts(hp, n_out):
    """B = 1, 63, 65, 200 at two first shots, packed and a byte per bit, all outputs and a sub-range inside bytes."""
    case = Case(hp, synth_form(n_out, MIXED, seed=n_out))
    info = case.h.info()
    assert (info["n_out"], info["num_e"], info["n_sites"], info["n_classes"]) == (n_out, case.form.num_e, 14, 4)
    assert info["n_windows"] == 1 and info["tables_in_lds"] == 1 and info["gap_k"] == K and info["row_words"] % 2 == 1
    assert info["lds_bytes"] <= 160 * 1024 and info["waves"] == 8
    whole = case.sweep()
    assert whole.any() and not whole.all()
    case.close()


CLASSES = {
    "one site, rare": [(error_probs(1e-3), 1)],
    "one site, always": [(error_probs(1.0), 1)],
    "K + 1 sites, rare": [(error_probs(1e-3), K + 1)],
    "K + 1 sites, always": [(error_probs(1.0), K + 1)],
    "2 K + 100 sites, rare": [(error_probs(1e-3), 2 * K + 100)],
    "2 K + 100 sites, always": [(error_probs(1.0), 2 * K + 100)],
    "the law model": [(error_probs(1e-3), 2 * K + 100), (error_probs(0.3), 1), (error_probs(0.5), 3), (error_probs(1.0), 1),
                      (DEP2(0.3), 2), (DEP2(1e-3), 1), (correlated_error_probs([0.2, 0.4, 0.3]), 1)],
    "multi-bit outcomes": [(DEP2(0.9375), 40), (correlated_error_probs([0.5, 0.5, 0.5, 0.5, 0.5]), 30),
                           (pauli_channel_2_probs(*np.random.default_rng(1).dirichlet(np.ones(16))[:15]), 50)],
}


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_classes(hp, name):
    """The class shapes of the law test: 70 outputs shared by every site (flips cancel inside a shot), lists of 0 .. 3."""
    form = synth_form(70, CLASSES[name], seed=len(name), hot=9 if "always" in name else None)
    assert (np.diff(form.col_ptr) == 0).any() or form.num_e == 1
    case = Case(hp, form)
    whole = case.sweep(Bs=(65, 200), first_shots=(64 * 3,))
    if "always" in name:  # every site fires in every shot: the rows are one constant row
        assert (whole == whole[0]).all()
    else:
        assert (whole != whole[0]).any() or name == "one site, rare"
    case.close()


def test_an_error_bit_with_an_empty_list_and_one_column_under_many_sites(hp):
    masks = [sum(1 << e for e in range(0, 600, 2)), 0, 1 << 599]
    form = faults.build_form([error_probs(0.5)] * 600, 600, masks, [1, 1, 0], 3)
    assert form.col_ptr[:3].tolist() == [0, 1, 1] and form.cols[-2:].tolist() == [0, 2] and len(form.cols) == 301
    case = Case(hp, form)
    whole = case.sweep(Bs=(200,), first_shots=(0,))
    assert 60 < whole[:, 0].sum() < 140 and whole[:, 1].all() and 60 < whole[:, 2].sum() < 140
    case.close()


def test_tables_in_global_memory(hp):
    """Nine distinct fire probabilities: 36 KiB of gap rows, more than the tables' share of LDS."""
    form = synth_form(40, [(error_probs(p), 7) for p in (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0)] + [(DEP2(0.4), 5)], seed=4)
    case = Case(hp, form)
    info = case.h.info()
    assert info["tables_in_lds"] == 0 and info["n_gaps"] == 10 and info["lds_bytes"] == 8 * 256 * info["row_words"]
    case.sweep(Bs=(65, 200), first_shots=(64,))
    case.close()


def test_a_request_cut_into_launches_and_the_last_shots(hp):
    case = Case(hp, synth_form(45, CLASSES["the law model"], seed=2))
    n_out = case.n_out
    _, one = case.launch(200, 0, True, 0, n_out, slack=0)
    _, a = case.launch(128, 0, True, 0, n_out, slack=0)
    _, b = case.launch(64, 128, True, 0, n_out, slack=0)
    _, c = case.launch(8, 192, True, 0, n_out, slack=0)
    assert np.array_equal(np.concatenate([a, b, c]), one) and np.array_equal(one, pack(case.want(200, 0)))
    _, other = case.launch(200, 0, True, 0, n_out, slack=0, key=(KEY[0], KEY[1] + 1))
    assert not np.array_equal(other, one)
    for first_shot in (2**32 - 128, MAX_SHOT - 256):  # the shot index crosses 2^32; the last shots there are
        _, got = case.launch(200, first_shot, False, 0, n_out, slack=0)
        assert np.array_equal(got, case.want(200, first_shot))
    case.close()


@pytest.mark.parametrize("n_out,windows", [(3360, 1), (21000, 2)])
def test_column_windows(hp, n_out, windows):
    """21 000 outputs are more than one wave's LDS holds (18 912 next to these tables): two windows, each redrawing the stream."""
    form = synth_form(n_out, [(DEP2(0.2), 250), (error_probs(1e-3), 150), (error_probs(0.5), 40)], seed=n_out, fan=4)
    case = Case(hp, form)
    info = case.h.info()
    assert info["n_windows"] == windows and info["lds_bytes"] <= 160 * 1024 and info["window"] % 32 == 0
    assert info["window"] == (18912 if windows > 1 else 3360) and info["waves"] == (1 if windows > 1 else 5)
    whole = case.want(128, 64)
    case.check(128, 64, whole, 0)
    case.check(128, 64, whole, 1)
    if windows > 1:  # a sub-range that fits one window, across the seam of the full request's windows
        used, got = case.launch(100, 64, True, 19000, 1999, slack=3)
        assert np.array_equal(got[:, :used], pack(whole[:100, 19000:20999])) and (got[:, used:] == 0xA5).all()
    case.close()


def test_argument_errors_come_before_any_launch(hp):
    good = faults.FaultHandle(synth_form(5, MIXED, seed=1))
    d = hp.malloc(4096)
    ok = dict(key=KEY, first_shot=0, out_row_bytes=1, out_packed=True, stream=hp.stream_ptr())
    good.sample_device(64, d.ptr, **ok)
    hp.synchronize()
    for change, match in ((dict(first_shot=32), "multiple of 64"), (dict(first_shot=-64), "multiple of 64"),
                          (dict(out_row_bytes=0), "out_row_bytes"), (dict(out_packed=False, out_row_bytes=1), "out_row_bytes"),
                          (dict(col0=4, n_cols=2), "outputs"), (dict(first_shot=2**38), "2\\^38")):
        with pytest.raises(ValueError, match=match):
            good.sample_device(64, d.ptr, **{**ok, **change})
    with pytest.raises(ValueError, match="NULL"):
        good.sample_device(64, 0, **ok)
    with pytest.raises(ValueError, match="negative"):
        good.sample_device(-1, d.ptr, **ok)
    good.sample_device(64, d.ptr, **{**ok, "first_shot": 2**38 - 64})  # the last word there is
    good.sample_device(0, 0, **ok)
    hp.synchronize()
    d.free()
    good.close()


# ---- the sampler ------------------------------------------------------------------------------------------------------

D3 = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.01, before_round_data_depolarization=0.01,
                                          before_measure_flip_probability=0.01)
SHOTS, BS = 2500, 1000  # three chunks of 1024, 1024, 452 rows
_rows: dict = {}


def host_rows(seed: int) -> np.ndarray:
    """What the host statement gives for the seed's first request: computed once, shared, left unchanged."""
    if seed not in _rows:
        s = CliffordCircuit(D3).compile_detector_sampler(seed=seed, method="faults")
        rows = faults.fault_rows_host(s._form, 0, SHOTS, s._next_key()).view(np.bool_)
        rows.setflags(write=False)
        _rows[seed] = rows
    return _rows[seed]


def test_detector_sampler(hip, tmp_path):
    c = CliffordCircuit(D3)
    rows = host_rows(8)
    mk = lambda: c.compile_detector_sampler(seed=8, method="faults")  # noqa: E731
    nd, n_out = mk().num_detectors, rows.shape[1]
    det, obs = rows[:, :nd], rows[:, nd:]
    ref = mk()._compute_reference_sample()
    assert rows.any() and n_out - nd == mk().num_observables == 1
    for packed in (False, True):
        out = (lambda a: pack(a)) if packed else (lambda a: a)
        kw = dict(batch_size=BS, bit_packed=packed)
        assert np.array_equal(mk().sample(SHOTS, **kw), out(det))
        assert np.array_equal(mk().sample(SHOTS, append_observables=True, **kw), out(rows))
        assert np.array_equal(mk().sample(SHOTS, prepend_observables=True, **kw), out(np.concatenate([obs, det], axis=1)))
        a, b = mk().sample(SHOTS, separate_observables=True, **kw)
        assert np.array_equal(a, out(det)) and np.array_equal(b, out(obs))
        flipped = mk().sample(SHOTS, append_observables=True, use_detector_reference_sample=True,
                              use_observable_reference_sample=True, **kw)
        assert np.array_equal(flipped, out(rows ^ ref))
        mask = np.zeros(nd, np.bool_)
        mask[:1] = True
        assert np.array_equal(mk().sample(SHOTS, postselection_mask=mask, **kw), out(det))
    assert np.array_equal(mk().sample(SHOTS), det)  # whatever the batch size
    s = mk()
    assert np.array_equal(s.sample(640), det[:640]) and not np.array_equal(s.sample(640), det[:640])  # one key per request
    assert np.array_equal(c.compile_detector_sampler(seed=8, method="faults", noise="device").sample(SHOTS), det)
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
    # sample_write(): b8 decodes back to the rows
    path, opath = tmp_path / "d3.b8", tmp_path / "d3.obs.b8"
    mk().sample_write(SHOTS, filepath=path, format="b8", append_observables=True, batch_size=BS)
    assert np.array_equal(shotdata_np.decode("b8", path.read_bytes(), n_out, (0, nd, n_out - nd)), rows)
    mk().sample_write(SHOTS, filepath=path, format="b8", obs_out_filepath=opath, obs_out_format="b8", batch_size=BS)
    assert np.array_equal(shotdata_np.decode("b8", path.read_bytes(), nd, (0, nd, 0)), det)
    assert np.array_equal(shotdata_np.decode("b8", opath.read_bytes(), n_out - nd, (0, 0, n_out - nd)), obs)


def test_d7_memory_circuit_rows(hp):
    """A circuit's own form (1897 sites in three classes, 337 outputs) through the handle."""
    text = circuits.rotated_surface_code_memory(7, 7, after_clifford_depolarization=1e-3, before_measure_flip_probability=1e-3)
    form = CliffordCircuit(text).compile_faults()
    assert (form.n_out, form.n_sites, form.n_classes) == (337, 1897, 3)
    case = Case(hp, form)
    whole = case.sweep(Bs=(640,), first_shots=(64 * 100,))
    assert 0.002 < whole.mean() < 0.02
    case.close()
