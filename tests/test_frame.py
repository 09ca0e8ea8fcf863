"""The Pauli-frame sampler without a device: the recorder and the numpy statement ``frame.frame_rows_host`` against the
symbolic analysis (independent code), the noiseless rows against ``method="affine"``, the law of the error bits against
``noise_law``, gauge detectors, independence from how a request is cut, a worked example and the size of the form."""

import ctypes as C

import numpy as np
import pytest

import noise_law
from test_affine import EXHAUSTIVE, WORKED

from tsim_amd import _lib, affine, circuits, frame
from tsim_amd.clifford import _ACTION_1Q, _TWO_QUBIT, CliffordCircuit, _bits

KEY = (0x243F6A88, 0x85A308D3)


# ---- random circuits over the whole gate table -----------------------------------------------------------------------------

def random_circuit(n_qubits: int, n_ops: int, seed: int, *, noise: bool = True, detectors: bool = True) -> str:
    """A few dozen operations: every kind of gate, measurement, reset, feedback and noise channel can occur; fire
    probabilities 0, 1 and in between."""
    rng = np.random.default_rng(seed)
    one, two = sorted(_ACTION_1Q), sorted(_TWO_QUBIT)
    lines, n_rec = [], 0
    turn = [7 * seed, 5 * seed]  # gates are taken in turn from the tables, so that a handful of circuits covers them all
    q = lambda: int(rng.integers(n_qubits))  # noqa: E731
    prob = lambda: [0.0, 1.0, 0.3, 0.05, 0.5][int(rng.integers(5))]  # noqa: E731

    def pair():
        a, b = rng.choice(n_qubits, size=2, replace=False)
        return int(a), int(b)

    def product(k):
        qs = rng.choice(n_qubits, size=min(k, n_qubits), replace=False)
        return [("XYZ"[int(rng.integers(3))], int(v)) for v in qs]

    kinds = ["g1", "g1", "g2", "g2", "m", "mr", "r", "mpp", "mpad", "spp", "fb"]
    if n_qubits < 2:
        kinds = [k for k in kinds if k != "g2"]
    if noise:
        kinds += ["e1", "dep1", "pc1", "her", "corr", "mnoisy"] + (["dep2", "pc2"] if n_qubits >= 2 else [])
    for _ in range(n_ops):
        k = kinds[int(rng.integers(len(kinds)))]
        if k == "g1":
            for _j in range(3):
                turn[0] += 1
                lines.append(f"{one[turn[0] % len(one)]} {q()}")
        elif k == "g2":
            for _j in range(3):
                a, b = pair()
                turn[1] += 1
                lines.append(f"{two[turn[1] % len(two)]} {a} {b}")
        elif k == "m":
            lines.append(f"{['M', 'MX', 'MY'][int(rng.integers(3))]} {'!' if rng.integers(2) else ''}{q()}")
            n_rec += 1
        elif k == "mnoisy":
            lines.append(f"{['M', 'MX', 'MY', 'MR', 'MRX'][int(rng.integers(5))]}({prob()}) {q()}")
            n_rec += 1
        elif k == "mr":
            lines.append(f"{['MR', 'MRX', 'MRY'][int(rng.integers(3))]} {q()}")
            n_rec += 1
        elif k == "r":
            lines.append(f"{['R', 'RX', 'RY'][int(rng.integers(3))]} {q()}")
        elif k == "mpp":
            if n_qubits >= 2 and rng.integers(2):
                a, b = pair()
                lines.append(f"{['MXX', 'MYY', 'MZZ'][int(rng.integers(3))]}{'(0.3)' if noise and rng.integers(2) else ''} {a} {b}")
            else:
                body = "*".join(f"{p}{v}" for p, v in product(int(rng.integers(1, 4))))
                lines.append(f"MPP{'(0.3)' if noise and rng.integers(2) else ''} {'!' if rng.integers(2) else ''}{body}")
            n_rec += 1
        elif k == "mpad":
            lines.append(f"MPAD{f'({prob()})' if noise and rng.integers(2) else ''} {int(rng.integers(2))}")
            n_rec += 1
        elif k == "spp":
            body = "*".join(f"{p}{v}" for p, v in product(int(rng.integers(1, 4))))
            lines.append(f"{['SPP', 'SPP_DAG'][int(rng.integers(2))]} {body}")
        elif k == "fb":
            if n_rec:
                back = int(rng.integers(1, min(n_rec, 5) + 1))
                form = int(rng.integers(5))
                if form < 3:
                    lines.append(f"{['CX', 'CY', 'CZ'][form]} rec[-{back}] {q()}")
                elif form == 3:
                    lines.append(f"CZ {q()} rec[-{back}]")
                else:
                    lines.append(f"{['XCZ', 'YCZ'][int(rng.integers(2))]} {q()} rec[-{back}]")
        elif k == "e1":
            lines.append(f"{['X_ERROR', 'Y_ERROR', 'Z_ERROR'][int(rng.integers(3))]}({prob()}) {q()}")
        elif k == "dep1":
            lines.append(f"DEPOLARIZE1({[0.0, 0.3, 0.75][int(rng.integers(3))]}) {q()}")
        elif k == "pc1":
            lines.append(f"PAULI_CHANNEL_1({['0.1, 0.2, 0.05', '0, 0, 0', '0.5, 0.25, 0.25'][int(rng.integers(3))]}) {q()}")
        elif k == "dep2":
            a, b = pair()
            lines.append(f"DEPOLARIZE2({[0.0, 0.3, 0.9375][int(rng.integers(3))]}) {a} {b}")
        elif k == "pc2":
            a, b = pair()
            ps = rng.dirichlet(np.ones(16))[:15] * [0.5, 1.0][int(rng.integers(2))]
            lines.append(f"PAULI_CHANNEL_2({', '.join(f'{p:.6f}' for p in ps)}) {a} {b}")
        elif k == "her":
            if rng.integers(2):
                lines.append(f"HERALDED_ERASE({[0.0, 0.4, 1.0][int(rng.integers(3))]}) {q()}")
            else:
                lines.append(f"HERALDED_PAULI_CHANNEL_1(0.1, 0.2, 0.05, 0.15) {q()}")
            n_rec += 1
        elif k == "corr":
            body = " ".join(f"{p}{v}" for p, v in product(int(rng.integers(1, 4))))
            lines.append(f"E({prob()}) {body}")
            for _j in range(int(rng.integers(3))):
                if rng.integers(3) == 0:  # something between the branches of the chain
                    lines.append(f"H {q()}")
                body = " ".join(f"{p}{v}" for p, v in product(int(rng.integers(1, 4))))
                lines.append(f"ELSE_CORRELATED_ERROR({prob()}) {body}")
        if detectors and n_rec and rng.integers(4) == 0:
            recs = sorted({int(v) for v in rng.integers(1, n_rec + 1, size=int(rng.integers(1, 4)))})
            name = "DETECTOR" if rng.integers(3) else f"OBSERVABLE_INCLUDE({int(rng.integers(3))})"
            lines.append(f"{name} " + " ".join(f"rec[-{v}]" for v in recs))
    if not n_rec:
        lines.append("M 0")
    return "\n".join(lines)


def word_bits(words: np.ndarray, B: int) -> np.ndarray:
    """``uint64[n, ceil(B / 64)]`` -> ``uint8[B, n]``."""
    n, nw = words.shape
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(n, nw * 8), axis=1, bitorder="little")[:, :B].T


def analysis_rows(an, outputs, e_bits, sym_bits):
    out = np.zeros((len(e_bits), len(outputs)), np.uint8)
    for j, (s, v, y) in enumerate(outputs):
        col = np.full(len(e_bits), int(v) & 1, np.uint8)
        for e in _bits(int(s)):
            col ^= e_bits[:, e]
        for r in _bits(int(y)):
            col ^= sym_bits[:, r]
        out[:, j] = col
    return out


def gauge_analysis(c: CliffordCircuit):
    """``analyze()`` with detectors whose symbols do not cancel allowed (the symbolic terms are still all there)."""
    from tsim_amd.clifford import _Sim

    class Sim(_Sim):
        allow_gauge = True

    return c._walk(Sim(max(1, c._qubit_count())))


SIZES = [(1, 30), (2, 40), (5, 60), (70, 60)]


@pytest.mark.parametrize("n_qubits,n_ops", SIZES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_propagation_against_the_symbolic_analysis(n_qubits, n_ops, seed):
    text = random_circuit(n_qubits, n_ops, 1000 * n_qubits + seed)
    c = CliffordCircuit(text)
    an = gauge_analysis(c)
    B, first_shot = 200, 64 * (seed - 1)
    n_random = max((int(y).bit_length() for y in an.rec_syms), default=0)
    sym = affine.random_words(KEY, n_random, first_shot // 64, (B + 63) // 64)  # [nw, n_random]
    sym_bits = word_bits(sym.T, B) if n_random else np.zeros((B, 0), np.uint8)
    form = c.compile_frame("measurements")
    assert form.num_e == an.num_e and form.n_random == n_random and form.n_records == len(an.rec_sets)
    assert len(form.channel_probs) == len(an.channel_probs)
    assert all(np.array_equal(a, b) for a, b in zip(form.channel_probs, an.channel_probs))
    rows, e = frame.frame_rows_host(form, B, first_shot, KEY, return_e=True)
    e_bits = word_bits(e, B) if an.num_e else np.zeros((B, 0), np.uint8)
    want = analysis_rows(an, list(zip(an.rec_sets, an.rec_vals, an.rec_syms)), e_bits, sym_bits)
    assert rows.dtype == np.uint8 and np.array_equal(rows, want), text
    # the detector form: detectors in order, then observables by index
    dform = c.compile_frame("detectors")
    keys = sorted(an.observables)
    outputs = [(s, v, y) for (s, v), y in zip(an.detectors, an.detector_syms)] + [tuple(an.observables[k]) for k in keys]
    assert dform.n_out == len(outputs) and dform.num_detectors == len(an.detectors)
    drows, de = frame.frame_rows_host(dform, B, first_shot, KEY, return_e=True)
    assert np.array_equal(de, e)
    assert np.array_equal(drows, analysis_rows(an, outputs, e_bits, sym_bits)), text


def test_the_random_circuits_cover_every_kind():
    texts = "\n".join(random_circuit(n, k, 1000 * n + s) for n, k in SIZES for s in (1, 2, 3))
    names = {ln.split("(")[0].split()[0] for ln in texts.splitlines()}
    for name in ("MPP", "MXX", "MR", "MRX", "MPAD", "HERALDED_ERASE", "HERALDED_PAULI_CHANNEL_1", "E", "ELSE_CORRELATED_ERROR",
                 "DEPOLARIZE1", "DEPOLARIZE2", "PAULI_CHANNEL_1", "PAULI_CHANNEL_2", "X_ERROR", "SPP", "DETECTOR", "OBSERVABLE_INCLUDE",
                 "R", "RX", *_ACTION_1Q, *_TWO_QUBIT):
        assert name in names, name
    assert "rec[-" in texts and "(0.0)" in texts and "(1.0)" in texts and "(0.3)" in texts
    kinds = set()
    for n, k in SIZES:
        kinds |= set(CliffordCircuit(random_circuit(n, k, 1000 * n + 1)).compile_frame().op_kind.tolist())
    assert kinds == set(range(7))


# ---- noiseless circuits: the rows of method="affine" ------------------------------------------------------------------------

NOISELESS = dict(EXHAUSTIVE, d3x2=circuits.rotated_surface_code_memory(3, 2), coin="H 0\n" + "M 0\n" * 70)


@pytest.mark.parametrize("name", sorted(NOISELESS))
def test_noiseless_rows_equal_the_affine_method(name):
    c = CliffordCircuit(NOISELESS[name])
    want = c.compile_sampler(seed=17, method="affine", noise="host")._sample_direct(1000)
    s = c.compile_sampler(seed=17, method="frame")
    got = frame.frame_rows_host(s._form, 1000, 0, s._next_key()).view(np.bool_)
    assert got.shape == (1000, c.num_measurements) and np.array_equal(got, want)


# ---- the law of the error bits --------------------------------------------------------------------------------------------

def law_model():
    """One site of each channel kind at fire probabilities 1e-3, 0.3 and 1; every error bit lands in a place of its own, so
    nothing but the draw shapes its law.  Qubits are measured nowhere: the e bits are read from the statement directly."""
    lines, q = [], 0
    for p in (1e-3, 0.3, 1.0):
        lines += [f"X_ERROR({p}) {q}", f"DEPOLARIZE1({p}) {q + 1}", f"PAULI_CHANNEL_1({p / 2}, {p / 4}, {p / 4}) {q + 2}",
                  f"DEPOLARIZE2({p}) {q + 3} {q + 4}", f"HERALDED_ERASE({p}) {q + 5}", f"M({p}) {q + 6}", f"MPAD({p}) 0",
                  f"E({p / 2}) X{q + 7}", f"ELSE_CORRELATED_ERROR({p}) Z{q + 8}"]
        q += 9
    return CliffordCircuit("\n".join(lines))


@pytest.fixture(scope="module")
def law_rows():
    c = law_model()
    form = c.compile_frame()
    B = 1 << 20
    _, e = frame.frame_rows_host(form, B, 64 * 5, (7, 11), return_e=True)
    return c, form, B, frame.e_rows(e, B)


def test_law_of_the_error_bits(law_rows):
    c, form, B, packed = law_rows
    probs = form.channel_probs
    num_e = form.num_e
    assert packed.shape == (B, (num_e + 63) // 64) and num_e == 3 * (1 + 2 + 2 + 4 + 3 + 1 + 1 + 2)
    T = np.eye(num_e, dtype=np.uint8)
    groups, at = [], 0
    for p in probs:
        k = int(np.log2(len(p)))
        groups.append(list(range(at, at + k)))
        at += k
    masks = noise_law.standard_masks(num_e, groups, np.random.default_rng(3))
    noise_law.check_biases(noise_law.empirical_bias(packed, masks), noise_law.parity_bias(probs, T, masks), B, masks)


@pytest.mark.parametrize("M", [64, 192])
def test_fire_rate_in_every_position_class(law_rows, M):
    """One-bit sites of one rate fire at that rate in every class ``shot mod M``: word seams are a class."""
    c, form, B, packed = law_rows
    for p in (1e-3, 0.3, 1.0):
        bits = [int(form.site_e0[n]) for n in range(len(form.site_chan))
                if len(form.channel_probs[form.site_chan[n]]) == 2 and form.channel_probs[form.site_chan[n]][1] == p]
        assert len(bits) == 3  # X_ERROR, M(p), MPAD(p)
        noise_law.check_position_classes(packed, bits, p, M)


def test_tables_of_the_draw():
    g = frame.gap_thresholds(1.0)
    assert g.dtype == np.uint32 and not g.any()  # an always-firing site skips nothing
    g = frame.gap_thresholds(0.25)
    assert g[0] == 3 << 30 and g[1] == 9 << 28 and (np.diff(g.astype(np.int64)) <= 0).all()
    assert frame.gap_thresholds(1e-30)[63] == 0xFFFFFFFF  # clamped
    p_fire, vals, thr = frame.outcome_thresholds([0.5, 0.25, 0.0, 0.25])
    assert p_fire == 0.5 and vals.tolist() == [1, 3] and thr.tolist() == [1 << 31, 0xFFFFFFFF]
    nk = frame.noise_key(KEY)
    assert nk != KEY and frame.site_key(nk, 0) == nk and frame.site_key(nk, 3) == (nk[0] ^ ((3 * 0x9E3779B9) & 0xFFFFFFFF), nk[1])


# ---- gauge outputs --------------------------------------------------------------------------------------------------------

def test_gauge_detector_is_sampled():
    c = CliffordCircuit("R 0\nH 0\nM 0\nDETECTOR rec[-1]")
    with pytest.raises(ValueError, match="not deterministic"):
        c.compile_detector_sampler(seed=1)
    s = c.compile_detector_sampler(seed=1, method="frame")
    assert s.num_detectors == 1 and s.num_observables == 0
    t = c.compile_detector_sampler(seed=1, method="frame")
    key = t._next_key()
    rows = frame.frame_rows_host(s._form, 300, 0, key)
    want = word_bits(affine.random_words(key, 1, 0, 5).T, 300)
    assert np.array_equal(rows, want) and 100 < rows.sum() < 200


# ---- how a request is cut -------------------------------------------------------------------------------------------------

NOISY = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.01, before_measure_flip_probability=0.01)
FEEDBACK = "R 0 1\nH 0\nX_ERROR(0.2) 1\nM 0\nCX rec[-1] 1\nHERALDED_ERASE(0.3) 1\nM 1\nDETECTOR rec[-1] rec[-3]\nOBSERVABLE_INCLUDE(0) rec[-2]"


def test_method_switch_and_argument_checks():
    from tsim_amd.sampler import CompiledDetectorSampler, CompiledMeasurementSampler

    c = CliffordCircuit(FEEDBACK)
    m, d = c.compile_sampler(seed=1, method="frame"), c.compile_detector_sampler(seed=1, method="frame", noise="device")
    assert isinstance(m, frame.CompiledFrameMeasurementSampler) and isinstance(m, CompiledMeasurementSampler)
    assert isinstance(d, frame.CompiledFrameDetectorSampler) and isinstance(d, CompiledDetectorSampler)
    assert m._channel_sampler is None and d._channel_sampler is None and not m._program.components
    assert (d.num_detectors, d.num_observables) == (1, 1) and "frame operations" in repr(d)
    with pytest.raises(ValueError, match="method"):
        c.compile_detector_sampler(method="affine")
    with pytest.raises(ValueError, match="noise"):
        c.compile_sampler(method="frame", noise="nowhere")
    assert type(c.compile_detector_sampler(seed=1)) is CompiledDetectorSampler
    for text in ("T 0\nM 0", "CX sweep[0] 1\nM 1"):
        with pytest.raises(NotImplementedError):
            CliffordCircuit(text).compile_frame()


def test_nothing_dense_is_built(monkeypatch):
    """``method="frame"`` calls none of the dense routes and builds no ``ChannelSampler``."""
    import tsim_amd.channels
    import tsim_amd.clifford as cl
    import tsim_amd.sampler

    def boom(*a, **k):
        raise AssertionError("a dense route was taken")

    for name in ("compile", "compile_measurements", "compile_affine_measurements", "analyze"):
        monkeypatch.setattr(cl.CliffordCircuit, name, boom)
    monkeypatch.setattr(cl, "_record_basis", boom)
    monkeypatch.setattr(cl, "find_basis", boom)
    monkeypatch.setattr(tsim_amd.channels.ChannelSampler, "__init__", boom)
    monkeypatch.setattr(tsim_amd.sampler, "ChannelSampler", boom)
    c = cl.CliffordCircuit(NOISY)
    m, d = c.compile_sampler(seed=2, method="frame"), c.compile_detector_sampler(seed=2, method="frame")
    assert frame.frame_rows_host(m._form, 64, 0, KEY).shape == (64, m._form.n_records)
    assert d.num_detectors == 24 and d.num_observables == 1
    assert not d._compute_reference_sample().any() and d._key == m._key  # (the reference costs no key)


@pytest.mark.parametrize("text", [NOISY, FEEDBACK])
def test_rows_do_not_depend_on_how_the_request_is_cut(text):
    c = CliffordCircuit(text)
    form = c.compile_frame()
    whole = frame.frame_rows_host(form, 1000, 0, KEY)
    assert whole.any() and not whole.all()
    for m in (1, 63, 64, 65, 640):
        assert np.array_equal(frame.frame_rows_host(form, m, 0, KEY), whole[:m]), m
    assert np.array_equal(frame.frame_rows_host(form, 1000 - 192, 192, KEY), whole[192:])
    assert not np.array_equal(frame.frame_rows_host(form, 1000, 0, (KEY[0], KEY[1] + 1)), whole)
    with pytest.raises(ValueError, match="multiple of 64"):
        frame.frame_rows_host(form, 10, 32, KEY)
    # the sampler: one key per request, whatever the batch size
    s, t = c.compile_sampler(seed=5, method="frame"), c.compile_sampler(seed=5, method="frame")
    a1, a2 = s.sample(640), s.sample(640)
    assert a1.dtype == np.bool_ and not np.array_equal(a1, a2)
    assert np.array_equal(t.sample(640, batch_size=64), a1) and np.array_equal(t.sample(200, batch_size=128), a2[:200])
    u = c.compile_sampler(seed=5, method="frame", noise="device")
    assert np.array_equal(u.sample(100, None, True), np.packbits(a1[:100], axis=1, bitorder="little"))  # noise= changes nothing
    assert s.sample(0).shape == (0, form.n_out) and s.sample(0, bit_packed=True).shape == (0, (form.n_out + 7) // 8)


def test_detector_sampler_keywords_on_the_host_statement():
    c = CliffordCircuit(NOISY)
    mk = lambda: c.compile_detector_sampler(seed=8, method="frame")  # noqa: E731
    s = mk()
    rows = frame.frame_rows_host(s._form, 500, 0, mk()._next_key()).view(np.bool_)
    nd = s.num_detectors
    assert np.array_equal(mk().sample(500), rows[:, :nd])
    det, obs = mk().sample(500, separate_observables=True)
    assert np.array_equal(det, rows[:, :nd]) and np.array_equal(obs, rows[:, nd:])
    assert np.array_equal(mk().sample(500, prepend_observables=True), np.concatenate([rows[:, nd:], rows[:, :nd]], axis=1))
    assert np.array_equal(mk().sample(500, append_observables=True, bit_packed=True), np.packbits(rows, axis=1, bitorder="little"))
    mask = np.zeros(nd, np.bool_)
    mask[:4] = True
    assert np.array_equal(mk().sample(500, postselection_mask=mask, use_detector_reference_sample=True), rows[:, :nd])
    # the records through the measurement-to-detection converter: the detector sampler's rows for the same seed
    meas = c.compile_sampler(seed=8, method="frame").sample(500)
    assert np.array_equal(c.compile_m2d_converter().csr()[2], s._compute_reference_sample().view(np.uint8))
    row_ptr, cols, ref = c.compile_m2d_converter().csr()
    conv = np.stack([(meas[:, cols[row_ptr[j]:row_ptr[j + 1]]].sum(axis=1) & 1) ^ ref[j] for j in range(len(ref))], axis=1)
    assert np.array_equal(conv.astype(np.bool_), rows)


# ---- the worked example ---------------------------------------------------------------------------------------------------

def test_worked_example():
    """``H 0 2; CX 0 1; M 0 1 2; CX 2 1; M 1 !0`` (the example of test_affine) with a flip on the third record."""
    c = CliffordCircuit("H 0 2\nCX 0 1\nM 0 1\nM(0.25) 2\nCX 2 1\nM 1 !0")
    form = c.compile_frame()
    assert (form.n_qubits, form.n_records, form.n_hidden, form.n_random, form.num_e) == (4, 5, 0, 2, 1)
    assert form.describe() == ["H 0 2", "CX 0>1", "MEASURE 0>0 1>1 2>2", "NOISE 0", "CX 2>1", "MEASURE 1>3 0>4"]
    assert form.batch_ptr.tolist() == [0, 2, 3, 6, 7, 8, 10]
    assert (form.site_chan.tolist(), form.site_e0.tolist(), form.site_table.tolist()) == ([0], [0], [0])
    assert form.targets.tolist() == [4 * 2 + frame.T_REC] and form.bit_ptr.tolist() == [0, 1] and form.site_bit.tolist() == [0, 1]
    assert form.out_vals.tolist() == [1] and form.out_thr.tolist() == [0xFFFFFFFF] and form.table_gap.tolist() == [0]
    assert form.gap_thr[0, :3].tolist() == [3 << 30, 9 << 28, 27 << 26]
    assert form.out_const.tolist() == [0, 0, 0, 0, 1]
    lists = [form.out_cols[form.out_ptr[i]:form.out_ptr[i + 1]].tolist() for i in range(5)]
    assert lists == [[0, 5], [1, 5], [2, 6], [3, 5, 6], [4, 5]]  # its own flip, then the symbols of test_affine's example
    rows = frame.frame_rows_host(form, 8, 0, (1, 2))
    assert rows.tolist() == WORKED_ROWS
    quiet = CliffordCircuit(WORKED).compile_frame()
    assert quiet.describe() == ["H 0 2", "CX 0>1", "MEASURE 0>0 1>1 2>2", "CX 2>1", "MEASURE 1>3 0>4"]
    flips = rows ^ frame.frame_rows_host(quiet, 8, 0, (1, 2))
    assert not flips[:, [0, 1, 3, 4]].any() and flips[:, 2].tolist() == [r[2] ^ q[2] for r, q in zip(WORKED_ROWS, frame.frame_rows_host(quiet, 8, 0, (1, 2)).tolist())]


WORKED_ROWS = [[1, 1, 1, 0, 0], [1, 1, 0, 0, 0], [0, 0, 1, 0, 1], [0, 0, 0, 0, 1], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [0, 0, 0, 0, 1],
               [0, 0, 0, 0, 1]]


# ---- scale ----------------------------------------------------------------------------------------------------------------

def test_form_of_the_d15_surface_code_is_linear_in_the_circuit():
    text = circuits.rotated_surface_code_memory(15, 15, after_clifford_depolarization=1e-3, before_measure_flip_probability=1e-3)
    c = CliffordCircuit(text)
    form = c.compile_frame("detectors")
    n_instr = len(c.instructions)
    n_targets = sum(len(i.targets) for i in c.instructions)
    assert form.n_records == 3585 and form.num_e == 60705 and form.n_qubits == 450
    assert form.num_detectors == 3360 and form.n_out == 3361
    for name, a in form.arrays().items():
        assert a.size <= 4 * (n_instr + n_targets) + 64 * 8, (name, a.size, n_instr, n_targets)
    assert form.n_batches < 40 * 15 + 40 and len(form.gap_thr) <= 4 and len(form.table_gap) <= 4
    assert len(c.compile_frame("measurements").out_const) == 3585


@pytest.mark.parametrize("text", [NOISY, FEEDBACK, "X_ERROR(0.1) 0\nM 0 1\nDETECTOR rec[-1]\nDETECTOR rec[-2]\nDETECTOR rec[-1] rec[-2]"])
def test_compile_fills_the_same_error_transform(text):
    """``compile()`` fills the basis rows from their set bits; the array is the one the bit-by-bit loop gave."""
    from tsim_amd.clifford import find_basis

    c = CliffordCircuit(text)
    an = c.analyze()
    outputs = list(an.detectors) + [tuple(an.observables[k][:2]) for k in sorted(an.observables)]
    rows = [s for s, _ in outputs if s]
    basis_idx, _ = find_basis(rows)
    want = np.zeros((len(basis_idx) + any(not s for s, _ in outputs), an.num_e), dtype=np.uint8)
    for pos, bi in enumerate(basis_idx):
        for e in range(an.num_e):
            want[pos, e] = (rows[bi] >> e) & 1
    got = c.compile()[2]
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want) and want.any()


def test_create_refuses_too_many_qubits_without_a_device():
    lib = _lib.load()
    import dataclasses

    form = dataclasses.replace(CliffordCircuit("H 0\nM 0").compile_frame(), n_qubits=10241)
    with pytest.raises(_lib.HipBackendError, match="at most 10240 qubits"):
        frame.FrameHandle(form).info()
    h = C.c_void_p()
    assert lib.tsim_frame_create(0, None, C.byref(h)) == -22 and lib.tsim_frame_info(None, (C.c_int64 * 16)()) == -22
    bad = frame.FrameHandle(CliffordCircuit("H 0\nM 0").compile_frame())
    bad.form.op_a[0] = 7  # a qubit that is not there
    with pytest.raises(ValueError, match="operation 0"):
        bad.info()
