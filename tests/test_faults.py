"""The fault-driven detector sampler without a device: the form against independent code (the error bits and detector rows of
``frame.frame_rows_host``, ``analyze()``'s masks), the numpy statement ``faults.fault_rows_host`` against its own error bits,
the law of the error bits against ``noise_law``, the tables of the draw, independence from how a request is cut, the method
switch, the size of the d = 15 form and what ``tsim_faults_create`` refuses before any device call."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import noise_law
from test_frame import FEEDBACK, KEY, NOISY, random_circuit, word_bits

from tsim_amd import _lib, circuits, faults, frame
from tsim_amd.clifford import CliffordCircuit, _bits

K = faults.K_GAP


# ---- random circuits over the whole gate table, with deterministic detectors -------------------------------------------------

def with_deterministic_detectors(body: str, seed: int) -> str:
    """``body`` (no detectors) plus detectors and observables over record sets whose random symbols cancel: the GF(2) null
    space of the records' symbol vectors, found by elimination."""
    rng = np.random.default_rng(seed)
    an = CliffordCircuit(body).analyze()
    n_rec = len(an.rec_syms)
    basis, quiet = {}, []  # pivot -> (reduced symbols, member records); record sets without symbols
    for i, y in enumerate(an.rec_syms):
        v, mem = int(y), 1 << i
        while v and (v & -v) in basis:
            bv, bm = basis[v & -v]
            v ^= bv
            mem ^= bm
        if v:
            basis[v & -v] = (v, mem)
        else:
            quiet.append(mem)
    assert quiet, "no deterministic record set"
    lines = []
    for n in range(10):
        mem = 0
        for i in rng.choice(len(quiet), size=min(len(quiet), int(rng.integers(1, 4))), replace=False):
            mem ^= quiet[int(i)]
        name = "DETECTOR" if n % 3 else f"OBSERVABLE_INCLUDE({int(rng.integers(3))})"
        lines.append(f"{name} " + " ".join(f"rec[-{n_rec - r}]" for r in _bits(mem)))
    return body + "\n" + "\n".join(lines)


def lists_of(form) -> list:
    return [form.cols[form.col_ptr[e]:form.col_ptr[e + 1]].tolist() for e in range(form.num_e)]


def rows_from_e(form, e_bits: np.ndarray) -> np.ndarray:
    """``out_const`` XOR the column lists of the error bits that are set (``e_bits``: ``uint8[B, num_e]``)."""
    rows = np.tile(form.out_const, (len(e_bits), 1))
    for e, cols in enumerate(lists_of(form)):
        for j in cols:
            rows[:, j] ^= e_bits[:, e]
    return rows


SIZES = [(1, 30), (2, 40), (5, 60), (70, 60)]


@pytest.mark.parametrize("n_qubits,n_ops", SIZES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_form_against_the_frame_statement_and_the_masks(n_qubits, n_ops, seed):
    text = with_deterministic_detectors(random_circuit(n_qubits, n_ops, 1000 * n_qubits + seed, detectors=False), seed)
    c = CliffordCircuit(text)
    an, form, fform = c.analyze(), c.compile_faults(), c.compile_frame("detectors")
    keys = sorted(an.observables)
    outputs = list(an.detectors) + [tuple(an.observables[k][:2]) for k in keys]
    assert form.n_out == fform.n_out == len(outputs) and form.num_detectors == len(an.detectors) and form.num_e == an.num_e
    assert np.array_equal(form.out_const, [v & 1 for _, v in outputs])
    # the column lists are the transpose of analyze()'s masks
    lists = lists_of(form)
    assert all(l == sorted(set(l)) for l in lists)
    for j, (s, _) in enumerate(outputs):
        assert set(_bits(int(s))) == {e for e, l in enumerate(lists) if j in l}, (j, text)
    # the sites: the channels that can fire, error bits numbered as analyze() numbers them, classes by first appearance
    first_bit = np.concatenate([[0], np.cumsum([int(np.log2(len(p))) for p in an.channel_probs])]).astype(np.int64)
    live = [ch for ch, p in enumerate(an.channel_probs) if 1.0 - float(p[0]) > 0.0]
    assert sorted(form.site_chan.tolist()) == live and np.array_equal(form.site_e0, first_bit[form.site_chan])
    firsts = []
    for cl in range(form.n_classes):
        chans = form.site_chan[form.class_ptr[cl]:form.class_ptr[cl + 1]]
        assert len(chans) and (np.diff(chans) > 0).all()
        assert all(np.array_equal(an.channel_probs[ch], an.channel_probs[chans[0]]) for ch in chans)
        assert 1 << int(form.table_bits[cl]) == len(an.channel_probs[chans[0]])
        firsts.append(int(chans[0]))
    assert firsts == sorted(firsts) and len({an.channel_probs[ch].tobytes() for ch in firsts}) == form.n_classes
    # the frame statement's error bits through the lists give the frame statement's detector rows, bit for bit
    B, first_shot = 200, 64 * (seed - 1)
    rows, e = frame.frame_rows_host(fform, B, first_shot, KEY, return_e=True)
    e_bits = word_bits(e, B) if an.num_e else np.zeros((B, 0), np.uint8)
    assert np.array_equal(rows_from_e(form, e_bits), rows), text


@pytest.mark.parametrize("text", [NOISY, FEEDBACK])
def test_host_statement_is_its_error_bits_through_the_lists(text):
    form = CliffordCircuit(text).compile_faults()
    B = 300
    rows, e = faults.fault_rows_host(form, 128, B, KEY, return_e=True)
    assert rows.dtype == np.uint8 and rows.shape == (B, form.n_out) and e.shape == (form.num_e, 5) and e.any()
    assert np.array_equal(rows, rows_from_e(form, word_bits(e, B)))
    assert np.array_equal(faults.fault_rows_host(form, 128, B, KEY), rows)
    assert not (e[:, -1] >> np.uint64(B - 256)).any()  # no bit beyond the last shot


# ---- the law of the error bits --------------------------------------------------------------------------------------------

N_LONG = 2 * K + 100


def law_model() -> CliffordCircuit:
    """A class of one site (``X_ERROR(0.3)``), a class of 2 K + 100 sites at 1e-3 (the walk restarts twice or more), three
    sites at 0.5, an always-firing site, 4-bit 15-outcome sites at two rates and a ``CORRELATED_ERROR`` chain.  Nothing is
    measured: the error bits are read from the statement."""
    q = N_LONG
    return CliffordCircuit("\n".join([
        "X_ERROR(0.001) " + " ".join(map(str, range(N_LONG))), "X_ERROR(0.3) 0", f"Z_ERROR(0.5) {q} {q + 1} {q + 2}", "Y_ERROR(1) 1",
        f"DEPOLARIZE2(0.3) {q} {q + 1} {q + 2} {q + 3}", f"DEPOLARIZE2(0.001) {q + 4} {q + 5}",
        "E(0.2) X0", "ELSE_CORRELATED_ERROR(0.4) Z1", "ELSE_CORRELATED_ERROR(0.3) Y2"]))


def packed_rows(e_words: np.ndarray, B: int) -> np.ndarray:
    """``frame.e_rows`` 64 error bits at a time (thousands of error bits over 2^18 shots)."""
    num_e, nw = e_words.shape
    out = np.zeros((B, (num_e + 63) // 64), np.uint64)
    for w in range(out.shape[1]):
        part = np.ascontiguousarray(e_words[64 * w:64 * w + 64])
        bits = np.zeros((B, 64), np.uint8)
        bits[:, :len(part)] = np.unpackbits(part.view(np.uint8).reshape(len(part), nw * 8), axis=1, bitorder="little")[:, :B].T
        out[:, w] = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)[:, 0]
    return out


@pytest.fixture(scope="module")
def law_rows():
    form = law_model().compile_faults()
    B = 1 << 18
    rows, e = faults.fault_rows_host(form, 64 * 5, B, (7, 11), return_e=True)
    assert rows.shape == (B, 0)
    packed = packed_rows(e, B)
    assert np.array_equal(packed[:4096], frame.e_rows(e[:, :64], 4096))
    return form, B, packed


def test_law_of_the_error_bits(law_rows):
    """2^18 shots under a fixed key.  The statement is integer arithmetic on tables fixed by float64 arithmetic, so the rows are
    the same wherever this runs; for this key and this many shots every parity below stays inside noise_law's own family bound
    (alpha = 1e-6 over all masks) of the exact law (2^19 shots do too; 2^18 keep the test at a few seconds)."""
    form, B, packed = law_rows
    probs, num_e = form.channel_probs, form.num_e
    assert num_e == N_LONG + 1 + 3 + 1 + 8 + 4 + 3 and packed.shape == (B, (num_e + 63) // 64)
    assert np.diff(form.class_ptr).tolist() == [N_LONG, 1, 3, 1, 2, 1, 1] and 5 <= len(form.gap_thr) <= 7
    groups, at = [], 0
    for p in probs:
        k = int(np.log2(len(p)))
        groups.append(list(range(at, at + k)))
        at += k
    masks = noise_law.standard_masks(num_e, groups, np.random.default_rng(3))
    T = np.eye(num_e, dtype=np.uint8)
    noise_law.check_biases(noise_law.empirical_bias(packed, masks), noise_law.parity_bias(probs, T, masks), B, masks)
    # neighbours across the restart seams, and the always-firing bit
    seams = [(K - 1, K), (K, K + 1), (2 * K - 1, 2 * K), (0, N_LONG - 1)]
    noise_law.check_biases(noise_law.empirical_bias(packed, seams), noise_law.parity_bias(probs, T, seams), B, seams)
    always = N_LONG + 1 + 3
    assert noise_law.bit_counts(packed)[always] == B


@pytest.mark.parametrize("M", [64, 192])
def test_fire_rate_in_every_position_class(law_rows, M):
    """One-bit sites of one rate fire at that rate in every class ``shot mod M``, wherever they stand in their class."""
    form, B, packed = law_rows
    noise_law.check_position_classes(packed, list(range(N_LONG)), 1e-3, M)
    for lo, hi in ((0, 64), (K - 32, K + 32), (2 * K - 32, 2 * K + 32), (N_LONG - 64, N_LONG)):  # around the seams of the walk
        noise_law.check_position_classes(packed, list(range(lo, hi)), 1e-3, M)
    noise_law.check_position_classes(packed, [N_LONG], 0.3, M)
    noise_law.check_position_classes(packed, [N_LONG + 1, N_LONG + 2, N_LONG + 3], 0.5, M)
    noise_law.check_position_classes(packed, [N_LONG + 4], 1.0, M)


# ---- the tables of the draw -----------------------------------------------------------------------------------------------

def test_tables_of_the_draw():
    g = faults.gap_thresholds(1.0)
    assert g.dtype == np.uint32 and g.shape == (K,) and not g.any()  # an always-firing site skips nothing
    g = faults.gap_thresholds(0.25)
    assert g[0] == 3 << 30 and g[1] == 9 << 28 and g[2] == 27 << 26 and (np.diff(g.astype(np.int64)) <= 0).all()
    g = faults.gap_thresholds(0.5)
    assert g[:32].tolist() == [1 << (32 - k) for k in range(1, 33)] and not g[32:].any()
    assert faults.gap_thresholds(1e-30)[K - 1] == 0xFFFFFFFF  # clamped
    g = faults.gap_thresholds(1e-3)
    assert abs(int(g[K - 1]) / 2**32 - 0.999**K) < 1e-9 and (np.diff(g.astype(np.int64)) < 0).all()
    # skip = #{k : x0 < gap_thr[k]}: exactly gap_thr[k] of the 2^32 values of x0 give skip >= k ...
    for k in (1, 2, 63, 64, 65, 500, K - 1, K):
        t = int(g[k - 1])
        assert faults.skip_of(g, [t - 1, t]).tolist() == [k, k - 1]
    assert faults.skip_of(g, [0, 0xFFFFFFFF]).tolist() == [K, 0]
    # ... so a walk that restarts at skip == K crosses K + k quiet sites for gap_thr[K] * gap_thr[k] of the 2^64 pairs of
    # draws: P(skip >= K + k) = P(skip >= K) P(skip >= k) on the integers, as the geometric law has it on the reals
    x0 = np.random.default_rng(5).integers(0, 1 << 32, size=(2, 200000), dtype=np.uint64).astype(np.uint32)
    first, second = faults.skip_of(g, x0[0]), faults.skip_of(g, x0[1])
    total = np.where(first == K, K + second, first)
    for k in (1, 100, 700):
        assert np.array_equal(total >= K + k, (x0[0] < g[K - 1]) & (x0[1] < g[k - 1]))
    p_fire, vals, thr = frame.outcome_thresholds([0.5, 0.25, 0.0, 0.25])
    assert p_fire == 0.5 and vals.tolist() == [1, 3] and thr.tolist() == [1 << 31, 0xFFFFFFFF]
    form = CliffordCircuit("X_ERROR(0.25) 0\nDEPOLARIZE1(0.75) 1\nX_ERROR(0.25) 2\nM(0.25) 0").compile_faults()
    assert form.class_ptr.tolist() == [0, 3, 4] and form.site_chan.tolist() == [0, 2, 3, 1] and form.site_e0.tolist() == [0, 3, 4, 1]
    assert form.table_bits.tolist() == [1, 2] and form.table_ptr.tolist() == [0, 1, 4] and form.out_vals.tolist() == [1, 1, 2, 3]
    assert form.out_thr.tolist() == [0xFFFFFFFF, 0x55555556, 0xAAAAAAAB, 0xFFFFFFFF] and form.table_gap.tolist() == [0, 1]
    assert np.array_equal(form.gap_thr, [faults.gap_thresholds(0.25), faults.gap_thresholds(0.75)])
    nk = faults.noise_key(KEY)
    assert nk != KEY and nk != frame.noise_key(KEY) and faults.class_key(nk, 0) == nk
    assert faults.class_key(nk, 3) == (nk[0] ^ ((3 * 0x9E3779B9) & 0xFFFFFFFF), nk[1])


def test_the_walk_by_hand():
    """One class of five one-bit sites at p = 0.25, each flipping its own output: the walk written out draw by draw."""
    from tsim_amd.affine import threefry2x32_np

    form = CliffordCircuit("X_ERROR(0.25) 0 1 2 3 4\nM 0 1 2 3 4\n" + "\n".join(f"DETECTOR rec[-{k}]" for k in range(5, 0, -1))).compile_faults()
    assert lists_of(form) == [[0], [1], [2], [3], [4]]
    rows = faults.fault_rows_host(form, 2**38 - 64, 64, KEY)
    k0, k1 = faults.class_key(faults.noise_key(KEY), 0)
    gap = form.gap_thr[0]
    for n in (0, 17, 63):
        g, want, pos, j = 2**38 - 64 + n, [0] * 5, -1, 0
        while True:
            x0, _ = threefry2x32_np(k0, k1, np.uint32(g & 0xFFFFFFFF), np.uint32((g >> 32) | (j << 6)))
            skip = sum(int(x0) < int(t) for t in gap)
            j += 1
            if skip == K:
                pos += K
                continue
            pos += skip + 1
            if pos >= 5:
                break
            want[pos] ^= 1
        assert rows[n].tolist() == want


# ---- how a request is cut -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("text", [NOISY, FEEDBACK])
def test_rows_do_not_depend_on_how_the_request_is_cut(text):
    c = CliffordCircuit(text)
    form = c.compile_faults()
    whole = faults.fault_rows_host(form, 0, 1000, KEY)
    assert whole.any() and not whole.all()
    for m in (1, 63, 64, 65, 640):
        assert np.array_equal(faults.fault_rows_host(form, 0, m, KEY), whole[:m]), m
    assert np.array_equal(faults.fault_rows_host(form, 192, 1000 - 192, KEY), whole[192:])
    assert not np.array_equal(faults.fault_rows_host(form, 0, 1000, (KEY[0], KEY[1] + 1)), whole)
    with pytest.raises(ValueError, match="multiple of 64"):
        faults.fault_rows_host(form, 32, 10, KEY)
    with pytest.raises(ValueError, match="2\\^38"):
        faults.fault_rows_host(form, 2**38 - 64, 65, KEY)
    # the sampler: one key per request, whatever the batch size
    s, t = c.compile_detector_sampler(seed=5, method="faults"), c.compile_detector_sampler(seed=5, method="faults")
    a1, a2 = s.sample(640, append_observables=True), s.sample(640, append_observables=True)
    assert a1.dtype == np.bool_ and not np.array_equal(a1, a2)
    assert np.array_equal(a1, faults.fault_rows_host(form, 0, 640, c.compile_detector_sampler(seed=5, method="faults")._next_key()).view(np.bool_))
    assert np.array_equal(t.sample(640, batch_size=64, append_observables=True), a1)
    assert np.array_equal(t.sample(200, batch_size=128, append_observables=True), a2[:200])
    u = c.compile_detector_sampler(seed=5, method="faults", noise="device")  # noise= changes nothing
    assert np.array_equal(u.sample(100, append_observables=True, bit_packed=True), np.packbits(a1[:100], axis=1, bitorder="little"))
    assert s.sample(0).shape == (0, form.num_detectors)


def test_detector_sampler_keywords_on_the_host_statement():
    c = CliffordCircuit(NOISY)
    mk = lambda: c.compile_detector_sampler(seed=8, method="faults")  # noqa: E731
    s = mk()
    rows = faults.fault_rows_host(s._form, 0, 500, mk()._next_key()).view(np.bool_)
    nd = s.num_detectors
    assert (nd, s.num_observables) == (24, 1) and rows[:, :nd].any()
    assert np.array_equal(mk().sample(500), rows[:, :nd])
    det, obs = mk().sample(500, separate_observables=True)
    assert np.array_equal(det, rows[:, :nd]) and np.array_equal(obs, rows[:, nd:])
    assert np.array_equal(mk().sample(500, prepend_observables=True), np.concatenate([rows[:, nd:], rows[:, :nd]], axis=1))
    assert np.array_equal(mk().sample(500, append_observables=True, bit_packed=True), np.packbits(rows, axis=1, bitorder="little"))
    mask = np.zeros(nd, np.bool_)
    mask[:4] = True
    assert np.array_equal(mk().sample(500, postselection_mask=mask, use_detector_reference_sample=True), rows[:, :nd])
    # two samples of one law: the detection fraction of the default method
    want = c.compile_detector_sampler(seed=8).sample(20000).mean()
    got = mk().sample(20000).mean()
    assert abs(got - want) < 6 * np.sqrt(want / (20000 * nd))  # (events of one shot are positively correlated: a loose bound)


# ---- the method switch ----------------------------------------------------------------------------------------------------

def test_method_switch_and_argument_checks():
    from tsim_amd.sampler import CompiledDetectorSampler

    c = CliffordCircuit(FEEDBACK)
    d = c.compile_detector_sampler(seed=1, method="faults", noise="device")
    assert isinstance(d, faults.CompiledFaultDetectorSampler) and isinstance(d, CompiledDetectorSampler)
    assert d._channel_sampler is None and not d._program.components and (d.num_detectors, d.num_observables) == (1, 1)
    assert "noise sites" in repr(d) and c.compile_faults() is d._form
    key = d._key
    assert np.array_equal(d._compute_reference_sample(), d._form.out_const.astype(np.bool_)) and d._key == key  # costs no key
    assert type(c.compile_detector_sampler(seed=1)) is CompiledDetectorSampler
    assert type(c.compile_detector_sampler(seed=1, method="frame")) is frame.CompiledFrameDetectorSampler
    for call, kw in ((c.compile_sampler, dict(method="faults")), (c.compile_sampler, dict(method="bogus")),
                     (c.compile_detector_sampler, dict(method="affine")), (c.compile_detector_sampler, dict(method="bogus"))):
        with pytest.raises(ValueError, match="method"):
            call(**kw)
    with pytest.raises(ValueError, match="noise"):
        c.compile_detector_sampler(method="faults", noise="nowhere")
    gauge = CliffordCircuit("R 0\nH 0\nM 0\nDETECTOR rec[-1]")
    for kw in (dict(), dict(method="faults")):  # refused exactly as the default method refuses it
        with pytest.raises(ValueError, match="DETECTOR rec\\[-1\\] \\(detector 0\\) is not deterministic"):
            gauge.compile_detector_sampler(seed=1, **kw)
    with pytest.raises(ValueError, match="OBSERVABLE 0 is not deterministic"):
        CliffordCircuit("H 0\nM 0\nOBSERVABLE_INCLUDE(0) rec[-1]").compile_detector_sampler(method="faults")
    for text in ("T 0\nM 0", "CX sweep[0] 1\nM 1"):
        with pytest.raises(NotImplementedError):
            CliffordCircuit(text).compile_detector_sampler(method="faults")


# ---- scale ----------------------------------------------------------------------------------------------------------------

def test_form_of_the_d15_surface_code_needs_nothing_dense(monkeypatch):
    """``method="faults"`` is ``analyze()`` plus a transposition: no basis, no ``error_transform``, no ``ChannelSampler``.  The
    d = 15, 15-round form: 60 705 error bits, 19 545 sites in 3 classes, 101 696 flips (at most 2 per error bit), 3 gap rows;
    its arrays take 0.83 MB where ``error_transform`` takes 207 MB."""
    import tsim_amd.channels
    import tsim_amd.clifford as cl
    import tsim_amd.sampler

    def boom(*a, **k):
        raise AssertionError("a dense route was taken")

    for name in ("compile", "compile_measurements", "compile_affine_measurements", "compile_frame"):
        monkeypatch.setattr(cl.CliffordCircuit, name, boom)
    monkeypatch.setattr(cl, "_record_basis", boom)
    monkeypatch.setattr(cl, "find_basis", boom)
    monkeypatch.setattr(tsim_amd.channels.ChannelSampler, "__init__", boom)
    monkeypatch.setattr(tsim_amd.sampler, "ChannelSampler", boom)
    text = circuits.rotated_surface_code_memory(15, 15, after_clifford_depolarization=1e-3, before_measure_flip_probability=1e-3)
    s = cl.CliffordCircuit(text).compile_detector_sampler(seed=2, method="faults")
    form = s._form
    assert (s.num_detectors, s.num_observables, form.num_e, form.n_sites, form.n_classes) == (3360, 1, 60705, 19545, 3)
    assert np.diff(form.class_ptr).tolist() == [3360, 12600, 3585] and form.table_bits.tolist() == [2, 4, 1]
    assert len(form.cols) == 101696 and np.diff(form.col_ptr).max() == 2 and form.gap_thr.shape == (2, K)
    assert sum(a.nbytes for a in form.arrays().values()) == 817729
    assert not s._compute_reference_sample().any()
    rows = faults.fault_rows_host(form, 0, 256, KEY)
    assert rows.shape == (256, 3361) and 0.005 < rows.mean() < 0.03


# ---- what create refuses, without a device ---------------------------------------------------------------------------------

def test_create_refuses_a_bad_form_without_a_device(monkeypatch):
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.tsim_faults_create(0, None, C.byref(h)) == -22 and lib.tsim_faults_info(None, (C.c_int64 * 16)()) == -22
    good = CliffordCircuit(NOISY).compile_faults()

    def refused(match, exc=ValueError, **changes):
        form = dataclasses.replace(good, **{k: v.copy() for k, v in good.arrays().items()})
        for name, (index, value) in changes.items():
            getattr(form, name)[index] = value
        with pytest.raises(exc, match=match):
            faults.FaultHandle(form).info()

    refused("cols\\[5\\] = 25", cols=(5, good.n_out))
    refused("cols\\[0\\] = -1", cols=(0, -1))
    refused("site 2 of class 1: error bits", site_e0=(int(good.class_ptr[1]) + 2, good.num_e))
    multi = int(np.argmax(np.diff(good.table_ptr)))  # a table of several outcomes
    refused(f"table {multi}: thresholds decrease", out_thr=(int(good.table_ptr[multi]), 0xFFFFFFFF))
    refused("gap row 0 increases", gap_thr=((0, 7), 0xFFFFFFFF))
    refused("col_ptr decreases", col_ptr=(3, int(good.col_ptr[-1])))
    refused("must run from 0", class_ptr=(-1, good.n_sites - 1))
    refused("gap row 9 of", table_gap=(0, 9))
    refused("has a bit beyond", out_vals=(int(good.table_ptr[multi]), 1 << int(good.table_bits[multi])))
    refused("error bits per site", table_bits=(0, 33))
    # a class too large for the draw index: refused by the form's builder and by create (which reads no site of it)
    d = _lib.FaultsDesc(**{n: 0 for n in _lib.FaultsDesc.SIZES}, **{n: None for n in _lib.FaultsDesc.ARRAYS})
    big = np.array([0, faults.MAX_CLASS_SITES + 1], np.int32)
    zero = np.zeros(2, np.int32)
    d.n_sites, d.n_classes, d.gap_k = int(big[1]), 1, K
    d.class_ptr, d.table_ptr, d.col_ptr = big.ctypes.data, zero.ctypes.data, zero.ctypes.data
    d.site_e0 = d.table_bits = d.table_gap = d.out_vals = d.out_thr = d.gap_thr = zero.ctypes.data
    assert lib.tsim_faults_create(0, C.byref(d), C.byref(h)) == -95 and b"the draw index has 26 bits" in lib.tsim_last_error()
    d.gap_k = 64
    assert lib.tsim_faults_create(0, C.byref(d), C.byref(h)) == -22 and b"gap_k" in lib.tsim_last_error()
    monkeypatch.setattr(faults, "MAX_CLASS_SITES", 3)
    with pytest.raises(NotImplementedError, match="class 0 has 4 sites"):
        CliffordCircuit("X_ERROR(0.1) 0 1 2 3").compile_faults()
