"""Fixed-weight fault sampling on the device (tsim_faults_set_split / tsim_faults_sample_weight_device,
csrc/tsim_faults_weight.hip.h): the kernel's bytes against the numpy statement ``fixed_weight.fixed_weight_rows_host`` - always
the oracle, bit for bit - the LDS rule, the sampler's ``count()`` with a decoder, and the stratified logical error rate against
direct sampling."""

import math

import numpy as np
import pytest

from test_frame import KEY
from test_gpu_faults import DEP2, Case, hp, pack, synth_form  # noqa: F401 - hp is a fixture

from tsim_amd import _lib, circuits, faults
from tsim_amd import fixed_weight as fw
from tsim_amd.channels import error_probs, pauli_channel_1_probs
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.counts import tally_rows
from tsim_amd.decode import UnionFindDecoder

pytestmark = pytest.mark.gpu

MAX_SHOT = 1 << 38
LDS, TAB_LDS, LIST = 160 * 1024, 32 * 1024, 32 * 256
# classes of 1, 2, 70 and 2 * 1024 + 100 sites
MIXED = [(error_probs(0.3), 1), (DEP2(0.5), 2), (pauli_channel_1_probs(0.1, 0.2, 0.05), 70), (error_probs(1e-3), 2 * 1024 + 100)]
WEIGHTS = (0, 1, 2, 5, 32)


class WeightCase(Case):
    """``Case`` of the fault sampler's tests over a ``FixedWeightHandle``: one split table, the weight set per launch."""

    def __init__(self, hp, form, kmax=None):
        self.hp, self.form, self.n_out = hp, form, form.n_out
        self.h = fw.FixedWeightHandle(form, min(fw.MAX_FAULT_WEIGHT, form.n_sites) if kmax is None else kmax)

    def want(self, B, first_shot, key=KEY):
        return fw.fixed_weight_rows_host(self.form, self.h.weight, first_shot, B, key)

    def at(self, k):
        self.h.weight = k
        return self


def rule(form, kmax):
    """The LDS rule of k_faults_weight as include/tsim_hip.h and csrc/tsim_faults.hip state it."""
    tab = 4 * (2 * len(form.out_vals) + form.n_classes * (kmax + 1) ** 2)
    in_lds = tab <= TAB_LDS
    tab = -(-tab // 16) * 16 if in_lds else 0
    words = max(1, (form.n_out + 31) // 32)
    S, waves = words | 1, 1
    if 256 * S + LIST <= LDS - tab:
        waves = min(8, (LDS - tab) // (256 * S + LIST))
    else:
        S = (LDS - tab - LIST) // 256
        S -= 1 - (S & 1)
    win = min(32 * S, 32 * words)
    return dict(kmax=kmax, waves=waves, lds_bytes=tab + waves * (256 * S + LIST), tables_in_lds=int(in_lds), row_words=S, window=win,
                n_windows=-(-form.n_out // win), split_bytes=4 * form.n_classes * (kmax + 1) ** 2)


@pytest.mark.parametrize("n_out", [1, 31, 32, 33, 64, 65])
def test_column_counts_and_weights(hp, n_out):
    """k = 0, 1, 2, 5, 32 at B = 1, 63, 65, 200, packed and a byte per bit, all outputs and a sub-range inside bytes, row
    strides that allow dword stores and that do not."""
    case = WeightCase(hp, synth_form(n_out, MIXED, seed=n_out))
    info = case.h.weight_info()
    assert info == rule(case.form, 32) and info["waves"] == 8 and info["tables_in_lds"] == 1 and info["n_windows"] == 1
    assert np.diff(case.form.class_ptr).tolist() == [1, 2, 70, 2148]
    for k in WEIGHTS:
        whole = case.at(k).sweep(first_shots=(64 * 7,))
        assert (whole == whole[0]).all() if k == 0 else (whole != whole[0]).any() or n_out == 1
    case.close()


def test_every_site_of_an_eight_site_form(hp):
    """k = all sites: classes of 1 and 2 sites are taken whole, the rejection loop hunts the last free position."""
    form = synth_form(40, [(error_probs(0.3), 1), (DEP2(0.1), 2), (error_probs(0.01), 5)], seed=8)
    case = WeightCase(hp, form)
    assert form.n_sites == 8 and case.h.kmax == 8
    for k in (8, 7, 3):
        case.at(k).sweep(Bs=(65, 200), first_shots=(0,))
    with pytest.raises(ValueError, match="serves 0 .. 8"):
        case.at(9).launch(64, 0, True, 0, 40)
    case.close()


def test_split_table_in_global_memory(hp):
    """Eight classes at kmax = 32: 34 KiB of split rows, more than the tables' share of LDS."""
    form = synth_form(40, [(error_probs(p), 9) for p in (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)] + [(DEP2(0.4), 5)], seed=4)
    case = WeightCase(hp, form)
    info = case.h.weight_info()
    assert info == rule(form, 32) and info["tables_in_lds"] == 0 and info["lds_bytes"] == 8 * (256 * info["row_words"] + LIST)
    for k in (1, 5, 32):
        case.at(k).sweep(Bs=(65, 200), first_shots=(64,))
    small = WeightCase(hp, form, kmax=5)  # the same form with a table that fits
    assert small.h.weight_info()["tables_in_lds"] == 1
    small.at(5).sweep(Bs=(200,), first_shots=(64,))
    small.close()
    case.close()


def test_a_request_cut_into_launches_and_the_last_shots(hp):
    case = WeightCase(hp, synth_form(45, MIXED, seed=2)).at(5)
    n_out = case.n_out
    _, one = case.launch(200, 0, True, 0, n_out, slack=0)
    _, a = case.launch(128, 0, True, 0, n_out, slack=0)
    _, b = case.launch(64, 128, True, 0, n_out, slack=0)
    _, c = case.launch(8, 192, True, 0, n_out, slack=0)
    assert np.array_equal(np.concatenate([a, b, c]), one) and np.array_equal(one, pack(case.want(200, 0)))
    _, other = case.launch(200, 0, True, 0, n_out, slack=0, key=(KEY[0], KEY[1] + 1))
    assert not np.array_equal(other, one)
    for first_shot in (2**32 - 64, MAX_SHOT - 256):  # the shot index crosses 2^32; the last shots there are
        _, got = case.launch(200, first_shot, False, 0, n_out, slack=0)
        assert np.array_equal(got, case.want(200, first_shot))
    case.close()


def test_two_column_windows(hp):
    """21 000 outputs are more than one wave's LDS holds next to its list: two windows, each redrawing the stream."""
    form = synth_form(21000, [(DEP2(0.2), 250), (error_probs(1e-3), 150), (error_probs(0.5), 40)], seed=21000, fan=4)
    case = WeightCase(hp, form, kmax=5).at(5)
    info = case.h.weight_info()
    assert info == rule(form, 5) and info["n_windows"] == 2 and info["waves"] == 1 and info["window"] == 19360
    whole = case.want(70, 64)
    case.check(70, 64, whole, 0)
    case.check(70, 64, whole, 1)
    used, got = case.launch(70, 64, True, 19000, 1999, slack=3)  # a sub-range that fits one window, across the full request's seam
    assert np.array_equal(got[:, :used], pack(whole[:, 19000:20999])) and (got[:, used:] == 0xA5).all()
    case.close()


def test_argument_errors_come_before_any_launch(hp):
    form = synth_form(5, MIXED, seed=1)
    good = fw.FixedWeightHandle(form, 4)
    d = hp.malloc(4096)
    ok = dict(key=KEY, first_shot=0, out_row_bytes=1, out_packed=True, stream=hp.stream_ptr())
    good.sample_device(64, d.ptr, **ok)
    hp.synchronize()
    for change, match in ((dict(first_shot=32), "multiple of 64"), (dict(out_row_bytes=0), "out_row_bytes"),
                          (dict(col0=4, n_cols=2), "outputs"), (dict(first_shot=2**38), "2\\^38")):
        with pytest.raises(ValueError, match=match):
            good.sample_device(64, d.ptr, **{**ok, **change})
    with pytest.raises(ValueError, match="NULL"):
        good.sample_device(64, 0, **ok)
    for k in (5, -1):
        good.weight = k
        with pytest.raises(ValueError, match="serves 0 .. 4"):
            good.sample_device(64, d.ptr, **ok)
    # the table's own checks, and a handle without one
    lib, h = _lib.load(), good._handle()
    table = fw.split_thresholds(form, 4)
    for kmax, t, code, match in ((33, table, -22, b"kmax"), (4, None, -22, b"NULL")):
        assert lib.tsim_faults_set_split(h, kmax, t.ctypes.data if t is not None else None) == code and match in lib.tsim_last_error()
    bad = table.copy()
    bad[1, 3, :2] = [5, 0]
    assert lib.tsim_faults_set_split(h, 4, bad.ctypes.data) == -22 and b"decreases" in lib.tsim_last_error()
    lone = synth_form(5, [(error_probs(0.3), 4), (error_probs(0.2), 1)], seed=1)  # 4 sites, then a class of one
    alone = fw.FixedWeightHandle(lone, 4)
    t = fw.split_thresholds(lone, 4)
    assert t[0, 3, :2].tolist() == [0, 0]  # taking 0 or 1 of 3 would leave the one site more than it holds
    t[0, 3, :2] = [0, 7]
    assert lib.tsim_faults_set_split(alone._handle(), 4, t.ctypes.data) == -22 and b"would leave" in lib.tsim_last_error()
    alone.close()
    always = faults.FaultHandle(synth_form(5, [(error_probs(0.3), 4), (error_probs(1.0), 1)], seed=1))
    assert lib.tsim_faults_set_split(always._handle(), 0, np.full(2, 0xFFFFFFFF, np.uint32).ctypes.data) == -95
    assert b"probability 1" in lib.tsim_last_error()
    assert lib.tsim_faults_sample_weight_device(always._handle(), 0, 64, 0, 1, 2, d.ptr, 1, 1, 0, 5, None) == -1  # TSIM_ESTATE
    assert always.info()["n_sites"] == 5
    always.close()
    hp.synchronize()
    d.free()
    good.close()


# ---- the sampler, a decoder and the stratified rate -------------------------------------------------------------------------

D3 = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=1e-3, before_measure_flip_probability=1e-3))


def test_count_with_a_decoder_equals_the_statement_decoded_in_numpy(hip):
    uf = UnionFindDecoder.from_circuit(D3)
    nd = uf.num_detectors
    mk = lambda: D3.compile_detector_sampler(seed=21, method="faults", fault_weight=2)  # noqa: E731
    rows = fw.fixed_weight_rows_host(D3.compile_faults(), 2, 0, 4096, mk()._next_key()).view(np.bool_)
    got = mk().count(4096, decoder=uf)
    assert got == tally_rows(rows, num_detectors=nd, decoder=uf, histogram_columns=(nd,))
    wrong = int((uf.decode(rows[:, :nd]) != rows[:, nd:]).any(axis=1).sum())
    assert got.decoded_errors == wrong and got.decoder_misses == int(uf.missed(rows[:, :nd]).sum()) and 100 < wrong < 400
    assert np.array_equal(mk().sample(4096, append_observables=True, batch_size=1000), rows)


def test_stratified_rate_against_direct_sampling(hip):
    """d = 3, p = 1e-3: 2e5 shots per weight 0 .. 6 against 2e6 directly sampled shots, fixed seeds.  The two standard errors
    are about 1.2e-5 and 1.8e-5, the tail is below 1e-10."""
    uf = UnionFindDecoder.from_circuit(D3)
    got = fw.stratified_error_rate(D3, uf, 200_000, kmax=6, seed=3)
    direct = D3.compile_detector_sampler(seed=4, method="faults").count(2_000_000, decoder=uf)
    p = direct.decoded_errors / 2e6
    print(f"stratified {got.estimate:.4e} +- {got.std_error:.2e} (tail {got.tail:.2e}), direct {p:.4e} +- {math.sqrt(p * (1 - p) / 2e6):.2e}, "
          f"f_k {got.f.tolist()}")
    assert got.shots.tolist() == [200_000] * 7 and got.decoded_errors[0] == 0 and got.tail < 1e-10
    assert abs(got.f[1] - 4 / 15 / 129) < 5 * math.sqrt(2.07e-3 / 2e5)
    assert abs(got.estimate - p) <= 4 * math.sqrt(got.std_error**2 + p * (1 - p) / 2e6) + got.tail
