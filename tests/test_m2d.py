"""compile_m2d_converter without a device: record lists, reference bits, argument checks, the numpy restatement."""

import numpy as np
import pytest

from tsim_amd import circuits
from tsim_amd.clifford import CliffordCircuit


def restated(conv, m: np.ndarray) -> np.ndarray:
    """``(m @ A.T + ref) % 2`` over all outputs (detectors, then observables): the converter's law in numpy."""
    row_ptr, cols, ref = conv.csr()
    A = np.zeros((len(ref), conv.num_measurements), np.int64)
    for j in range(len(ref)):
        for k in cols[row_ptr[j]:row_ptr[j + 1]]:
            A[j, k] ^= 1
    return ((np.asarray(m, np.int64) @ A.T + ref) % 2).astype(np.bool_)


def records(conv) -> list:
    row_ptr, cols, _ = conv.csr()
    return [cols[row_ptr[j]:row_ptr[j + 1]].tolist() for j in range(len(row_ptr) - 1)]


def test_record_offsets_and_order():
    c = CliffordCircuit("M 0 1 2\nDETECTOR rec[-1] rec[-3]\nM 1\nDETECTOR rec[-1] rec[-3]\nOBSERVABLE_INCLUDE(0) rec[-2]")
    conv = c.compile_m2d_converter()
    assert (conv.num_measurements, conv.num_detectors, conv.num_observables) == (4, 2, 1)
    assert records(conv) == [[0, 2], [1, 3], [2]]


def test_duplicates_cancel():
    c = CliffordCircuit("M 0 1\nDETECTOR rec[-1] rec[-1]\nDETECTOR rec[-1] rec[-2] rec[-1]\n"
                        "OBSERVABLE_INCLUDE(0) rec[-1]\nOBSERVABLE_INCLUDE(0) rec[-1] rec[-2]")
    conv = c.compile_m2d_converter()
    assert records(conv) == [[], [0], [0]]
    m = np.array([[1, 1], [0, 1], [1, 0]], np.bool_)
    assert restated(conv, m).tolist() == [[False, True, True], [False, False, False], [False, True, True]]


def test_inversions_and_reference_bits():
    c = CliffordCircuit("X 1\nM !0 1 2\nDETECTOR rec[-3]\nDETECTOR rec[-2]\nDETECTOR rec[-1] rec[-2]\nOBSERVABLE_INCLUDE(0) rec[-3] rec[-2]")
    conv = c.compile_m2d_converter()
    assert conv.csr()[2].tolist() == [1, 1, 1, 0]
    assert c.compile_m2d_converter(skip_reference_sample=True).csr()[2].tolist() == [0, 0, 0, 0]
    # the noiseless record converts to all zeros; hand-computed rows
    assert not restated(conv, np.array([[1, 1, 0]])).any()
    assert restated(conv, np.array([[0, 1, 1]])).tolist() == [[True, False, True, True]]
    skip = c.compile_m2d_converter(skip_reference_sample=True)
    assert restated(skip, np.array([[1, 1, 0]])).tolist() == [[True, True, True, False]]


def test_mpad_and_repeat():
    c = CliffordCircuit("MPAD 1 0\nREPEAT 3 {\n  M 0\n  DETECTOR rec[-1] rec[-3]\n}\nDETECTOR rec[-5]")
    conv = c.compile_m2d_converter()
    assert conv.num_measurements == 5
    assert records(conv) == [[0, 2], [1, 3], [2, 4], [0]]
    assert conv.csr()[2].tolist() == [1, 0, 0, 1]


def test_observable_columns_follow_compile():
    c = CliffordCircuit("M 0 1 2\nOBSERVABLE_INCLUDE(3) rec[-1]\nDETECTOR rec[-2]\nOBSERVABLE_INCLUDE(1) rec[-3]\n"
                        "OBSERVABLE_INCLUDE(3) rec[-2]")
    conv = c.compile_m2d_converter()
    prog = c.compile()[0]
    assert conv.num_detectors == int(prog.num_detectors) == 1
    assert conv.num_observables == int(prog.num_outputs) - 1 == 2
    assert records(conv) == [[1], [0], [1, 2]]  # detector, then observables 1 and 3 (index 0 and 2 absent)


def test_surface_code_shapes():
    conv = CliffordCircuit(circuits.rotated_surface_code_memory(5, 5)).compile_m2d_converter()
    assert (conv.num_measurements + 7) // 8 == 19
    assert (conv.num_detectors + conv.num_observables + 7) // 8 == 16


def test_non_deterministic_outputs_raise():
    with pytest.raises(ValueError, match="not deterministic"):
        CliffordCircuit("H 0\nM 0\nDETECTOR rec[-1]").compile_m2d_converter()
    with pytest.raises(ValueError, match="not deterministic"):
        CliffordCircuit("H 0\nM 0\nOBSERVABLE_INCLUDE(0) rec[-1]").compile_m2d_converter()


def test_argument_errors_before_any_device_call():
    conv = CliffordCircuit("M 0 1\nDETECTOR rec[-1]\nOBSERVABLE_INCLUDE(0) rec[-2]").compile_m2d_converter()
    m = np.zeros((4, 2), np.bool_)
    with pytest.raises(ValueError, match="separate_observables=True with append_observables=True"):
        conv.convert(measurements=m, separate_observables=True, append_observables=True)
    with pytest.raises(NotImplementedError):
        conv.convert(measurements=m, sweep_bits=np.zeros((4, 0), np.bool_))
    with pytest.raises(ValueError, match="shape"):
        conv.convert(measurements=np.zeros((4, 3), np.bool_))
    with pytest.raises(ValueError, match="shape"):
        conv.convert(measurements=np.zeros(2, np.bool_))
    with pytest.raises(ValueError, match="shape"):
        conv.convert(measurements=np.zeros((4, 2), np.uint8), bit_packed=True)
    with pytest.raises(ValueError, match="uint8"):
        conv.convert(measurements=np.zeros((4, 1), np.int32), bit_packed=True)
    with pytest.raises(ValueError, match="bool or 0/1 uint8"):
        conv.convert(measurements=np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        conv.convert_device(0, 4, 0, in_row_bytes=2, in_packed=False, out_row_bytes=2, out_packed=False, cols=slice(0, 2, 2))
    with pytest.raises(ValueError, match="cannot hold"):
        conv.convert_device(0, 4, 0, in_row_bytes=1, in_packed=False, out_row_bytes=2, out_packed=False)
    assert conv._h is None  # nothing above created the device handle


def test_empty_results_without_device():
    conv = CliffordCircuit("M 0 1\nDETECTOR rec[-1]\nOBSERVABLE_INCLUDE(0) rec[-2]").compile_m2d_converter()
    assert conv.convert(measurements=np.zeros((0, 2), np.bool_)).shape == (0, 1)
    d, o = conv.convert(measurements=np.zeros((0, 1), np.uint8), bit_packed=True, separate_observables=True)
    assert d.shape == (0, 1) and o.shape == (0, 1) and d.dtype == np.uint8
    none = CliffordCircuit("M 0 1").compile_m2d_converter()
    out = none.convert(measurements=np.ones((5, 2), np.bool_))
    assert out.shape == (5, 0) and out.dtype == np.bool_
    assert none.convert(measurements=np.ones((5, 1), np.uint8), bit_packed=True).shape == (5, 0)
    conv.convert_device(0, 0, 0, in_row_bytes=2, in_packed=False, out_row_bytes=2, out_packed=False)
    assert conv._h is None


def test_restatement_against_hand_computed_rows():
    c = CliffordCircuit("M 0 1 2 3\nDETECTOR rec[-4] rec[-3]\nDETECTOR rec[-3] rec[-2] rec[-1]\nOBSERVABLE_INCLUDE(0) rec[-1]")
    conv = c.compile_m2d_converter()
    m = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1], [0, 1, 1, 0]])
    assert restated(conv, m).astype(int).tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 1], [1, 0, 0]]


def test_limits_of_the_windowed_csr_are_reported():
    """The C ABI refuses, before touching a device, only what its per-window CSR cannot hold."""
    import ctypes as C

    from tsim_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    n_out = 1000
    row_ptr = np.zeros(n_out + 1, np.int32)
    ref = np.zeros(n_out, np.uint8)
    rc = lib.tsim_m2d_create(0, 1 << 30, n_out, _lib.ptr(row_ptr), None, _lib.ptr(ref), C.byref(h))
    assert rc == -95 and b"windows" in lib.tsim_last_error()
    cols = np.array([5], np.int32)
    row_ptr[1:] = 1
    rc = lib.tsim_m2d_create(0, 5, n_out, _lib.ptr(row_ptr), _lib.ptr(cols), _lib.ptr(ref), C.byref(h))
    assert rc == -22 and b"not a measurement record" in lib.tsim_last_error()
