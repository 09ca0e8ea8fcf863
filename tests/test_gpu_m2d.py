"""The measurements -> detection events kernel (tsim_m2d_*) on the device: bit-exact against a numpy restatement for
random record lists and inputs, and chained behind the measurement sampler."""

import ctypes as C

import numpy as np
import pytest

from tsim_amd import circuits, synth
from tsim_amd.channels import ChannelSampler
from tsim_amd.clifford import CliffordCircuit
from tsim_amd.m2d import CompiledMeasurementsToDetectionEventsConverter

pytestmark = pytest.mark.gpu


def restated(conv, m: np.ndarray) -> np.ndarray:
    """``(m @ A.T + ref) % 2`` (all outputs), formed as prefix XORs over the gathered record columns."""
    row_ptr, cols, ref = conv.csr()
    g = (np.asarray(m) != 0).astype(np.uint8)[:, cols]
    px = np.zeros((len(g), len(cols) + 1), np.uint8)
    if len(cols):
        np.bitwise_xor.accumulate(g, axis=1, out=px[:, 1:])
    return (px[:, row_ptr[1:]] ^ px[:, row_ptr[:-1]] ^ ref[None, :]).astype(np.bool_)


def random_converter(M: int, n_out: int, seed: int) -> CompiledMeasurementsToDetectionEventsConverter:
    rng = np.random.default_rng(seed)
    records = []
    for j in range(n_out):
        k = int(rng.integers(0, 6))
        centre = int(rng.integers(0, M))
        records.append(sorted({int(x) % M for x in centre + rng.integers(-70, 70, k)}) if j % 7 else
                       sorted(set(rng.integers(0, M, k).tolist())))  # local lists, and some anywhere in the record
    ref = rng.integers(0, 2, n_out)
    return CompiledMeasurementsToDetectionEventsConverter(records, ref, num_measurements=M, num_detectors=max(0, n_out - 3))


def pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")


CASES = [(1, 5), (63, 40), (64, 64), (65, 70), (145, 121), (1441, 1321), (5185, 4896)]


@pytest.mark.parametrize("M,n_out", CASES)
def test_convert_matches_restatement(hip, M, n_out):
    conv = random_converter(M, n_out, seed=M)
    rng = np.random.default_rng(M + 1)
    B = 1000 if M < 5000 else 7000  # 7000 rows of 10 KB: two staged chunks of the host convert
    m = rng.integers(0, 2, (B, M)).astype(np.bool_)
    want = restated(conv, m)
    nd = conv.num_detectors
    packed_in = pack(m)
    if M % 8:  # garbage in the pad bits of the last byte
        packed_in[:, -1] |= (rng.integers(0, 256, B).astype(np.uint8) & np.uint8((0xFF << (M % 8)) & 0xFF))
    for bit_packed in (False, True):
        inputs = [packed_in] if bit_packed else [m, m.astype(np.uint8)]
        for x in inputs:
            got = conv.convert(measurements=x, bit_packed=bit_packed)
            assert np.array_equal(got, pack(want[:, :nd]) if bit_packed else want[:, :nd])
            got = conv.convert(measurements=x, bit_packed=bit_packed, append_observables=True)
            assert np.array_equal(got, pack(want) if bit_packed else want)
            d, o = conv.convert(measurements=x, bit_packed=bit_packed, separate_observables=True)
            assert np.array_equal(d, pack(want[:, :nd]) if bit_packed else want[:, :nd])
            assert np.array_equal(o, pack(want[:, nd:]) if bit_packed else want[:, nd:])
            assert (d.dtype, o.dtype) == ((np.uint8, np.uint8) if bit_packed else (np.bool_, np.bool_))


@pytest.mark.parametrize("M,n_out", [(63, 40), (145, 121), (1441, 1321)])
def test_convert_device_strides_and_packings(hip, M, n_out):
    """Caller-owned device rows with padded strides (the uint64 rows of the sampler), every in/out packing, a slice."""
    conv = random_converter(M, n_out, seed=3 * M)
    hp = hip.HipProgram(synth.kat_h_m(), device=0)  # device buffers and a stream
    rng = np.random.default_rng(M)
    B = 333
    m = rng.integers(0, 2, (B, M)).astype(np.uint8)
    want = restated(conv, m)
    for in_packed in (False, True):
        rows = pack(m) if in_packed else m
        in_rb = 8 * ((rows.shape[1] + 7) // 8) + 8
        host_in = rng.integers(0, 256, (B, in_rb)).astype(np.uint8)  # garbage past the used bytes
        host_in[:, :rows.shape[1]] = rows
        if in_packed and M % 8:
            host_in[:, rows.shape[1] - 1] |= np.uint8((0xFF << (M % 8)) & 0xFF)
        d_in = hp.malloc(host_in.nbytes)
        hp.h2d(d_in, host_in)
        for out_packed in (False, True):
            for sl in (slice(None), slice(2, n_out - 1)):
                start, stop, _ = sl.indices(n_out)
                n = stop - start
                used = (n + 7) // 8 if out_packed else n
                out_rb = used + 5
                got = np.full((B, out_rb), 0xA5, np.uint8)
                d_out = hp.malloc(got.nbytes)
                hp.h2d(d_out, got)
                conv.convert_device(d_in.ptr, B, d_out.ptr, in_row_bytes=in_rb, in_packed=in_packed,
                                    out_row_bytes=out_rb, out_packed=out_packed, cols=sl, stream=hp.stream_ptr())
                hp.synchronize()
                hp.d2h(got, d_out)
                d_out.free()
                w = want[:, start:stop]
                assert np.array_equal(got[:, :used], pack(w) if out_packed else w.astype(np.uint8)), (in_packed, out_packed, sl)
                assert (got[:, used:] == 0xA5).all()  # bytes past a row's outputs are not written
        d_in.free()
    hp.close()


def test_noiseless_surface_code_converts_to_zeros(hip):
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3))
    ms = c.compile_sampler(seed=11).sample(2000)
    assert (ms.any(axis=0) & ~ms.all(axis=0)).any(), "the records should carry random outcomes"
    conv = c.compile_m2d_converter()
    assert not conv.convert(measurements=ms, append_observables=True).any()
    assert not conv.convert(measurements=pack(ms), bit_packed=True, append_observables=True).any()
    # without the reference bits the conversion is the noiseless outputs' values
    skip = c.compile_m2d_converter(skip_reference_sample=True)
    assert np.array_equal(skip.convert(measurements=ms, append_observables=True),
                          np.broadcast_to(conv.csr()[2].astype(np.bool_), (len(ms), conv.num_detectors + conv.num_observables)))


def test_noisy_rates_agree_with_detector_sampler(hip):
    text = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.01,
                                                before_round_data_depolarization=0.01, before_measure_flip_probability=0.01)
    c = CliffordCircuit(text)
    N = 10**6
    ms = c.compile_sampler(seed=21).sample(N)
    conv = c.compile_m2d_converter()
    got = conv.convert(measurements=ms, append_observables=True).mean(axis=0)
    want = c.compile_detector_sampler(seed=22).sample(N, append_observables=True).mean(axis=0)
    p = (got + want) / 2
    sigma = np.sqrt(2 * p * (1 - p) / N)
    assert (want > 0.005).all(), "every detector should fire at this noise level"
    assert (np.abs(got - want) <= 5 * sigma + 1e-12).all(), np.abs(got - want) / np.maximum(sigma, 1e-12)


def test_device_chain_behind_sample_steps(hip):
    """Padded uint64 rows of HipProgram.sample_steps_device -> convert_device on the program's stream == host conversion."""
    text = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.02, before_measure_flip_probability=0.02)
    c = CliffordCircuit(text)
    prog, probs, et = c.compile_measurements()
    hp = hip.HipProgram(prog, device=0)
    cs = ChannelSampler(channel_probs=probs, error_transform=et, seed=5)
    B, nf, M = 5000, int(et.shape[0]), int(prog.num_outputs)
    f = cs.sample_packed(B)
    wo = (M + 63) // 64
    conv = c.compile_m2d_converter()
    n_out = conv.num_detectors + conv.num_observables
    rb = (n_out + 7) // 8
    d_f, d_o, d_e = hp.malloc(f.nbytes), hp.malloc(B * wo * 8), hp.malloc(B * rb)
    hp.h2d(d_f, f)
    ks = (C.c_uint32 * 2)(0, 7)
    hp.sample_steps_device([d_f.ptr], B, nf, ks, [d_o.ptr])
    hp.pipeline_join(0)
    conv.convert_device(d_o.ptr, B, d_e.ptr, in_row_bytes=8 * wo, in_packed=True, out_row_bytes=rb, out_packed=True,
                        stream=hp.stream_ptr())
    hp.synchronize()
    rows = np.zeros((B, 8 * wo), np.uint8)
    hp.d2h(rows, d_o)
    events = np.zeros((B, rb), np.uint8)
    hp.d2h(events, d_e)
    host = conv.convert(measurements=rows[:, : (M + 7) // 8], bit_packed=True, append_observables=True)
    assert np.array_equal(events, host)
    assert events.any(), "noise at 2 % should fire some detectors"
    hp.close()


def test_addresses_past_2_gib(hip):
    """B * in_row_bytes > 2^31: the rows at the end of the buffer are converted from the right addresses."""
    c = CliffordCircuit(circuits.rotated_surface_code_memory(5, 5))
    conv = c.compile_m2d_converter()
    M, n_out = conv.num_measurements, conv.num_detectors + conv.num_observables
    in_rb, rb = 4096, (n_out + 7) // 8
    B = (1 << 31) // in_rb + 1001
    assert B * in_rb > 1 << 31
    hp = hip.HipProgram(synth.kat_h_m(), device=0)
    d_in, d_out = hp.malloc(B * in_rb), hp.malloc(B * rb)
    rng = np.random.default_rng(3)
    # 65537 rows (256 MiB) tiled over the buffer: the period does not divide 2^32 / in_rb rows, so a row offset that
    # wrapped at 32 bits would read a row of other contents
    block = rng.integers(0, 256, ((1 << 16) + 1, in_rb)).astype(np.uint8)
    for r0 in range(0, B, len(block)):
        n = min(len(block), B - r0)
        hp.h2d(d_in.ptr + r0 * in_rb, block[:n])
    conv.convert_device(d_in.ptr, B, d_out.ptr, in_row_bytes=in_rb, in_packed=True, out_row_bytes=rb, out_packed=True,
                        stream=hp.stream_ptr())
    hp.synchronize()
    assert ((1 << 32) // in_rb) % len(block) != 0
    for lo, hi in ((0, 300), (B - 1500, B)):
        got = np.zeros((hi - lo, rb), np.uint8)
        hp.d2h(got, d_out.ptr + lo * rb)
        rows = block[np.arange(lo, hi) % len(block), : (M + 7) // 8]
        bits = np.unpackbits(rows, axis=1, bitorder="little")[:, :M]
        assert np.array_equal(got, pack(restated(conv, bits)))
    hp.close()


@pytest.mark.parametrize("M,n_out", [(7617, 300), (65536, 65536)])
def test_records_in_windows(hip, M, n_out):
    """More records than one wave's LDS holds (7616): windows of record columns, outputs up to 65,536."""
    conv = random_converter(M, n_out, seed=M)
    rng = np.random.default_rng(M + 2)
    B = 200
    m = rng.integers(0, 2, (B, M)).astype(np.bool_)
    want = restated(conv, m)
    nd = conv.num_detectors
    assert np.array_equal(conv.convert(measurements=m, append_observables=True), want)
    packed_in = pack(m)
    if M % 8:
        packed_in[:, -1] |= np.uint8((0xFF << (M % 8)) & 0xFF)
    assert np.array_equal(conv.convert(measurements=packed_in, bit_packed=True, append_observables=True), pack(want))
    d, o = conv.convert(measurements=packed_in, bit_packed=True, separate_observables=True)
    assert np.array_equal(d, pack(want[:, :nd])) and np.array_equal(o, pack(want[:, nd:]))


def test_distance_21_surface_code(hip):
    """rotated_surface_code_memory(21, 21): 9681 records, converted in windows, against the restatement."""
    conv = CliffordCircuit(circuits.rotated_surface_code_memory(21, 21)).compile_m2d_converter()
    assert conv.num_measurements == 9681
    rng = np.random.default_rng(21)
    m = rng.random((500, conv.num_measurements)) < 0.05
    want = restated(conv, m)
    assert np.array_equal(conv.convert(measurements=m, append_observables=True), want)
    assert np.array_equal(conv.convert(measurements=pack(m), bit_packed=True, append_observables=True), pack(want))
