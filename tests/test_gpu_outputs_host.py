"""The host side the column-list handles share (csrc/tsim_outputs_host.hip.h), on the device: the same lists and the same input
bits through the converter (tsim_m2d_*, bit-packed input) and through the affine handle without random symbols (tsim_affine_*,
``num_f = M``, ``flip = ref``) give the same rows, equal to a numpy restatement - for one window of 64 columns, the largest
single window (7616 columns) and the smallest windowed form (7617 columns: four windows of 2048)."""

import ctypes as C

import numpy as np
import pytest

from tsim_amd import _lib, affine, m2d, synth

pytestmark = pytest.mark.gpu

N_OUT, B = 70, 130  # 130 rows: two whole tiles and a tail of two
KEY = (0x13198A2E, 0x03707344)
RANGES = ((0, N_OUT), (3, 65))
SLACK = 5


def lists(M: int):
    """70 outputs over M columns: up to 12 columns each (the first list empty, one column listed twice), and the columns on
    both sides of every seam of windows of 2048 columns, the first and the last."""
    rng = np.random.default_rng(M)
    records = [sorted(rng.choice(M, size=int(n), replace=False).tolist()) for n in rng.integers(0, 13, N_OUT)]
    records[0] = []
    records[1] = [M - 1, 0, M - 1]
    seams = [c for s in range(2048, M, 2048) for c in (s - 1, s)] + [0, M - 1]
    for i, c in enumerate(seams):
        records[2 + i % (N_OUT - 2)].append(c)
    records[-1] = seams + records[-1]  # one list that crosses every seam
    return records, rng.integers(0, 2, N_OUT).astype(np.uint8)


def restate(records, ref, bits):
    out = np.empty((len(bits), len(records)), np.uint8)
    for j, r in enumerate(records):
        out[:, j] = ref[j] ^ (np.bitwise_xor.reduce(bits[:, r], axis=1) if r else 0)
    return out


def pack(bits):
    return np.packbits(bits, axis=1, bitorder="little")


@pytest.fixture(scope="module")
def hp(hip):
    prog = hip.HipProgram(synth.kat_h_m(), device=0)  # device buffers and a stream
    yield prog
    prog.close()


class Pair:
    """The converter and the affine handle of one set of lists, and the input rows on the device (stride with slack, garbage in
    the pad bits and past them)."""

    def __init__(self, hp, M):
        self.hp, self.M = hp, M
        self.records, self.ref = lists(M)
        self.conv = m2d.CompiledMeasurementsToDetectionEventsConverter(self.records, self.ref, num_measurements=M, num_detectors=N_OUT)
        row_ptr, cols, ref = self.conv.csr()
        self.aff = affine.AffineHandle(M, 0, row_ptr, cols, ref)
        rng = np.random.default_rng(M + 1)
        self.in_rb = 8 * ((M + 63) // 64) + 8
        rows = rng.integers(0, 256, (B, self.in_rb)).astype(np.uint8)
        self.want = restate(self.records, self.ref, np.unpackbits(rows, axis=1, bitorder="little")[:, :M])
        self.d_in = hp.malloc(rows.nbytes)
        hp.h2d(self.d_in, rows)

    def run(self, which, n_rows, out_packed, col0, n_cols):
        """One call into a 0xA5-filled buffer of ``B`` rows: ``(used bytes per row, the rows with their slack)``."""
        used = (n_cols + 7) // 8 if out_packed else n_cols
        rb = used + SLACK
        got = np.full((B, rb), 0xA5, np.uint8)
        d_out = self.hp.malloc(got.nbytes)
        self.hp.h2d(d_out, got)
        if which == "m2d":  # (convert_device returns before the library for an empty request: the call itself)
            _lib.check(_lib.load().tsim_m2d_convert_device(self.conv._handle(), C.c_void_p(self.d_in.ptr), n_rows, self.in_rb, 1,
                                                           C.c_void_p(d_out.ptr), rb, int(out_packed), col0, n_cols,
                                                           self.hp.stream_ptr() or None), "tsim_m2d_convert_device")
        else:
            self.aff.sample_device(self.d_in.ptr, n_rows, d_out.ptr, key=KEY, first_shot=0, f_row_bytes=self.in_rb, out_row_bytes=rb,
                                   out_packed=out_packed, col0=col0, n_cols=n_cols, stream=self.hp.stream_ptr())
        self.hp.synchronize()
        self.hp.d2h(got, d_out)
        d_out.free()
        return used, got

    def close(self):
        self.d_in.free()
        self.conv.close()
        self.aff.close()


@pytest.mark.parametrize("M", [64, 7616, 7617])
def test_converter_and_affine_handle_agree(hp, M):
    p = Pair(hp, M)
    info = p.aff.info()
    assert (info["window"], info["n_windows"]) == ((M, 1) if M <= 7616 else (2048, 4))
    assert info["lds_bytes_per_wave"] == 8 * info["window"] + 4416 <= 65536
    assert p.conv.info() == {"num_measurements": M, "n_out": N_OUT, "nnz": sum(map(len, p.records)), "device": 0}
    for out_packed in (False, True):
        for col0, n_cols in RANGES:
            w = p.want[:, col0:col0 + n_cols]
            w = pack(w) if out_packed else w
            for which in ("m2d", "affine"):
                used, got = p.run(which, B, out_packed, col0, n_cols)
                assert np.array_equal(got[:, :used], w), (which, out_packed, col0)
                assert (got[:, used:] == 0xA5).all(), (which, out_packed, col0)  # bytes past a row's outputs are not written
    for which in ("m2d", "affine"):  # empty requests succeed and write nothing
        for n_rows, n_cols in ((0, 65), (B, 0)):
            _, got = p.run(which, n_rows, True, 3, n_cols)
            assert (got == 0xA5).all(), (which, n_rows, n_cols)
    p.close()
