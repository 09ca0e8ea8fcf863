"""Measurements -> detection events on the GPU (``Circuit.compile_m2d_converter``, src/tsim/circuit.py:423-456).

The reference hands this call to stim's ``CompiledMeasurementsToDetectionEventsConverter``; here it is the
``tsim_m2d_*`` handle of ``libtsim_hip.so`` (kernel: ``csrc/tsim_m2d.hip.h``).  Per shot every output is
``ref_j XOR (XOR of the measurement records in S_j)``: the detectors in order, then the observables in the columns
``CliffordCircuit.compile()`` gives them.  Arguments are checked before any device call, and the device handle is only
created by the first conversion that has work to do.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

__all__ = ["CompiledMeasurementsToDetectionEventsConverter"]

_BOTH_FLAGS = "Can't specify separate_observables=True with append_observables=True or prepend_observables=True"


class CompiledMeasurementsToDetectionEventsConverter(_lib.DeviceHandle):
    """stim's converter surface over a CSR of record indices: ``records[j]`` lists the measurement records output ``j``
    XORs (outputs = ``num_detectors`` detectors, then the observables), ``ref[j]`` its constant bit."""

    def __init__(self, records: list, ref, *, num_measurements: int, num_detectors: int, device: int = 0):
        self._M = int(num_measurements)
        self._nd = int(num_detectors)
        self._n_out = len(records)
        if not 0 <= self._nd <= self._n_out:
            raise ValueError(f"num_detectors={self._nd} of {self._n_out} outputs")
        self._row_ptr = np.zeros(self._n_out + 1, np.int32)
        self._row_ptr[1:] = np.cumsum([len(r) for r in records], dtype=np.int64)
        self._cols = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int64) for r in records]) if records else
                                          np.zeros(0, np.int64), dtype=np.int32)
        if self._cols.size and (self._cols.min() < 0 or self._cols.max() >= self._M):
            raise ValueError("a record index is outside 0 .. num_measurements - 1")
        self._ref = np.ascontiguousarray(np.asarray(ref, dtype=np.uint8).reshape(-1) & 1)
        if self._ref.shape != (self._n_out,):
            raise ValueError(f"ref must have {self._n_out} entries")
        self._device = int(device)

    # -- stim's properties ---------------------------------------------------------------------------------------
    @property
    def num_measurements(self) -> int:
        return self._M

    @property
    def num_detectors(self) -> int:
        return self._nd

    @property
    def num_observables(self) -> int:
        return self._n_out - self._nd

    def csr(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(row_ptr, cols, ref)`` as the device handle receives them."""
        return self._row_ptr.copy(), self._cols.copy(), self._ref.copy()

    # -- the device handle ------------------------------------------------------------------------------------------
    CREATE, DESTROY = "tsim_m2d_create", "tsim_m2d_destroy"
    INFO = ("tsim_m2d_info", ("num_measurements", "n_out", "nnz", "device"))

    def _create_args(self) -> tuple:
        return self._device, self._M, self._n_out, _lib.ptr(self._row_ptr), _lib.ptr(self._cols), _lib.ptr(self._ref)

    # -- conversion -------------------------------------------------------------------------------------------------
    def _columns(self, separate_observables: bool, append_observables: bool) -> list[tuple[int, int]]:
        if separate_observables and append_observables:
            raise ValueError(_BOTH_FLAGS)
        if separate_observables:
            return [(0, self._nd), (self._nd, self._n_out - self._nd)]
        return [(0, self._n_out if append_observables else self._nd)]

    def _input(self, measurements, bit_packed: bool) -> np.ndarray:
        m = np.asarray(measurements)
        width = (self._M + 7) // 8 if bit_packed else self._M
        if m.ndim != 2 or m.shape[1] != width:
            raise ValueError(f"measurements must have shape [B, {width}] ({'bit-packed ' if bit_packed else ''}"
                             f"{self._M} measurements), got {m.shape}")
        if bit_packed and m.dtype != np.uint8:
            raise ValueError(f"bit-packed measurements must be uint8, got {m.dtype}")
        if not bit_packed and m.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"measurements must be bool or 0/1 uint8, got {m.dtype}")
        return np.ascontiguousarray(m).view(np.uint8)

    def convert(self, *, measurements, sweep_bits=None, separate_observables: bool = False, append_observables: bool = False,
                bit_packed: bool = False):
        """Detection events (and observable flips) of measurement rows, stim's ``convert`` surface: bool rows, or
        ``bit_packed=True`` little-endian bytes in and out (pad bits ignored on input, zero on output)."""
        if sweep_bits is not None:
            raise NotImplementedError("sweep bits are not supported: the Clifford front-end has no sweep[] targets")
        blocks = self._columns(separate_observables, append_observables)
        m = self._input(measurements, bit_packed)
        if separate_observables:
            # one pass over the input for both blocks: every output unpacked, split (and packed) on the host
            rows = self._run(m, bit_packed, 0, self._n_out, False).view(np.bool_)
            det, obs = np.ascontiguousarray(rows[:, :self._nd]), np.ascontiguousarray(rows[:, self._nd:])
            if bit_packed:
                return (np.packbits(det.view(np.uint8), axis=1, bitorder="little"),
                        np.packbits(obs.view(np.uint8), axis=1, bitorder="little"))
            return det, obs
        (col0, n), = blocks
        out = self._run(m, bit_packed, col0, n, bit_packed)
        return out if bit_packed else out.view(np.bool_)

    def _run(self, m: np.ndarray, in_packed: bool, col0: int, n: int, out_packed: bool) -> np.ndarray:
        B = int(m.shape[0])
        width = (n + 7) // 8 if out_packed else n
        out = np.zeros((B, width), np.uint8)
        if B and n:
            _lib.check(_lib.load().tsim_m2d_convert(self._handle(), _lib.ptr(m), B, int(m.shape[1]), int(in_packed),
                                                    _lib.ptr(out), width, int(out_packed), col0, n), "tsim_m2d_convert")
        return out

    def convert_device(self, d_meas: int, B: int, d_out: int, *, in_row_bytes: int, in_packed: bool, out_row_bytes: int,
                       out_packed: bool, cols: slice | None = None, stream: int = 0) -> None:
        """Caller-owned device buffers, asynchronous on ``stream`` (0: the converter's own stream).  ``cols``: a slice
        of the outputs (default: all, detectors then observables); rows are ``in_row_bytes`` / ``out_row_bytes`` apart,
        so the padded ``uint64`` rows of :meth:`HipProgram.sample_steps_device` chain in with ``in_row_bytes = 8 *
        ceil(M / 64)``."""
        start, stop, step = (cols if cols is not None else slice(None)).indices(self._n_out)
        if step != 1:
            raise ValueError("cols must be a contiguous slice")
        n = max(0, stop - start)
        if int(B) < 0:
            raise ValueError("negative B")
        in_used = (self._M + 7) // 8 if in_packed else self._M
        out_used = (n + 7) // 8 if out_packed else n
        if int(in_row_bytes) < in_used or int(out_row_bytes) < out_used:
            raise ValueError(f"rows of {in_row_bytes} / {out_row_bytes} bytes cannot hold {in_used} / {out_used}")
        if int(B) == 0 or n == 0:
            return
        _lib.check(_lib.load().tsim_m2d_convert_device(self._handle(), C.c_void_p(int(d_meas)), int(B), int(in_row_bytes),
                                                       int(bool(in_packed)), C.c_void_p(int(d_out)), int(out_row_bytes),
                                                       int(bool(out_packed)), start, n, stream or None),
                   "tsim_m2d_convert_device")

    def convert_file(self, *, measurements_filepath, measurements_format: str = "01", sweep_bits_filepath=None,
                     sweep_bits_format: str = "01", detection_events_filepath, detection_events_format: str = "01",
                     append_observables: bool = False, obs_out_filepath=None, obs_out_format: str = "01") -> None:
        """stim's ``convert_file``: the measurement file is decoded on the device (:mod:`tsim_amd.shotdata`), converted by
        :meth:`convert_device` and encoded on the device - the rows never exist on the host.  The detection event file
        (and ``obs_out_filepath``'s observables) equal the encoding of ``convert(measurements=<the file's rows>,
        append_observables=append_observables)`` (``dets``: measurements ``M``, detectors ``D``, observables ``L``)."""
        from . import shotdata

        if sweep_bits_filepath is not None:
            raise NotImplementedError("sweep bits are not supported: the Clifford front-end has no sweep[] targets")
        for f in (measurements_format, sweep_bits_format, detection_events_format) + ((obs_out_format,) if obs_out_filepath is not None else ()):
            shotdata.check_format(f)
        if obs_out_filepath is not None and append_observables:
            raise ValueError("Can't specify obs_out_filepath with append_observables=True")
        if measurements_format in ("b8", "ptb64") and self._M < 1:
            raise ValueError(f"{measurements_format} needs at least one measurement to be read")
        n_obs = self._n_out - self._nd
        main = slice(0, self._n_out if append_observables else self._nd)
        outs = [(detection_events_filepath, detection_events_format, main, (0, self._nd, n_obs if append_observables else 0))]
        if obs_out_filepath is not None:
            outs.append((obs_out_filepath, obs_out_format, slice(self._nd, self._n_out), (0, 0, n_obs)))
        c = shotdata.codec(self._device)
        lib = _lib.load()
        writers, slots = [], []
        try:
            for path, fmt, cols, sec in outs:
                writers.append(shotdata.ShotWriter(path, fmt, cols.stop - cols.start, sec, device=self._device))
                slots.append(c.take_slot())
            for d_meas, B, rb in shotdata.iter_device_rows(measurements_filepath, measurements_format, self._M, (self._M, 0, 0),
                                                                  device=self._device):
                for w, (_p, _f, cols, _s), slot in zip(writers, outs, slots):
                    n = cols.stop - cols.start
                    ob = (n + 7) // 8
                    d_out = c.staging(slot, B * ob, pinned=False)
                    self.convert_device(d_meas, B, d_out, in_row_bytes=rb, in_packed=True, out_row_bytes=ob, out_packed=True, cols=cols)
                    _lib.check(lib.tsim_device_synchronize(self._device), "tsim_device_synchronize")
                    w.write_device(d_out, B, ob)
                for w in writers:  # the decoded rows and the outputs are reused by the next chunk
                    w._flush(0)
                c.sync()
        except BaseException:
            for w in writers:
                w.abort()
            for s in slots:
                c.give_slot(s)
            raise
        for s in slots:
            c.give_slot(s)
        shotdata.close_all(writers)

    def __repr__(self) -> str:
        return (f"CompiledMeasurementsToDetectionEventsConverter(num_measurements={self._M}, "
                f"num_detectors={self._nd}, num_observables={self.num_observables})")
