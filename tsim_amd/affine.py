"""Affine measurement sampling of Clifford circuits (``CliffordCircuit.compile_sampler(method="affine")``).

Every measurement record of a Clifford circuit with Pauli noise is an affine GF(2) function of the error bits ``f`` and of
independent uniform bits ``r``, the random outcomes of the noiseless run::

    rec_i = flip_i XOR (XOR of f_b, b in the record's error set) XOR (XOR of r_s, s in the record's random symbols)

``CliffordCircuit.compile_affine_measurements()`` gives that map as a CSR over the columns ``[f | r]``.  Nothing is
autoregressive, so circuits whose records form components too large for the stabilizer-rank engine (or for its
2048-parameter cap) sample at the cost of one XOR per list entry.  The rows are produced by the ``tsim_affine_*`` handle of
``libtsim_hip.so`` (kernel: ``csrc/tsim_affine.hip.h``) and, for circuits sampled without a device and as the oracle of the
tests, by :func:`affine_rows_host`, the numpy statement of the same function.

Random bits: symbol ``s`` of the shot with global index ``g`` is bit ``g % 64`` of ``x0 | x1 << 32`` where
``(x0, x1) = threefry2x32(key, counter = (s, g // 64))``.  ``key`` is one ``_next_key()`` of the sampler per request and
``g`` runs over the request, so the rows depend on the seed and on the shot's index only - never on ``batch_size``, on how
the request is cut into launches, or on whether a GPU did the work.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, prng
from .program import CompiledProgram
from .sampler import CompiledMeasurementSampler, _check_request

__all__ = ["AffineHandle", "CompiledAffineMeasurementSampler", "affine_rows_host", "random_words", "threefry2x32_np"]

_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
MAX_SHOT = 1 << 38  # first_shot + B: the tile index g // 64 is a 32-bit Threefry counter


def threefry2x32_np(k0: int, k1: int, c0, c1) -> tuple[np.ndarray, np.ndarray]:
    """:func:`tsim_amd.prng.threefry2x32` over arrays of counters (uint32, broadcast against each other)."""
    k0, k1 = np.uint32(int(k0) & 0xFFFFFFFF), np.uint32(int(k1) & 0xFFFFFFFF)
    ks = (k0, k1, k0 ^ k1 ^ np.uint32(0x1BD11BDA))
    x0, x1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint32), np.asarray(c1, dtype=np.uint32))
    with np.errstate(over="ignore"):
        x0, x1 = x0 + ks[0], x1 + ks[1]
        for blk in range(5):
            for r in _ROT[blk & 1]:
                x0 = x0 + x1
                x1 = ((x1 << np.uint32(r)) | (x1 >> np.uint32(32 - r))) ^ x0
            x0 = x0 + ks[(blk + 1) % 3]
            x1 = x1 + ks[(blk + 2) % 3] + np.uint32(blk + 1)
    return x0, x1


def random_words(key, n_random: int, tile0: int, n_tiles: int) -> np.ndarray:
    """``uint64[n_tiles, n_random]``: word ``[t, s]`` holds symbol ``s`` of the shots ``64 (tile0 + t) .. + 63``."""
    s = np.arange(n_random, dtype=np.uint32)[None, :]
    t = (int(tile0) + np.arange(n_tiles, dtype=np.int64)).astype(np.uint32)[:, None]
    x0, x1 = threefry2x32_np(key[0], key[1], s, t)
    return x0.astype(np.uint64) | (x1.astype(np.uint64) << np.uint64(32))


def _check_csr(num_f: int, n_random: int, row_ptr, cols, flip) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32).reshape(-1)
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    flip = np.ascontiguousarray(np.asarray(flip, dtype=np.uint8).reshape(-1) & 1)
    if num_f < 0 or n_random < 0:
        raise ValueError(f"bad sizes: num_f={num_f} n_random={n_random}")
    if len(row_ptr) != len(flip) + 1 or row_ptr[0] != 0 or (np.diff(row_ptr) < 0).any() or row_ptr[-1] != len(cols):
        raise ValueError("row_ptr must start at 0, not decrease, end at len(cols) and have one entry more than flip")
    if len(cols) and (cols.min() < 0 or cols.max() >= num_f + n_random):
        raise ValueError(f"a column is outside 0 .. num_f + n_random - 1 = {num_f + n_random - 1}")
    return row_ptr, cols, flip


def affine_rows_host(flip, row_ptr, cols, num_f: int, n_random: int, f_packed, B: int, first_shot: int, key) -> np.ndarray:
    """``uint8[B, n_out]`` (0/1): output ``j`` of shot ``n`` is ``flip[j]`` XOR the columns ``cols[row_ptr[j]:row_ptr[j+1]]``
    (one listed twice cancels) of ``[f | r]``: bit ``c < num_f`` of row ``n`` of ``f_packed`` (little-endian bit rows, uint8
    or uint64, any width that holds ``num_f`` bits; ``None`` when ``num_f = 0``), then the ``n_random`` symbols of shot
    ``first_shot + n`` (module docstring).  The statement the device kernel is tested against, and the sampler's path
    without a device."""
    num_f, n_random, B, first_shot = int(num_f), int(n_random), int(B), int(first_shot)
    row_ptr, cols, flip = _check_csr(num_f, n_random, row_ptr, cols, flip)
    if B < 0 or first_shot < 0 or first_shot + B > MAX_SHOT:
        raise ValueError(f"shots {first_shot} .. {first_shot} + {B} are outside 0 .. 2^38")
    n_out, n_col = len(flip), num_f + n_random
    # S[c, j] = 1 iff column c occurs an odd number of times in the list of output j
    S = np.zeros((n_col, n_out), dtype=np.uint8)
    np.bitwise_xor.at(S, (cols, np.repeat(np.arange(n_out), np.diff(row_ptr))), 1)
    S = S.astype(np.float32)
    if num_f:
        f_bytes = np.ascontiguousarray(f_packed).view(np.uint8).reshape(len(f_packed), -1)
        if len(f_bytes) < B or f_bytes.shape[1] * 8 < num_f:
            raise ValueError(f"f rows of shape {f_bytes.shape} cannot hold {B} x {num_f} bits")
    out = np.empty((B, n_out), dtype=np.uint8)
    step = max(64, (1 << 22) // max(1, n_col) // 64 * 64)  # a few MB of bits at a time
    for lo in range(0, B, step):
        n = min(step, B - lo)
        x = np.empty((n, n_col), dtype=np.float32)
        if num_f:
            x[:, :num_f] = np.unpackbits(f_bytes[lo:lo + n, : (num_f + 7) // 8], axis=1, bitorder="little")[:, :num_f]
        if n_random:
            g0 = first_shot + lo
            t0, t1 = g0 // 64, (g0 + n + 63) // 64
            words = random_words(key, n_random, t0, t1 - t0)
            bits = (words[:, None, :] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)
            x[:, num_f:] = bits.reshape(-1, n_random)[g0 - 64 * t0: g0 - 64 * t0 + n]
        # counts of set columns per output are below 2^24: exact in float32
        out[lo:lo + n] = (x @ S).astype(np.int64) & 1
    return out ^ flip[None, :]


class AffineHandle(_lib.DeviceHandle):
    """``tsim_affine`` of one device: the CSR (``row_ptr``, ``cols`` over ``num_f`` f bits then ``n_random`` symbols) and
    the outputs' constant bits.  The device handle is created by the first launch."""

    def __init__(self, num_f: int, n_random: int, row_ptr, cols, flip, *, device: int = 0):
        self.num_f, self.n_random, self._device = int(num_f), int(n_random), int(device)
        self.row_ptr, self.cols, self.flip = _check_csr(self.num_f, self.n_random, row_ptr, cols, flip)
        self.n_out = len(self.flip)

    CREATE, DESTROY = "tsim_affine_create", "tsim_affine_destroy"
    INFO = ("tsim_affine_info", ("num_f", "n_random", "n_out", "nnz", "device", "window", "n_windows", "lds_bytes_per_wave"))

    def _create_args(self) -> tuple:
        return (self._device, self.num_f, self.n_random, self.n_out, _lib.ptr(self.row_ptr), _lib.ptr(self.cols),
                _lib.ptr(self.flip))

    def sample_device(self, d_f: int, B: int, d_out: int, *, key, first_shot: int = 0, f_row_bytes: int, out_row_bytes: int,
                      out_packed: bool, col0: int = 0, n_cols: int | None = None, stream: int = 0) -> None:
        """Caller-owned device buffers, asynchronous on ``stream`` (0: the handle's own stream); see
        ``tsim_affine_sample_device`` in ``include/tsim_hip.h``."""
        self._request("tsim_affine_sample_device", (C.c_void_p(int(d_f)) if d_f else None, int(f_row_bytes)), B, d_out, key=key,
                      first_shot=first_shot, out_row_bytes=out_row_bytes, out_packed=out_packed, col0=col0, n_cols=n_cols,
                      stream=stream)


class CompiledAffineMeasurementSampler(CompiledMeasurementSampler):
    """A measurement sampler over the affine form of a Clifford circuit.  It is a :class:`CompiledMeasurementSampler` whose
    program has no components: the rows come from the hook such programs use (``_direct_on_device`` / ``_direct_device`` /
    ``_sample_direct``), so ``count()`` and ``sample_write()`` work as they do for every sampler."""

    def __init__(self, form: dict, *, seed: int | None = None, device: int = 0, noise: str = "host"):
        self._form = form
        self._flip = np.ascontiguousarray(form["flip"], dtype=np.uint8)
        n_out = len(self._flip)
        program = CompiledProgram(components=(), direct_f_indices=np.zeros(0, np.int32), direct_flips=np.zeros(0, np.bool_),
                                  output_order=np.arange(n_out, dtype=np.int32), output_reindex=None, num_outputs=n_out,
                                  num_detectors=0)
        super().__init__(program, channel_probs=form["channel_probs"], error_transform=form["error_transform"], seed=seed,
                         device=device, noise=noise)
        self._num_f, self._n_random = int(form["num_f"]), int(form["n_random"])
        if self._num_f != self._channel_sampler.num_f:
            raise ValueError(f"the form has {self._num_f} f bits, its error_transform {self._channel_sampler.num_f}")
        self._row_ptr, self._cols, _ = _check_csr(self._num_f, self._n_random, form["row_ptr"], form["cols"], self._flip)
        self._affine = None
        self._carrier = None

    # -- device plumbing --------------------------------------------------------------------------------------------
    def _hip(self):
        """Device buffers, streams and the noise sampler hang off a program handle; the records are not outputs of any
        engine program, so a one-output direct program carries them."""
        if self._carrier is None:
            from .backend import get_hip_program
            from .program import make_program

            self._carrier = get_hip_program(make_program([], [(0, 0, False)], 1, 0), self._device, self._mode)
        return self._carrier

    def _affine_handle(self) -> AffineHandle:
        """The handle writes whole uint64 words per row: outputs beyond the records are constant zeros, so the padded rows
        the tally and the file sink read need no clearing."""
        if self._affine is None:
            n_out = len(self._flip)
            pad = -n_out % 64
            row_ptr = np.concatenate([self._row_ptr, np.full(pad, self._row_ptr[-1], np.int32)])
            self._affine = AffineHandle(self._num_f, self._n_random, row_ptr, self._cols,
                                        np.concatenate([self._flip, np.zeros(pad, np.uint8)]), device=self._device)
        return self._affine

    def _direct_on_device(self, shots: int) -> bool:
        """``noise="device"``: always.  ``noise="host"``: whenever a device is there - the rows are the same either way."""
        if self._seam_replaced() or not len(self._flip):
            return False
        if self._noise == "device":
            return True
        try:
            _lib.load(build=False)
            return _lib.device_count() > 0
        except Exception:  # noqa: BLE001 - no library / no device: the host statement is complete on its own
            return False

    # -- rows ---------------------------------------------------------------------------------------------------------
    def _sample_direct(self, shots: int) -> np.ndarray:
        """No device: one channel draw for the request, one key, the host statement."""
        f = self._channel_sampler.sample_packed(shots)
        return affine_rows_host(self._flip, self._row_ptr, self._cols, self._num_f, self._n_random, f, shots, 0,
                                self._next_key()).view(np.bool_)

    def _direct_device(self, shots: int, batch_size: int | None, packed_columns: int | None = None, sink=None):
        """The request in chunks of whole 64-shot tiles: f rows (host noise: ONE ``sample_packed(shots)``, uploaded chunk
        by chunk; device noise: the noise kernel, one noise key per chunk), then the affine kernel with ``first_shot``
        running over the request under one key.  ``sink`` (``count()``, ``sample_write()``) takes each chunk's padded
        bit-packed rows where they are; otherwise the rows are written in the layout asked for and downloaded."""
        hp = self._hip()
        n_out, num_f = len(self._flip), self._num_f
        wf, wo = max(1, (num_f + 63) // 64), (n_out + 63) // 64
        if packed_columns is not None and packed_columns != n_out:
            raise ValueError(f"packed_columns = {packed_columns} of {n_out} records")
        chunk = -(-min(shots, batch_size or (1 << 20), 1 << 20) // 64) * 64
        key = self._next_key()
        handle = self._affine_handle()
        host_noise = self._noise == "host"
        f_all = self._channel_sampler.sample_packed(shots) if host_noise else None
        d_f = self._scratch(hp, "affine_f", chunk * wf * 8) if num_f else None
        if sink is not None:
            out, row_bytes, n_cols, packed = None, wo * 8, wo * 64, True
            s_sink = hp.aux_stream(1)
        elif packed_columns is not None:
            row_bytes, n_cols, packed = (n_out + 7) // 8, n_out, True
            out = np.empty((shots, row_bytes), dtype=np.uint8)
        else:
            row_bytes, n_cols, packed = n_out, n_out, False
            out = np.empty((shots, n_out), dtype=np.uint8)
        d_rows = self._scratch(hp, "affine_rows", chunk * row_bytes + 16)
        stream = hp.stream_ptr()
        for lo in range(0, shots, chunk):
            n = min(chunk, shots - lo)
            if num_f and host_noise:
                hp.h2d(d_f, f_all[lo:lo + n])
            elif num_f:
                self._noise_key, sub = prng.split(self._noise_key)
                self._device_noise_sampler(hp).sample_into(d_f.ptr, n, sub, stream)
            handle.sample_device(d_f.ptr if num_f else 0, n, d_rows.ptr, key=key, first_shot=lo, f_row_bytes=wf * 8,
                                 out_row_bytes=row_bytes, out_packed=packed, n_cols=n_cols, stream=stream)
            hp.stream_synchronize(stream)
            if sink is not None:  # (the next chunk overwrites the rows: the sink finishes first)
                sink(d_rows.ptr, row_bytes, lo, lo + n, s_sink)
                hp.stream_synchronize(s_sink)
            else:
                hp.d2h(out[lo:lo + n], d_rows.ptr)
        if out is None:
            return None
        return out if packed_columns is not None else out.view(np.bool_)

    def sample(self, shots: int, batch_size: int | None = None, bit_packed: bool = False) -> np.ndarray:
        """``bool[shots, num_measurements]``, or - ``bit_packed=True`` - ``uint8[shots, ceil(num_measurements / 8)]``
        little-endian bit rows.  For a fixed seed the rows do not depend on ``batch_size`` with ``noise="host"``."""
        _check_request(shots, batch_size)
        n_out = len(self._flip)
        if shots == 0:
            return np.empty((0, (n_out + 7) // 8), np.uint8) if bit_packed else np.empty((0, n_out), np.bool_)
        if self._direct_on_device(shots):
            return self._direct_device(shots, batch_size, packed_columns=n_out if bit_packed else None)
        rows = self._sample_direct(shots)
        return np.packbits(rows.view(np.uint8), axis=1, bitorder="little") if bit_packed else rows

    def __repr__(self) -> str:
        return (f"CompiledAffineMeasurementSampler({len(self._flip)} records, {self._num_f} error bits in the basis, "
                f"{self._n_random} random symbols, {len(self._cols)} list entries)")
