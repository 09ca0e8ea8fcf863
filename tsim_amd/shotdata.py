"""stim's shot-data file formats, encoded and decoded on the GPU (``tsim_shotdata_*``, kernels: ``csrc/tsim_shotdata.hip.h``).

A row of ``n`` bits, columns ``0 .. n-1``, is written as:

- ``01``: ``n`` characters ``'0'`` / ``'1'``, then ``'\\n'``;
- ``b8``: ``ceil(n/8)`` bytes, column ``c`` = bit ``c % 8`` of byte ``c // 8`` (pad bits 0);
- ``r8``: per 1 bit (and an implicit 1 at column ``n``) the number of 0 bits before it, 255 meaning "255 zeros, the run
  continues";
- ``ptb64``: shots in groups of 64; per group and column a little-endian uint64 whose bit ``s`` is shot ``64 g + s``;
- ``hits``: the set columns, ascending, in decimal, separated by ``','``, then ``'\\n'``;
- ``dets``: ``"shot"``, then ``" M<k>"`` / ``" D<k>"`` / ``" L<k>"`` per set column of the measurement, detector and
  observable sections, then ``'\\n'``.

Readers accept what the writers write, tokens of ``hits`` / ``dets`` in any order (duplicates set the bit once), more than
one space between ``dets`` tokens and a last text row without its ``'\\n'``; anything else is a ``ValueError`` naming the
file and the byte offset of the first fault.  Files stream through the device in chunks of :data:`CHUNK_BYTES` (a row
longer than a chunk grows it): files larger than HBM work, and results do not depend on the chunk size.
"""

from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

from . import _lib

__all__ = ["FORMATS", "read_shot_data_file", "write_shot_data_file", "encode_rows_device", "decode_bytes_device", "CHUNK_BYTES"]

FORMATS = ("01", "b8", "r8", "ptb64", "hits", "dets")
CHUNK_BYTES = 16 << 20  # file bytes per device chunk (tests lower it)
ROW_BUFFER_BYTES = 64 << 20  # decoded rows per device pass, at most

_FAULTS = {1: "bad character", 2: "01 line of the wrong length", 3: "index outside its section", 4: "unknown or missing dets prefix",
           5: "r8 run past the end of the row", 6: "the file ends inside a row", 7: "malformed token"}


def check_format(format: str) -> int:
    """The format's code (its index in :data:`FORMATS`); ``ValueError`` for an unknown name."""
    if not isinstance(format, str) or format not in FORMATS:
        raise ValueError(f"unknown shot data format {format!r}; expected one of {', '.join(FORMATS)}")
    return FORMATS.index(format)


def check_sections(num_measurements: int, num_detectors: int, num_observables: int) -> tuple:
    sec = tuple(int(x) for x in (num_measurements, num_detectors, num_observables))
    if min(sec) < 0:
        raise ValueError(f"section sizes must be non-negative, got {sec}")
    return sec


# -- the device handle ------------------------------------------------------------------------------------------------
class _Codec:
    """``tsim_shotdata`` of one device, and the staging slots it lends to readers and writers."""

    SLOTS = 16

    def __init__(self, device: int):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.tsim_shotdata_create(int(device), C.byref(h)), "tsim_shotdata_create")
        self.h, self.device = h, int(device)
        self._free = list(range(self.SLOTS))
        weakref.finalize(self, self.lib.tsim_shotdata_destroy, h)

    def take_slot(self) -> int:
        if not self._free:
            raise RuntimeError("no staging slot left")
        return self._free.pop(0)

    def give_slot(self, slot: int) -> None:
        self._free.insert(0, slot)

    def staging(self, slot: int, nbytes: int, pinned: bool) -> int:
        p = C.c_void_p()
        _lib.check(self.lib.tsim_shotdata_staging(self.h, int(slot), int(bool(pinned)), int(nbytes), C.byref(p)), "tsim_shotdata_staging")
        return int(p.value or 0)

    def copy(self, dst: int, src: int, nbytes: int, stream: int = 0) -> None:
        if nbytes:
            _lib.check(self.lib.tsim_shotdata_copy(self.h, C.c_void_p(dst), C.c_void_p(src), int(nbytes), C.c_void_p(stream) if stream else None),
                       "tsim_shotdata_copy")

    def sync(self, stream: int = 0) -> None:
        _lib.check(self.lib.tsim_shotdata_synchronize(self.h, C.c_void_p(stream) if stream else None), "tsim_shotdata_synchronize")

    def encode(self, fmt: int, d_rows: int, n: int, row_bytes: int, n_bits: int, sec: tuple, d_out: int, out_cap: int,
               stream: int = 0) -> int:
        nbytes = C.c_int64(0)
        rc = self.lib.tsim_shotdata_encode(self.h, fmt, C.c_void_p(d_rows) if d_rows else None, int(n), int(row_bytes), int(n_bits),
                                           sec[0], sec[1], sec[2], C.c_void_p(d_out) if d_out else None, int(out_cap),
                                           C.byref(nbytes), C.c_void_p(stream) if stream else None)
        _lib.check(rc, "tsim_shotdata_encode")
        return int(nbytes.value)

    def decode(self, fmt: int, d_in: int, n_in: int, final: bool, n_bits: int, sec: tuple, d_rows: int, row_bytes: int, max_rows: int,
               stream: int = 0) -> tuple:
        res = (C.c_int64 * 4)()
        _lib.check(self.lib.tsim_shotdata_decode(self.h, fmt, C.c_void_p(d_in) if d_in else None, int(n_in), int(bool(final)), int(n_bits),
                                                 sec[0], sec[1], sec[2], C.c_void_p(d_rows) if d_rows else None, int(row_bytes),
                                                 int(max_rows), res, C.c_void_p(stream) if stream else None), "tsim_shotdata_decode")
        return tuple(int(x) for x in res)


_codecs: dict = {}


def codec(device: int = 0) -> _Codec:
    c = _codecs.get(int(device))
    if c is None:
        c = _codecs[int(device)] = _Codec(int(device))
    return c


def _dets_sections(fmt: int, n_bits: int, sec: tuple) -> tuple:
    if fmt == 5 and sum(sec) != n_bits:
        raise ValueError(f"dets needs num_measurements + num_detectors + num_observables = {n_bits} columns, got {sec}")
    return sec if fmt == 5 else (0, 0, 0)


def encode_rows_device(d_rows: int, n: int, *, row_bytes: int, n_bits: int, format: str, d_out: int, out_capacity: int,
                       num_measurements: int = 0, num_detectors: int = 0, num_observables: int = 0, device: int = 0,
                       stream: int = 0) -> int:
    """``n`` bit-packed device rows (``row_bytes`` apart, ``n_bits`` columns) in ``format`` at ``d_out``.  Returns the
    encoded size; when it exceeds ``out_capacity`` nothing is written (grow the buffer and call again).  Asynchronous on
    ``stream`` (0: the codec's own) once the size is known."""
    fmt = check_format(format)
    sec = _dets_sections(fmt, int(n_bits), check_sections(num_measurements, num_detectors, num_observables))
    if int(n) < 0 or int(n_bits) < 0 or int(row_bytes) < (int(n_bits) + 7) // 8:
        raise ValueError(f"bad shape: n={n}, n_bits={n_bits}, row_bytes={row_bytes}")
    if fmt == 3 and int(n) % 64:
        raise ValueError(f"ptb64 needs a multiple of 64 rows, got {n}")
    return codec(device).encode(fmt, int(d_rows), int(n), int(row_bytes), int(n_bits), sec, int(d_out), int(out_capacity), int(stream))


def decode_bytes_device(d_bytes: int, n_bytes: int, *, final: bool, n_bits: int, format: str, d_rows: int, row_bytes: int,
                        max_rows: int, num_measurements: int = 0, num_detectors: int = 0, num_observables: int = 0,
                        device: int = 0, stream: int = 0) -> tuple:
    """A chunk of a file (starting at a row boundary) in device memory -> at most ``max_rows`` rows at ``d_rows``.  Returns
    ``(rows, bytes_consumed, fault_offset, fault_kind)`` (offset -1: no fault)."""
    fmt = check_format(format)
    sec = _dets_sections(fmt, int(n_bits), check_sections(num_measurements, num_detectors, num_observables))
    if fmt in (1, 3) and int(n_bits) < 1:
        raise ValueError(f"{format} needs at least one column to be read")
    return codec(device).decode(fmt, int(d_bytes), int(n_bytes), bool(final), int(n_bits), sec, int(d_rows), int(row_bytes), int(max_rows),
                                int(stream))


# -- writing ----------------------------------------------------------------------------------------------------------
class ShotWriter:
    """Streams bit-packed device rows into a file: encode on the device in pieces of at most about :data:`CHUNK_BYTES`
    of ``01`` text (so device and pinned staging stay bounded whatever a call hands over), download into pinned staging,
    and write each piece to the file at the next call, while the device keeps working on later rows.  ``ptb64`` carries
    a partial group of 64 rows from call to call."""

    def __init__(self, path, format: str, n_bits: int, sections: tuple = (0, 0, 0), *, device: int = 0):
        self.fmt = check_format(format)
        self.n_bits = int(n_bits)
        self.sec = _dets_sections(self.fmt, self.n_bits, check_sections(*sections))
        self.used = (self.n_bits + 7) // 8
        self.c = codec(device)
        self.path = os.fspath(path)
        self.bytes_written = 0
        self._piece = max(64, (max(1, int(CHUNK_BYTES)) // (self.n_bits + 1)) // 64 * 64)  # rows encoded at a time
        self._slots = []
        self._f = None
        try:
            self._slots = [self.c.take_slot() for _ in range(2)]  # the encoded bytes, the ptb64 carry
            self._cap = 0
            self._pending = None
            self._carry = 0
            self._f = open(self.path, "wb")
        except BaseException:
            self._release()
            raise

    def _release(self) -> None:
        for s in self._slots:
            self.c.give_slot(s)
        self._slots = []

    def _flush(self, stream: int) -> None:
        """Wait for the pending download and write it to the file."""
        if self._pending is not None:
            ptr, n, s = self._pending
            self.c.sync(s)
            self._pending = None
            if n:
                self._f.write(memoryview((C.c_uint8 * n).from_address(ptr)))
                self.bytes_written += n

    def _emit(self, d_rows: int, n: int, row_bytes: int, stream: int) -> None:
        for r0 in range(0, n, self._piece):
            self._emit_piece(d_rows + r0 * row_bytes, min(self._piece, n - r0), row_bytes, stream)

    def _emit_piece(self, d_rows: int, n: int, row_bytes: int, stream: int) -> None:
        self._flush(stream)  # (the staging below is free again)
        slot = self._slots[0]
        d_out = self.c.staging(slot, self._cap, pinned=False) if self._cap else 0
        nbytes = self.c.encode(self.fmt, d_rows, n, row_bytes, self.n_bits, self.sec, d_out, self._cap, stream)
        if nbytes > self._cap:
            self._cap = max(nbytes, 2 * self._cap)
            d_out = self.c.staging(slot, self._cap, pinned=False)
            nbytes = self.c.encode(self.fmt, d_rows, n, row_bytes, self.n_bits, self.sec, d_out, self._cap, stream)
        host = self.c.staging(slot, nbytes, pinned=True)
        self.c.copy(host, d_out, nbytes, stream)
        self._pending = (host, nbytes, stream)

    def write_device(self, d_rows: int, n: int, row_bytes: int, stream: int = 0) -> None:
        """``n`` rows at ``d_rows`` (``row_bytes`` apart), valid in the order of ``stream``; they may be overwritten once
        the stream has passed this call's work."""
        n = int(n)
        if self.fmt != 3:
            self._emit(d_rows, n, row_bytes, stream)
            return
        if n and self.used and row_bytes != self.used:
            raise ValueError("ptb64 rows must be packed (row_bytes == ceil(n_bits / 8))")
        carry = self.c.staging(self._slots[1], 64 * self.used, pinned=False)
        a = 0
        if self._carry:
            t = min(64 - self._carry, n)
            self.c.copy(carry + self._carry * self.used, d_rows, t * self.used, stream)
            self._carry += t
            a = t
            if self._carry == 64:
                self._emit(carry, 64, self.used, stream)
                self._carry = 0
        whole = (n - a) // 64 * 64
        self._emit(d_rows + a * row_bytes, whole, row_bytes, stream)
        a += whole
        if a < n:  # (the carry was empty here; work that still reads it comes earlier on the same stream)
            self.c.copy(carry, d_rows + a * row_bytes, (n - a) * self.used, stream)
            self._carry = n - a

    def write_packed(self, packed: np.ndarray) -> None:
        """Host rows, ``uint8[rows, ceil(n_bits/8)]`` with zero pad bits, through the device codec."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        rows = packed.shape[0]
        step = max(64, (CHUNK_BYTES // max(1, self.used)) // 64 * 64)
        up = self.c.take_slot()
        try:
            for r0 in range(0, rows, step):
                part = packed[r0:r0 + step]
                nb = part.nbytes
                d_in = self.c.staging(up, nb, pinned=False)
                self._flush(0)  # (the upload buffers are free once the previous encode has run)
                h_in = self.c.staging(up, nb, pinned=True)
                if nb:
                    C.memmove(h_in, part.ctypes.data, nb)
                self.c.copy(d_in, h_in, nb)
                self.write_device(d_in, len(part), self.used)
        finally:
            self._flush(0)
            self.c.give_slot(up)

    def close(self) -> None:
        try:
            if self._f is not None:
                self._flush(0)
                self.c.sync(0)
                if self._carry:
                    raise ValueError(f"ptb64 needs a multiple of 64 shots: {self._carry} rows are left over")
        finally:
            if self._f is not None:
                self._f.close()
                self._f = None
            self._release()

    def abort(self) -> None:
        """Close without flushing (an error happened upstream)."""
        try:
            self.c.sync(0)
        except Exception:  # noqa: BLE001 - the original error matters more
            pass
        if self._f is not None:
            self._f.close()
            self._f = None
        self._release()


def close_all(writers) -> None:
    """Close every writer, even when one of them raises; the first error is raised once all are closed."""
    err = None
    for w in writers:
        try:
            w.close()
        except BaseException as exc:  # noqa: BLE001 - re-raised below, after the other writers are closed
            err = err or exc
    if err is not None:
        raise err


def _as_packed(data, n_bits_hint=None) -> tuple:
    """``(packed uint8 rows, n_bits)`` of bool rows or of bit-packed uint8 rows."""
    a = np.asarray(data)
    if a.ndim != 2:
        raise ValueError(f"data must be 2-D [shots, columns], got shape {a.shape}")
    if a.dtype == np.bool_:
        return np.packbits(a.view(np.uint8), axis=1, bitorder="little"), a.shape[1]
    if a.dtype == np.uint8:
        if n_bits_hint is None:
            return a, 8 * a.shape[1]
        n = int(n_bits_hint)
        if a.shape[1] != (n + 7) // 8:
            raise ValueError(f"bit-packed data must have {(n + 7) // 8} bytes per row for {n} columns, got {a.shape[1]}")
        out = np.ascontiguousarray(a).copy()
        if n % 8 and out.shape[1]:
            out[:, -1] &= (1 << (n % 8)) - 1
        return out, n
    raise ValueError(f"data must be bool (one column per bit) or uint8 (bit-packed), got {a.dtype}")


def write_shot_data_file(*, data, path, format: str, num_measurements: int = 0, num_detectors: int = 0, num_observables: int = 0,
                         device: int = 0) -> None:
    """stim's ``write_shot_data_file``: bool ``data`` has one column per bit; uint8 ``data`` is bit-packed with ``ceil(n/8)``
    bytes per row, ``n`` = the sum of the section sizes when one is given, else ``8 * bytes``."""
    fmt = check_format(format)
    sec = check_sections(num_measurements, num_detectors, num_observables)
    a = np.asarray(data)
    if a.dtype not in (np.bool_, np.uint8):
        raise ValueError(f"data must be bool (one column per bit) or uint8 (bit-packed), got {a.dtype}")
    packed, n_bits = _as_packed(a, sum(sec) if (a.dtype == np.uint8 and sum(sec)) else None)
    if sum(sec) and sum(sec) != n_bits:
        raise ValueError(f"data has {n_bits} columns, the sections {sec} add up to {sum(sec)}")
    if fmt == 5 and sum(sec) != n_bits:
        raise ValueError(f"dets needs num_measurements + num_detectors + num_observables = {n_bits} columns, got {sec}")
    if fmt == 3 and packed.shape[0] % 64:
        raise ValueError(f"ptb64 needs a multiple of 64 shots, got {packed.shape[0]}")
    w = ShotWriter(path, format, n_bits, sec if fmt == 5 else (0, 0, 0), device=device)
    try:
        w.write_packed(packed)
    except BaseException:
        w.abort()
        raise
    w.close()


# -- reading ----------------------------------------------------------------------------------------------------------
def _row_bound(fmt: int, n_in: int, n_bits: int) -> int:
    """Most rows a chunk of n_in bytes can hold."""
    if fmt == 0:
        return n_in // (n_bits + 1) + 1
    if fmt == 1:
        return n_in // max(1, (n_bits + 7) // 8)
    if fmt == 3:
        return 64 * (n_in // (8 * n_bits))
    if fmt == 5:
        return n_in // 5 + 1
    return n_in + 1


def iter_device_rows(path, format: str, n_bits: int, sections: tuple = (0, 0, 0), *, device: int = 0, row_bytes: int | None = None):
    """Decode a file chunk by chunk; yields ``(d_rows, rows, row_bytes)`` - device rows valid until the next step."""
    fmt = check_format(format)
    n_bits = int(n_bits)
    sec = _dets_sections(fmt, n_bits, sections)
    used = (n_bits + 7) // 8
    rb = used if row_bytes is None else int(row_bytes)
    if fmt in (1, 3) and n_bits < 1:
        raise ValueError(f"{format} needs at least one column to be read")
    c = codec(device)
    path = os.fspath(path)
    size = os.path.getsize(path)
    slots = [c.take_slot() for _ in range(2)]
    try:
        with open(path, "rb") as f:
            pos = 0  # file offset of the chunk's first byte
            carry = b""
            chunk = max(1, int(CHUNK_BYTES))
            while True:
                want = max(chunk - len(carry), 1)
                fresh = f.read(want)
                buf = carry + fresh
                n_in = len(buf)
                final = pos + n_in >= size
                if n_in == 0:
                    return
                h_in = c.staging(slots[0], n_in, pinned=True)
                C.memmove(h_in, buf, n_in)
                d_in = c.staging(slots[0], n_in, pinned=False)
                c.copy(d_in, h_in, n_in)
                off = 0
                while off < n_in:
                    bound = _row_bound(fmt, n_in - off, n_bits)
                    max_rows = bound if rb == 0 else max(1, min(bound, ROW_BUFFER_BYTES // rb))
                    if fmt == 3:
                        max_rows = max(64, max_rows // 64 * 64)
                    d_rows = c.staging(slots[1], max_rows * rb, pinned=False)
                    rows, used_bytes, fault, kind = c.decode(fmt, d_in + off, n_in - off, final, n_bits, sec, d_rows, rb, max_rows)
                    if fault >= 0:
                        raise ValueError(f"{path}: {_FAULTS.get(kind, 'fault')} at byte offset {pos + off + fault} ({format} format)")
                    if rows == 0:
                        break
                    yield d_rows, rows, rb
                    off += used_bytes
                if final:
                    if off < n_in:  # (every fault is reported above; kept as a guard)
                        raise ValueError(f"{path}: the file ends inside a row at byte offset {size} ({format} format)")
                    return
                carry = buf[off:]
                pos += off
                if off == 0:
                    chunk *= 2  # a row longer than the chunk
    finally:
        for s in slots:
            c.give_slot(s)


def read_shot_data_file(*, path, format: str, bit_packed: bool = False, num_measurements: int = 0, num_detectors: int = 0,
                        num_observables: int = 0, device: int = 0) -> np.ndarray:
    """stim's ``read_shot_data_file``: rows of ``num_measurements + num_detectors + num_observables`` columns, as bools or
    (``bit_packed=True``) ``uint8[rows, ceil(n/8)]`` with zero pad bits."""
    fmt = check_format(format)
    sec = check_sections(num_measurements, num_detectors, num_observables)
    n_bits = sum(sec)
    if fmt in (1, 3) and n_bits < 1:
        raise ValueError(f"{format} needs at least one column to be read")
    used = (n_bits + 7) // 8
    parts = []
    total = 0
    c = codec(device)
    for d_rows, rows, rb in iter_device_rows(path, format, n_bits, sec if fmt == 5 else (0, 0, 0), device=device):
        host = np.empty((rows, used), dtype=np.uint8)
        if host.nbytes:
            c.copy(host.ctypes.data, d_rows, host.nbytes)
        c.sync()
        parts.append(host)
        total += rows
    packed = np.concatenate(parts, axis=0) if parts else np.zeros((0, used), np.uint8)
    if bit_packed:
        return packed
    return np.unpackbits(packed, axis=1, count=n_bits, bitorder="little").view(np.bool_) if n_bits else np.zeros((total, 0), np.bool_)


# -- the samplers' sink ------------------------------------------------------------------------------------------------
class FileSink:
    """``sample_write``: the rows a sampler path hands over (padded device rows of ``in_words`` uint64, request rows
    ``[lo, hi)`` of its row space) arranged per file with ``tsim_arrange_rows_device`` (column list, reference flips in
    bit 31) and streamed into that file's :class:`ShotWriter`."""

    def __init__(self, hp, in_words: int, files: list, *, lo: int, hi: int):
        self.hp, self.wo, self.lo, self.hi = hp, int(in_words), int(lo), int(hi)
        self.files = []  # (writer, n_cols, device column table)
        self._bufs = []
        self._arr = [None] * len(files)
        try:
            for writer, cols in files:
                cols = np.ascontiguousarray(cols, dtype=np.uint32)
                d_cols = None
                if len(cols):
                    d_cols = hp.malloc(cols.nbytes + 16)
                    self._bufs.append(d_cols)
                    hp.h2d(d_cols, cols)
                self.files.append((writer, len(cols), d_cols))
        except BaseException:
            self.release()
            raise

    def _arranged(self, k: int, nbytes: int, stream: int):
        have = self._arr[k]
        if have is None or have.nbytes < nbytes:
            if have is not None:  # the previous call's encode may still read it on the sink's stream
                self.hp.stream_synchronize(stream)
                have.free()
            self._arr[k] = have = self.hp.malloc(max(64, nbytes) + 16)
        return have

    def __call__(self, d_first: int, row_bytes: int, r0: int, r1: int, stream: int = 0) -> None:
        a, b = max(r0, self.lo), min(r1, self.hi)
        if b <= a:
            return
        src = d_first + (a - r0) * row_bytes
        for k, (writer, n_cols, d_cols) in enumerate(self.files):
            nb = (n_cols + 7) // 8
            if n_cols == 0:
                writer.write_device(src, b - a, 0, stream)
                continue
            dst = self._arranged(k, (b - a) * nb, stream)
            self.hp.arrange_rows_device(src, b - a, self.wo, d_cols.ptr, n_cols, True, dst.ptr, stream=stream)
            writer.write_device(dst.ptr, b - a, nb, stream)

    def release(self) -> None:
        for buf in self._bufs + [x for x in self._arr if x is not None]:
            buf.free()
        self._bufs = []
        self._arr = [None] * len(self._arr)
