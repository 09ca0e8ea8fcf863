"""The numpy statement of stim's six shot-data formats (test helper, not part of the library): ``encode(format, rows)``
turns bool rows into file bytes, ``decode(format, data, n)`` turns file bytes back into bool rows."""

from __future__ import annotations

import numpy as np

FORMATS = ("01", "b8", "r8", "ptb64", "hits", "dets")


def _prefixes(n: int, sections) -> list:
    nm, nd, no = sections if sections is not None else (0, n, 0)
    assert nm + nd + no == n
    return [("M", c) for c in range(nm)] + [("D", c) for c in range(nd)] + [("L", c) for c in range(no)]


def encode(format: str, rows, sections=None) -> bytes:
    rows = np.asarray(rows, dtype=np.bool_)
    B, n = rows.shape
    if format == "01":
        return b"".join(b"".join(b"1" if x else b"0" for x in r) + b"\n" for r in rows)
    if format == "b8":
        return np.packbits(rows.view(np.uint8), axis=1, bitorder="little").tobytes()
    if format == "r8":
        out = bytearray()
        for r in rows:
            prev = -1
            for c in list(np.flatnonzero(r)) + [n]:
                gap = int(c) - prev - 1
                out += b"\xff" * (gap // 255) + bytes([gap % 255])
                prev = int(c)
        return bytes(out)
    if format == "ptb64":
        assert B % 64 == 0
        out = bytearray()
        for g in range(B // 64):
            blk = rows[64 * g:64 * g + 64]
            for c in range(n):
                out += int(sum(1 << s for s in range(64) if blk[s, c])).to_bytes(8, "little")
        return bytes(out)
    if format == "hits":
        return b"".join((",".join(str(int(c)) for c in np.flatnonzero(r)) + "\n").encode() for r in rows)
    if format == "dets":
        pre = _prefixes(n, sections)
        return b"".join(("shot" + "".join(f" {pre[c][0]}{pre[c][1]}" for c in np.flatnonzero(r)) + "\n").encode() for r in rows)
    raise ValueError(format)


def decode(format: str, data: bytes, n: int, sections=None) -> np.ndarray:
    """Bytes -> bool rows (well-formed input only; the GPU decoders' faults are tested separately)."""
    if format == "b8":
        nb = (n + 7) // 8
        a = np.frombuffer(data, dtype=np.uint8).reshape(-1, nb)
        return np.unpackbits(a, axis=1, count=n, bitorder="little").astype(np.bool_)
    if format == "ptb64":
        w = np.frombuffer(data, dtype="<u8").reshape(-1, n)
        rows = np.zeros((64 * len(w), n), dtype=np.bool_)
        for g in range(len(w)):
            for s in range(64):
                rows[64 * g + s] = (w[g] >> np.uint64(s)) & np.uint64(1)
        return rows
    if format == "r8":
        out, row, pos = [], np.zeros(n, np.bool_), 0
        for b in data:
            pos += b
            if b == 255:
                continue
            if pos == n:
                out.append(row)
                row, pos = np.zeros(n, np.bool_), 0
            else:
                row[pos] = True
                pos += 1
        assert pos == 0
        return np.array(out, dtype=np.bool_).reshape(-1, n)
    text = data.decode()
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines = lines[:-1]
    rows = np.zeros((len(lines), n), dtype=np.bool_)
    if format == "01":
        for i, ln in enumerate(lines):
            assert len(ln) == n
            rows[i] = [ch == "1" for ch in ln]
        return rows
    if format == "hits":
        for i, ln in enumerate(lines):
            for t in ln.split(",") if ln else []:
                rows[i, int(t)] = True
        return rows
    if format == "dets":
        nm, nd, _no = sections if sections is not None else (0, n, 0)
        base = {"M": 0, "D": nm, "L": nm + nd}
        for i, ln in enumerate(lines):
            toks = ln.split()
            assert toks[0] == "shot"
            for t in toks[1:]:
                rows[i, base[t[0]] + int(t[1:])] = True
        return rows
    raise ValueError(format)
