"""A maximum-likelihood lookup-table decoder, built from pattern counts and applied where the shots are.

``train = sampler.count(N, pattern_columns="all")`` returns which (detectors, observables) patterns occurred and how
often; :meth:`LookupDecoder.from_counts` keeps, per detector pattern (syndrome), the observable pattern seen most often.
``sampler.count(M, decoder=dec)`` then looks every kept shot's syndrome up on the GPU (a row table loaded from the host,
``tsim_rowtab_load`` / ``tsim_rowtab_decode_device``, ``csrc/tsim_rowtab.hip.h``) and counts the shots whose observables
differ from the prediction (``ShotCounts.decoded_errors``) and those whose syndrome is unknown
(``ShotCounts.decoder_misses``); :meth:`LookupDecoder.decode` / :meth:`LookupDecoder.missed` are the same in numpy.
"""

from __future__ import annotations

import numpy as np

__all__ = ["LookupDecoder"]


def _pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(np.asarray(bits, dtype=np.bool_), axis=1, bitorder="little")


def _as_uint64(bits: np.ndarray) -> np.ndarray:
    """bool ``[n, k]`` (``k <= 64``) -> uint64 ``[n]``, bit ``i`` = column ``i``."""
    out = np.zeros((len(bits), 8), dtype=np.uint8)
    p = _pack(bits)
    out[:, : p.shape[1]] = p
    return out.view("<u8").reshape(len(bits))


class LookupDecoder:
    """``syndromes`` bool ``[D, num_detectors]`` (distinct rows) with ``predictions`` bool ``[D, num_observables]``
    (at most 64 observables): a shot with syndrome ``syndromes[i]`` is predicted to have flipped ``predictions[i]``; a
    syndrome that is not listed predicts no flip."""

    def __init__(self, syndromes, predictions):
        s = np.asarray(syndromes, dtype=np.bool_)
        p = np.asarray(predictions, dtype=np.bool_)
        if s.ndim != 2 or p.ndim != 2 or len(s) != len(p):
            raise ValueError(f"syndromes [D, nd] and predictions [D, n_obs] expected, got shapes {s.shape} and {p.shape}")
        if p.shape[1] > 64:
            raise ValueError(f"at most 64 observables, got {p.shape[1]}")
        self.syndromes, self.predictions = s.copy(), p.copy()
        self._keys = _pack(s).reshape(len(s), (s.shape[1] + 7) // 8)
        self._index = {k.tobytes(): i for i, k in enumerate(self._keys)}
        if len(self._index) != len(s):
            raise ValueError("the syndromes must be distinct")

    @property
    def num_detectors(self) -> int:
        return self.syndromes.shape[1]

    @property
    def num_observables(self) -> int:
        return self.predictions.shape[1]

    def __len__(self) -> int:
        return len(self.syndromes)

    def table(self):
        """``(keys uint8[D, ceil(nd/8)], values uint64[D])``: the bit-packed syndromes and predictions (bit ``i`` = observable
        ``i``), as ``tsim_rowtab_load`` takes them."""
        return self._keys, _as_uint64(self.predictions)

    @classmethod
    def from_counts(cls, counts) -> "LookupDecoder":
        """From a ``ShotCounts`` whose ``pattern_columns`` are all the detectors followed by all the observables
        (``count(N, pattern_columns="all")``): per syndrome the observable pattern with the largest count, a tie going to
        the smaller packed value (bit ``i`` = observable ``i``)."""
        n_cols, nd = len(counts.column_counts), int(counts.num_detectors)
        if counts.patterns is None or tuple(counts.pattern_columns) != tuple(range(n_cols)):
            raise ValueError('the counts must carry the patterns over every column: count(..., pattern_columns="all")')
        if n_cols - nd > 64:
            raise ValueError(f"at most 64 observables, got {n_cols - nd}")
        pat, cnt = np.asarray(counts.patterns, dtype=np.bool_), np.asarray(counts.pattern_counts, dtype=np.int64)
        if len(pat) == 0:
            return cls(np.zeros((0, nd), np.bool_), np.zeros((0, n_cols - nd), np.bool_))
        uniq, inv = np.unique(_pack(pat[:, :nd]).reshape(len(pat), (nd + 7) // 8), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        val = _as_uint64(pat[:, nd:])
        order = np.lexsort((val, -cnt, inv))  # per syndrome: the largest count first, then the smaller value
        first = order[np.concatenate([[True], inv[order][1:] != inv[order][:-1]])]
        return cls(pat[first, :nd], pat[first, nd:])

    def _lookup(self, dets) -> np.ndarray:
        """The entry of each row's syndrome, -1 for an unknown one."""
        d = np.asarray(dets, dtype=np.bool_)
        if d.ndim != 2 or d.shape[1] != self.num_detectors:
            raise ValueError(f"dets must be [n, {self.num_detectors}], got shape {d.shape}")
        if len(d) == 0:
            return np.zeros(0, dtype=np.int64)
        uniq, inv = np.unique(_pack(d).reshape(len(d), (d.shape[1] + 7) // 8), axis=0, return_inverse=True)
        idx = np.fromiter((self._index.get(k.tobytes(), -1) for k in uniq), np.int64, len(uniq))
        return idx[np.asarray(inv).reshape(-1)]

    def decode(self, dets) -> np.ndarray:
        """bool ``[n, num_observables]``: the predicted observable flips of detector rows bool ``[n, num_detectors]``."""
        idx = self._lookup(dets)
        out = np.zeros((len(idx), self.num_observables), dtype=np.bool_)
        out[idx >= 0] = self.predictions[idx[idx >= 0]]
        return out

    def missed(self, dets) -> np.ndarray:
        """bool ``[n]``: the rows whose syndrome is not in the table."""
        return self._lookup(dets) < 0
