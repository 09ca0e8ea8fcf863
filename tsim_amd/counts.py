"""Counts instead of rows: kept shots, observable flips, per-column counts and a histogram, reduced on the GPU.

``CompiledDetectorSampler.count()`` / ``CompiledMeasurementSampler.count()`` run the batches ``sample()`` would run and
hand the finished rows, still in HBM, to the tally kernel (``tsim_tally_rows_device``, ``csrc/tsim_tally.hip.h``)
instead of downloading them: only the counters cross PCIe.  The results are exact integers; for a fresh sampler with
the same seed and arguments they are the numpy tally (:func:`tally_rows`) of what ``sample()`` returns, and the key
chains stand where ``sample()`` would leave them.

``pair_columns`` adds the second-order statistic: ``pair_counts[a, b]``, the kept shots with columns ``pair_columns[a]``
and ``pair_columns[b]`` both set (a binary ``X^T X`` by the pair kernels, ``tsim_pairs_*``, ``csrc/tsim_pairs.hip.h``), and
:meth:`ShotCounts.pair_correlations`, the p_ij estimator computed from it.

:func:`tally_rows_device` / :func:`tally_pairs_device` / :func:`tally_patterns_device` run the kernels on device rows the
caller owns (``m2d`` output, ``sample_steps_device`` rows).

``pattern_columns`` adds the joint statistic: the distinct patterns of the kept shots over those columns, each with its
exact count (the row table, ``tsim_rowtab_*``, ``csrc/tsim_rowtab.hip.h``) - what ``np.unique(sample(), axis=0)`` gives
without the rows crossing PCIe.  ``decoder`` (:class:`tsim_amd.decode.LookupDecoder`, a table of syndromes, or
:class:`tsim_amd.decode.UnionFindDecoder`, cluster growth on the circuit's decoding graph, ``tsim_uf_*``, or
:class:`tsim_amd.decode.WindowedUnionFindDecoder`, the same window after window for long runs, ``tsim_ufw_*``, with heralded
erasures too when the decoder has ``heralds=True``; ``uf.with_cluster_matching()`` and, on a graph with heralds,
``uf.with_erasure_matching()`` are union-find decoders that match small clusters) is applied to every kept shot where it lies,
and the wrong predictions are counted.  ``corrected=True`` goes one step further: the predictions are XORed into the observable columns of the rows in HBM
(``tsim_pred_rows_device``, ``csrc/tsim_predrows.hip.h``) before anything is counted, so the column counts, the histogram, the
pair counts and the patterns are those of the corrected rows - per-observable logical error rates and the joint law of the
residual flips.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib

__all__ = ["ShotCounts", "tally_rows", "tally_rows_device", "tally_pairs_device", "tally_patterns_device", "counters_length",
           "check_pair_columns", "check_pattern_columns", "pair_correlations_from_moments", "MAX_HISTOGRAM_COLUMNS",
           "MAX_PAIR_COLUMNS", "DEFAULT_PATTERN_CAPACITY"]

MAX_HISTOGRAM_COLUMNS = 16
MAX_PAIR_COLUMNS = 4096
DEFAULT_PATTERN_CAPACITY = 1 << 20


@dataclass(frozen=True, eq=False)
class ShotCounts:
    """Counts over the kept shots of a request.  ``column_counts[c]``: kept shots with column ``c`` set (detectors, then
    observables); ``histogram[b]``: kept shots whose bits at ``histogram_columns`` spell ``b`` (bit ``i`` = column
    ``histogram_columns[i]``; no columns: one bin, ``kept``).  ``pair_counts[a, b]`` (int64, symmetric; ``None`` when no
    ``pair_columns`` were asked for): kept shots with columns ``pair_columns[a]`` and ``pair_columns[b]`` both set - its
    diagonal is ``column_counts[list(pair_columns)]``.  ``patterns`` (bool ``[D, k]``, columns in the order of
    ``pattern_columns``) and ``pattern_counts`` (int64 ``[D]``; both ``None`` when no ``pattern_columns`` were asked for):
    the distinct patterns of the kept shots over ``pattern_columns`` and how often each occurred, ordered by count
    descending, ties by the bit-packed (little-endian) pattern bytes ascending; ``pattern_overflow``: kept shots whose
    pattern found no room (``sum(pattern_counts) + pattern_overflow == kept``; the patterns present are exact).
    ``decoded_errors`` / ``decoder_misses`` (``None`` without a decoder): kept shots whose observables differ from the
    decoder's prediction, and kept shots whose syndrome the decoder does not know (it predicts no flip for them).
    ``soft_output`` (``None`` unless the decoder is a ``UnionFindDecoder.with_soft_output(metric, bins)``, a
    ``WindowedUnionFindDecoder.with_soft_output(metric, bins)``, whose values combine over its windows, or a cluster-matching
    one ``with_gap_output(...)``, whose metric is ``"gap"`` and whose value is the deficit ``(gap_cap - gap) // gap_step``): the metric's name;
    then ``soft_kept[b]`` (int64 ``[bins]``) are the kept shots whose metric falls into bin ``b = min(value, bins - 1)`` and
    ``soft_errors[b]`` those of them that count in ``decoded_errors`` (``soft_kept.sum() == kept``,
    ``soft_errors.sum() == decoded_errors``); :meth:`rejection_curve` sums them up.  ``corrected`` (``count(decoder=...,
    corrected=True)``): every kept shot's prediction was XORed into its observables before anything was counted, so
    ``observable_counts[k]`` are the kept shots in which observable ``k`` is still flipped after decoding, ``histogram``,
    ``pair_counts`` and ``patterns`` are over the corrected rows and ``kept_with_observable_flip == decoded_errors``; ``kept``,
    ``detector_counts`` and the decoder's own counts are what they are without it."""

    shots: int
    kept: int
    kept_with_observable_flip: int
    column_counts: np.ndarray
    num_detectors: int
    histogram_columns: tuple
    histogram: np.ndarray
    pair_columns: tuple = ()
    pair_counts: np.ndarray | None = None
    pattern_columns: tuple = ()
    patterns: np.ndarray | None = None
    pattern_counts: np.ndarray | None = None
    pattern_overflow: int = 0
    decoded_errors: int | None = None
    decoder_misses: int | None = None
    soft_output: str | None = None
    soft_kept: np.ndarray | None = None
    soft_errors: np.ndarray | None = None
    corrected: bool = False

    @property
    def detector_counts(self) -> np.ndarray:
        return self.column_counts[: self.num_detectors]

    @property
    def observable_counts(self) -> np.ndarray:
        return self.column_counts[self.num_detectors:]

    @property
    def kept_fraction(self) -> float:
        return self.kept / self.shots if self.shots else math.nan

    def __eq__(self, other) -> bool:
        if not isinstance(other, ShotCounts):
            return NotImplemented
        return (self.shots == other.shots and self.kept == other.kept
                and self.kept_with_observable_flip == other.kept_with_observable_flip
                and self.num_detectors == other.num_detectors and tuple(self.histogram_columns) == tuple(other.histogram_columns)
                and np.array_equal(self.column_counts, other.column_counts) and np.array_equal(self.histogram, other.histogram)
                and tuple(self.pair_columns) == tuple(other.pair_columns)
                and (self.pair_counts is None) == (other.pair_counts is None)
                and (self.pair_counts is None or np.array_equal(self.pair_counts, other.pair_counts))
                and tuple(self.pattern_columns) == tuple(other.pattern_columns)
                and (self.patterns is None) == (other.patterns is None)
                and (self.patterns is None or (np.array_equal(self.patterns, other.patterns)
                                               and np.array_equal(self.pattern_counts, other.pattern_counts)))
                and self.pattern_overflow == other.pattern_overflow
                and self.decoded_errors == other.decoded_errors and self.decoder_misses == other.decoder_misses
                # ("no soft output" is any false value: callers that build counts from the fields in front of the soft ones,
                # positionally, hand the last field's False to soft_output since `corrected` was appended)
                and (self.soft_output or None) == (other.soft_output or None)
                and (self.soft_kept is None) == (other.soft_kept is None)
                and (self.soft_kept is None or np.array_equal(self.soft_kept, other.soft_kept))
                and (self.soft_errors is None) == (other.soft_errors is None)
                and (self.soft_errors is None or np.array_equal(self.soft_errors, other.soft_errors))
                and bool(self.corrected) == bool(other.corrected))

    def pair_correlations(self) -> np.ndarray:
        """The float64 ``[k, k]`` matrix of the p_ij estimator over ``pair_columns`` (diagonal NaN):
        :func:`pair_correlations_from_moments` of ``pair_counts / kept``."""
        if self.pair_counts is None:
            raise ValueError("no pair counts: ask count() for pair_columns")
        n = np.asarray(self.pair_counts, dtype=np.float64)
        if self.kept == 0:
            return np.full(n.shape, np.nan)
        return pair_correlations_from_moments(np.diagonal(n) / self.kept, n / self.kept)

    def rejection_curve(self):
        """``(accepted int64[bins], errors int64[bins])``: entry ``t`` is what is left when the shots of a bin above ``t`` are
        discarded - the kept shots of the bins ``0 .. t`` and the decoded errors among them (the running sums of ``soft_kept``
        and ``soft_errors``; the last entry is ``(kept, decoded_errors)``)."""
        if self.soft_output is None or self.soft_kept is None or self.soft_errors is None:
            raise ValueError("no soft output: give count() a UnionFindDecoder.with_soft_output(metric, bins)")
        return np.cumsum(np.asarray(self.soft_kept, dtype=np.int64)), np.cumsum(np.asarray(self.soft_errors, dtype=np.int64))

    __hash__ = None

    @classmethod
    def from_counters(cls, counters: np.ndarray, *, shots: int, n_cols: int, num_detectors: int, histogram_columns=()) -> "ShotCounts":
        """The counters of :func:`tally_rows_device` (``counters_length(n_cols, k)`` uint64) as counts."""
        c = np.asarray(counters).astype(np.int64)
        hc = tuple(int(x) for x in histogram_columns)
        if c.shape != (counters_length(n_cols, len(hc)),):
            raise ValueError(f"counters must have {counters_length(n_cols, len(hc))} entries, got shape {c.shape}")
        return cls(int(shots), int(c[0]), int(c[1]), c[2:2 + n_cols].copy(), int(num_detectors), hc, c[2 + n_cols:].copy())


def counters_length(n_cols: int, n_hist: int) -> int:
    """uint64 entries of the counter buffer of :func:`tally_rows_device`: kept, kept with an observable, the columns, the bins."""
    return 2 + int(n_cols) + (1 << int(n_hist))


def check_histogram_columns(columns, n_cols: int) -> tuple:
    """Distinct column indices ``0 <= c < n_cols``, at most 16 of them, as a tuple of ints (raises ``ValueError``)."""
    cols = np.asarray(list(columns) if not isinstance(columns, np.ndarray) else columns)
    if cols.ndim != 1 or (cols.size and not np.issubdtype(cols.dtype, np.integer)):
        raise ValueError("histogram_columns must be a sequence of column indices")
    if cols.size > MAX_HISTOGRAM_COLUMNS:
        raise ValueError(f"at most {MAX_HISTOGRAM_COLUMNS} histogram columns, got {cols.size}")
    if cols.size and (cols.min() < 0 or cols.max() >= n_cols):
        raise ValueError(f"histogram columns must lie in 0 .. {n_cols - 1}, got {cols.tolist()}")
    if len(set(cols.tolist())) != cols.size:
        raise ValueError(f"histogram columns must be distinct, got {cols.tolist()}")
    return tuple(int(c) for c in cols)


def check_pair_columns(columns, n_cols: int, num_detectors: int) -> tuple:
    """The selection of ``count(pair_columns=...)`` as a tuple of ints: ``None`` / ``()`` (none), ``"all"`` (every column),
    ``"detectors"`` (columns ``0 .. num_detectors - 1``) or a sequence of distinct indices ``0 <= c < n_cols`` in any
    order; at most 4096 (raises ``ValueError``)."""
    if columns is None:
        return ()
    if isinstance(columns, str):
        if columns not in ("all", "detectors"):
            raise ValueError(f'pair_columns must be "all", "detectors" or a sequence of column indices, got {columns!r}')
        count = int(n_cols) if columns == "all" else int(num_detectors)
        if count > MAX_PAIR_COLUMNS:
            raise ValueError(f"at most {MAX_PAIR_COLUMNS} pair columns, got {count}")
        return tuple(range(count))
    cols = np.asarray(list(columns) if not isinstance(columns, np.ndarray) else columns)
    if cols.ndim != 1 or (cols.size and not np.issubdtype(cols.dtype, np.integer)):
        raise ValueError("pair_columns must be a sequence of column indices")
    if cols.size > MAX_PAIR_COLUMNS:
        raise ValueError(f"at most {MAX_PAIR_COLUMNS} pair columns, got {cols.size}")
    if cols.size and (cols.min() < 0 or cols.max() >= n_cols):
        raise ValueError(f"pair columns must lie in 0 .. {n_cols - 1}, got {cols.tolist()}")
    if len(set(cols.tolist())) != cols.size:
        raise ValueError(f"pair columns must be distinct, got {cols.tolist()}")
    return tuple(int(c) for c in cols)


def check_pattern_columns(columns, n_cols: int, num_detectors: int) -> tuple:
    """The selection of ``count(pattern_columns=...)`` as a tuple of ints: ``None`` / ``()`` (none), ``"all"`` (every
    column), ``"detectors"`` (columns ``0 .. num_detectors - 1``) or a sequence of distinct indices ``0 <= c < n_cols`` in
    any order, as many as there are columns (raises ``ValueError``)."""
    if columns is None:
        return ()
    if isinstance(columns, str):
        if columns not in ("all", "detectors"):
            raise ValueError(f'pattern_columns must be "all", "detectors" or a sequence of column indices, got {columns!r}')
        return tuple(range(int(n_cols) if columns == "all" else int(num_detectors)))
    cols = np.asarray(list(columns) if not isinstance(columns, np.ndarray) else columns)
    if cols.ndim != 1 or (cols.size and not np.issubdtype(cols.dtype, np.integer)):
        raise ValueError("pattern_columns must be a sequence of column indices")
    if cols.size and (cols.min() < 0 or cols.max() >= n_cols):
        raise ValueError(f"pattern columns must lie in 0 .. {n_cols - 1}, got {cols.tolist()}")
    if len(set(cols.tolist())) != cols.size:
        raise ValueError(f"pattern columns must be distinct, got {cols.tolist()}")
    return tuple(int(c) for c in cols)


def check_pattern_capacity(capacity) -> int | None:
    if capacity is None:
        return None
    if int(capacity) != capacity or not 1 <= int(capacity) <= 1 << 30:
        raise ValueError(f"pattern_capacity must be an integer in 1 .. 2^30, got {capacity!r}")
    return int(capacity)


def ordered_patterns(keys: np.ndarray, counts: np.ndarray, k: int):
    """Bit-packed patterns ``uint8[D, ceil(k/8)]`` with their counts -> ``(bool[D, k], int64[D])`` in the order of
    :class:`ShotCounts`: count descending, ties by the packed bytes ascending."""
    keys = np.asarray(keys, dtype=np.uint8).reshape(len(counts), (k + 7) // 8)
    counts = np.asarray(counts).astype(np.int64)
    order = np.lexsort(tuple(keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)) + (-counts,))
    bits = np.unpackbits(keys[order], axis=1, bitorder="little", count=k).astype(np.bool_)
    return bits.reshape(len(counts), k), counts[order]


def warn_pattern_overflow(counts: "ShotCounts", capacity) -> "ShotCounts":
    if counts.pattern_overflow > 0:
        import warnings

        warnings.warn(f"count(): {counts.pattern_overflow} kept shots carry a pattern that found no room in a table of "
                      f"pattern_capacity={capacity} (the {len(counts.pattern_counts)} patterns returned are exact); raise "
                      "pattern_capacity", RuntimeWarning, stacklevel=3)
    return counts


def pair_correlations_from_moments(x, xx) -> np.ndarray:
    """The standard p_ij estimator from first moments ``x[i] = <x_i>`` and second moments ``xx[i, j] = <x_i x_j>``:
    ``p_ij = 1/2 - sqrt(1/4 - (xx_ij - x_i x_j) / (1 - 2 (x_i + x_j - 2 xx_ij)))``.  For two detectors that share one
    error mechanism of probability ``p`` and otherwise see independent errors it is ``p`` on the exact moments.  NaN on
    the diagonal and where the denominator or the radicand is not positive."""
    x = np.asarray(x, dtype=np.float64)
    xx = np.asarray(xx, dtype=np.float64)
    if x.ndim != 1 or xx.shape != (x.size, x.size):
        raise ValueError(f"moments of shapes {x.shape} and {xx.shape}: expected [k] and [k, k]")
    xi, xj = x[:, None], x[None, :]
    den = 1.0 - 2.0 * (xi + xj - 2.0 * xx)
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = 0.25 - (xx - xi * xj) / np.where(den > 0, den, np.nan)
        p = 0.5 - np.sqrt(np.where(rad > 0, rad, np.nan))
    p[np.arange(x.size), np.arange(x.size)] = np.nan
    return p


def default_histogram_columns(num_detectors: int, n_cols: int) -> tuple:
    """The observables when there are 1 .. 16 of them, else none."""
    n_obs = n_cols - num_detectors
    return tuple(range(num_detectors, n_cols)) if 1 <= n_obs <= MAX_HISTOGRAM_COLUMNS else ()


class _HostTally:
    """The numpy statement of the tally, accumulated batch by batch (memory O(columns + bins))."""

    def __init__(self, n_cols: int, num_detectors: int, postselection_mask, histogram_columns, pair_columns=(), pattern_columns=(),
                 pattern_capacity=None, decoder=None, corrected: bool = False):
        self.n_cols, self.nd = int(n_cols), int(num_detectors)
        self.corrected = check_corrected(corrected, decoder)
        self.tc, self.tcap = tuple(pattern_columns), pattern_capacity
        self.table = {}          # packed pattern bytes -> rows, in the order of first appearance
        self.overflow = 0
        self.decoder = decoder
        self.errors = self.misses = 0
        self.soft = _soft_choice(decoder)   # (metric, bins) of a union-find decoder with_soft_output (whole or windowed), or None
        self.soft_hist = np.zeros((2, self.soft[1]), dtype=np.int64) if self.soft else None
        self.pc = tuple(pair_columns)
        self.pairs = np.zeros((len(self.pc), len(self.pc)), dtype=np.int64) if self.pc else None
        self.mask = None if postselection_mask is None else np.asarray(postselection_mask, dtype=np.bool_)
        self.hc = tuple(histogram_columns)
        self.shots = self.kept = self.kept_obs = 0
        self.cols = np.zeros(self.n_cols, dtype=np.int64)
        self.hist = np.zeros(1 << len(self.hc), dtype=np.int64)

    def add(self, rows: np.ndarray) -> None:
        rows = np.asarray(rows, dtype=np.bool_).reshape(-1, self.n_cols)
        self.shots += len(rows)
        if self.mask is not None:
            rows = rows[~(rows[:, : self.nd] & self.mask).any(axis=1)]
        self.kept += len(rows)
        if self.decoder is not None and len(rows):
            dets, obs = rows[:, : self.nd], rows[:, self.nd:]
            pred = self.decoder.decode(dets)
            wrong = (pred != obs).any(axis=1)
            self.errors += int(wrong.sum())
            self.misses += int(self.decoder.missed(dets).sum())
            if self.soft:
                kept, errors = self.decoder.soft_bin_counts(dets, wrong)
                self.soft_hist[0] += kept
                self.soft_hist[1] += errors
            if self.corrected:  # everything below counts the corrected rows (a copy: the caller's rows stay)
                rows = np.concatenate([dets, obs ^ pred], axis=1)
        self.kept_obs += int(rows[:, self.nd:].any(axis=1).sum())
        self.cols += rows.sum(axis=0, dtype=np.int64)
        idx = np.zeros(len(rows), dtype=np.int64)
        for i, c in enumerate(self.hc):
            idx |= rows[:, c].astype(np.int64) << i
        self.hist += np.bincount(idx, minlength=len(self.hist))
        if self.pc:  # (float64 products of 0/1 are exact below 2^53 rows; BLAS does not multiply integers)
            sel = rows[:, list(self.pc)].astype(np.float64)
            self.pairs += np.rint(sel.T @ sel).astype(np.int64)
        if self.tc and len(rows):
            packed = np.packbits(rows[:, list(self.tc)], axis=1, bitorder="little")
            uniq, first, cnt = np.unique(packed, axis=0, return_index=True, return_counts=True)
            for i in np.argsort(first, kind="stable"):  # (a capacity admits patterns in the order of first appearance)
                key = uniq[i].tobytes()
                if key in self.table:
                    self.table[key] += int(cnt[i])
                elif self.tcap is None or len(self.table) < self.tcap:
                    self.table[key] = int(cnt[i])
                else:
                    self.overflow += int(cnt[i])

    def result(self) -> ShotCounts:
        patterns = pattern_counts = None
        if self.tc:
            kb = (len(self.tc) + 7) // 8
            keys = np.frombuffer(b"".join(self.table), dtype=np.uint8).reshape(len(self.table), kb)
            patterns, pattern_counts = ordered_patterns(keys, np.fromiter(self.table.values(), np.int64, len(self.table)), len(self.tc))
        return ShotCounts(self.shots, self.kept, self.kept_obs, self.cols.copy(), self.nd, self.hc, self.hist.copy(), self.pc,
                          None if self.pairs is None else self.pairs.copy(), self.tc, patterns, pattern_counts, self.overflow,
                          None if self.decoder is None else self.errors, None if self.decoder is None else self.misses,
                          *((self.soft[0], self.soft_hist[0].copy(), self.soft_hist[1].copy()) if self.soft else ()),
                          corrected=self.corrected)


def tally_rows(rows, *, num_detectors: int, postselection_mask=None, histogram_columns=(), pair_columns=(), pattern_columns=(),
               pattern_capacity=None, decoder=None, corrected: bool = False) -> ShotCounts:
    """The tally of boolean rows (detectors, then observables) in numpy: a row is kept iff no masked detector is set; the
    column counts, ``kept_with_observable_flip`` (a set observable), the histogram and the pair counts over
    ``pair_columns`` (:func:`check_pair_columns`) are taken over the kept rows.  ``pattern_columns``
    (:func:`check_pattern_columns`): the distinct patterns of the kept rows (``np.unique``) with their counts, in the order
    of :class:`ShotCounts`; ``pattern_capacity`` (default: no limit) admits that many patterns in the order of first
    appearance and counts the rows of the others in ``pattern_overflow``.  ``decoder``: a
    :class:`tsim_amd.decode.LookupDecoder`, :class:`tsim_amd.decode.UnionFindDecoder` or
    :class:`tsim_amd.decode.WindowedUnionFindDecoder` applied to the kept rows; a union-find decoder with a soft output
    (``with_soft_output``, whole or windowed) also fills ``soft_kept`` / ``soft_errors``, from its ``soft_outputs()``.  ``corrected``
    (needs a decoder): every kept row gets ``obs ^= decoder.decode(dets)`` before anything but the decoder's own counts is
    taken (:class:`ShotCounts`); ``rows`` itself is not changed."""
    rows = np.asarray(rows, dtype=np.bool_)
    if rows.ndim != 2:
        raise ValueError(f"rows must be 2-D, got shape {rows.shape}")
    n_cols = rows.shape[1]
    if not 0 <= num_detectors <= n_cols:
        raise ValueError(f"num_detectors={num_detectors} of {n_cols} columns")
    if postselection_mask is not None and np.asarray(postselection_mask).shape != (num_detectors,):
        raise ValueError(f"postselection_mask must have shape ({num_detectors},), got {np.asarray(postselection_mask).shape}")
    t = _HostTally(n_cols, num_detectors, postselection_mask, check_histogram_columns(histogram_columns, n_cols),
                   check_pair_columns(pair_columns, n_cols, num_detectors),
                   check_pattern_columns(pattern_columns, n_cols, num_detectors), check_pattern_capacity(pattern_capacity),
                   check_decoder(decoder, n_cols, num_detectors), corrected)
    t.add(rows)
    return t.result()


def _soft_choice(decoder):
    """``(metric, bins)`` of a :class:`tsim_amd.decode.UnionFindDecoder` or :class:`tsim_amd.decode.WindowedUnionFindDecoder`
    that carries a soft output, else ``None``."""
    from .decode import UnionFindDecoder, WindowedUnionFindDecoder

    if isinstance(decoder, (UnionFindDecoder, WindowedUnionFindDecoder)) and decoder.soft_output is not None:
        return decoder.soft_output, int(decoder.soft_bins)
    return None


def check_decoder(decoder, n_cols: int, num_detectors: int):
    """``decoder`` (or ``None``) when it fits rows of ``num_detectors`` detectors and ``n_cols - num_detectors`` observables."""
    if decoder is None:
        return None
    if (decoder.num_detectors, decoder.num_observables) != (int(num_detectors), int(n_cols) - int(num_detectors)):
        raise ValueError(f"the decoder is for {decoder.num_detectors} detectors and {decoder.num_observables} observables, the rows "
                         f"have {num_detectors} and {int(n_cols) - int(num_detectors)}")
    if decoder.num_detectors < 1:
        raise ValueError("a decoder needs at least one detector")
    return decoder


def check_corrected(corrected, decoder) -> bool:
    """``corrected`` as a bool; ``ValueError`` when it is asked for without a decoder."""
    if corrected and decoder is None:
        raise ValueError("corrected=True needs a decoder: the predictions are what is XORed into the observables")
    return bool(corrected)


def tally_rows_device(d_rows: int, n: int, *, row_bytes: int, n_cols: int, d_counts: int, d_xor: int = 0, d_test: int = 0,
                      observables: tuple = (0, 0), histogram_columns=(), device: int = 0, stream: int = 0) -> None:
    """Counts over ``n`` bit-packed device rows (``row_bytes`` apart, ``n_cols`` columns, little-endian), ACCUMULATED into
    the caller's ``uint64[counters_length(n_cols, len(histogram_columns))]`` at ``d_counts`` - read them back with
    :meth:`ShotCounts.from_counters`.  ``d_xor`` / ``d_test``: optional device rows of ``ceil(n_cols/8)`` bytes (XORed into
    every row; a row is kept iff ``(row ^ xor) & test == 0``); ``observables``: the column range ``[lo, hi)`` of
    ``kept_with_observable_flip``.  Asynchronous on ``stream`` (0: the null stream) of ``device``."""
    n, n_cols = int(n), int(n_cols)
    if n < 0:
        raise ValueError(f"n must be non-negative, got {n}")
    if n_cols < 1:
        raise ValueError(f"n_cols must be at least 1, got {n_cols}")
    if int(row_bytes) < (n_cols + 7) // 8:
        raise ValueError(f"rows of {row_bytes} bytes cannot hold {n_cols} columns")
    lo, hi = (int(x) for x in observables)
    if not 0 <= lo <= hi <= n_cols:
        raise ValueError(f"observables {lo} .. {hi} of {n_cols} columns")
    hc = np.asarray(check_histogram_columns(histogram_columns, n_cols), dtype=np.int32)
    if n == 0:
        return
    _lib.check(_lib.load().tsim_tally_rows_device(int(device), C.c_void_p(int(d_rows)), n, int(row_bytes), n_cols,
                                                  C.c_void_p(int(d_xor)) if d_xor else None,
                                                  C.c_void_p(int(d_test)) if d_test else None, lo, hi,
                                                  _lib.ptr(hc) if hc.size else None, int(hc.size), C.c_void_p(int(d_counts)),
                                                  C.c_void_p(int(stream)) if stream else None),
               "tsim_tally_rows_device")


def tally_pairs_device(d_rows: int, n: int, *, row_bytes: int, n_cols: int, pair_columns, d_xor: int = 0, d_test: int = 0,
                       device: int = 0, stream: int = 0) -> np.ndarray:
    """Pair counts over ``n`` bit-packed device rows the caller owns (laid out as for :func:`tally_rows_device`, ``d_xor`` /
    ``d_test`` meaning the same): the symmetric int64 ``[k, k]`` matrix over ``pair_columns`` (distinct indices, at most
    4096).  Runs on ``stream`` (0: the null stream) of ``device`` and returns when the counts are on the host."""
    n, n_cols = int(n), int(n_cols)
    if n < 0:
        raise ValueError(f"n must be non-negative, got {n}")
    if n_cols < 1:
        raise ValueError(f"n_cols must be at least 1, got {n_cols}")
    if int(row_bytes) < (n_cols + 7) // 8:
        raise ValueError(f"rows of {row_bytes} bytes cannot hold {n_cols} columns")
    pc = np.asarray(check_pair_columns(pair_columns, n_cols, n_cols), dtype=np.int32)
    if pc.size == 0:
        raise ValueError("pair_columns is empty")
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.tsim_pairs_create(int(device), n_cols, _lib.ptr(pc), int(pc.size), C.byref(h)), "tsim_pairs_create")
    try:
        st = C.c_void_p(int(stream)) if stream else None
        _lib.check(lib.tsim_pairs_add_device(h, C.c_void_p(int(d_rows)), n, int(row_bytes), C.c_void_p(int(d_xor)) if d_xor else None,
                                             C.c_void_p(int(d_test)) if d_test else None, st), "tsim_pairs_add_device")
        out = np.zeros((pc.size, pc.size), dtype=np.uint64)
        _lib.check(lib.tsim_pairs_read(h, _lib.ptr(out), st), "tsim_pairs_read")
    finally:
        lib.tsim_pairs_destroy(h)
    return out.astype(np.int64)


def tally_patterns_device(d_rows: int, n: int, *, row_bytes: int, n_cols: int, pattern_columns, capacity: int = DEFAULT_PATTERN_CAPACITY,
                          d_xor: int = 0, d_test: int = 0, device: int = 0, stream: int = 0):
    """Pattern counts over ``n`` bit-packed device rows the caller owns (laid out as for :func:`tally_rows_device`, ``d_xor`` /
    ``d_test`` meaning the same): ``(patterns bool[D, k], counts int64[D], overflow)`` over ``pattern_columns`` (distinct
    indices, any number), ordered as in :class:`ShotCounts`, from a table of ``capacity`` slots.  Runs on ``stream`` (0: the
    null stream) of ``device`` and returns when the entries are on the host."""
    n, n_cols = int(n), int(n_cols)
    if n < 0:
        raise ValueError(f"n must be non-negative, got {n}")
    if n_cols < 1:
        raise ValueError(f"n_cols must be at least 1, got {n_cols}")
    if int(row_bytes) < (n_cols + 7) // 8:
        raise ValueError(f"rows of {row_bytes} bytes cannot hold {n_cols} columns")
    tc = np.asarray(check_pattern_columns(pattern_columns, n_cols, n_cols), dtype=np.int32)
    if tc.size == 0:
        raise ValueError("pattern_columns is empty")
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.tsim_rowtab_create(int(device), n_cols, _lib.ptr(tc), int(tc.size), check_pattern_capacity(capacity), C.byref(h)),
               "tsim_rowtab_create")
    try:
        st = C.c_void_p(int(stream)) if stream else None
        _lib.check(lib.tsim_rowtab_add_device(h, C.c_void_p(int(d_rows)), n, int(row_bytes), C.c_void_p(int(d_xor)) if d_xor else None,
                                              C.c_void_p(int(d_test)) if d_test else None, st), "tsim_rowtab_add_device")
        keys, counts, info = rowtab_read(lib, h, int(tc.size), st)
    finally:
        lib.tsim_rowtab_destroy(h)
    return ordered_patterns(keys, counts, int(tc.size)) + (int(info[4]),)


def rowtab_read(lib, handle, n_key: int, stream):
    """``(keys uint8[D, ceil(n_key/8)], counts uint64[D], info int64[8])`` of a row table (``tsim_rowtab_info``, ``tsim_rowtab_read``)."""
    info = (C.c_int64 * 8)()
    _lib.check(lib.tsim_rowtab_info(handle, info), "tsim_rowtab_info")
    entries = int(info[1])
    keys = np.zeros((entries, (int(n_key) + 7) // 8), dtype=np.uint8)
    counts = np.zeros(entries, dtype=np.uint64)
    got = C.c_int64()
    _lib.check(lib.tsim_rowtab_read(handle, _lib.ptr(keys), _lib.ptr(counts), entries, C.byref(got), stream), "tsim_rowtab_read")
    return keys, counts, np.array(list(info), dtype=np.int64)


class _DeviceTally:
    """The counters of one ``count()`` on a program's device, the masks in the layout of its rows, and the shot range
    ``[lo, hi)`` of the rows handed to it that belong to the request (a reference row riding in front, padding behind)."""

    def __init__(self, hp, n_cols: int, num_detectors: int, *, xor_bits=None, test_bits=None, histogram_columns=(), lo: int = 0,
                 hi: int = 0, pair_columns=(), pattern_columns=(), pattern_capacity=None, decoder=None, corrected: bool = False):
        self.hp, self.n_cols, self.nd, self.hc = hp, int(n_cols), int(num_detectors), tuple(histogram_columns)
        self.corrected = check_corrected(corrected, decoder)
        self._d_pred = None      # corrected: the predictions of one call's rows, uint64[_d_pred_rows], grown on demand
        self._d_pred_rows = 0
        self.lo, self.hi = int(lo), int(hi)
        self.pc = tuple(pair_columns)
        self.tc = tuple(pattern_columns)
        self.decoder = decoder
        self._bufs = []
        self._pairs = None       # the pair counter's handle (tsim_pairs), when pair columns are asked for
        self._pairs_stream = 0   # the stream its launches went to
        self._table = None       # the row table's handle (tsim_rowtab), when pattern columns are asked for
        self._dec = None         # the decoder's (handle, what decodes rows by it, what destroys it): a row table loaded from the
        #                          host (a LookupDecoder), a tsim_uf (a UnionFindDecoder) or a tsim_ufw (a WindowedUnionFindDecoder)
        self.d_decoded = None    # its three counters
        self.soft = _soft_choice(decoder)   # (metric, bins): the union-find decoder's soft output (whole or windowed), binned on the device
        self.d_soft_hist = None  # its two histograms, uint64[2 * bins]
        try:
            if self.pc:
                self._pairs = hp.pairs_create(self.n_cols, self.pc)
            if self.tc:
                self._table = hp.rowtab_create(self.n_cols, self.tc, pattern_capacity or DEFAULT_PATTERN_CAPACITY)
            if decoder is not None:
                self._dec = decoder._handle(hp, self.n_cols)
                self.d_decoded = self._upload(np.zeros(3, dtype=np.uint64))
                if self.soft:
                    self.d_soft_hist = self._upload(np.zeros(2 * self.soft[1], dtype=np.uint64))
                    self._dec = (self._dec[0], decoder._soft_call(hp, self.d_soft_hist.ptr), self._dec[2])
            self.d_counts = self._upload(np.zeros(counters_length(self.n_cols, len(self.hc)), dtype=np.uint64))
            self.d_xor = self._upload(self._row(xor_bits)) if xor_bits is not None and np.any(xor_bits) else None
            self.d_test = self._upload(self._row(test_bits)) if test_bits is not None else None
        except BaseException:
            self.release()
            raise

    def _row(self, bits) -> np.ndarray:
        full = np.zeros(self.n_cols, dtype=np.uint8)
        b = np.asarray(bits, dtype=np.uint8)
        full[: len(b)] = b
        return np.packbits(full, bitorder="little")

    def _upload(self, a: np.ndarray):
        buf = self.hp.malloc(a.nbytes + 16)
        self._bufs.append(buf)
        self.hp.h2d(buf, a)
        return buf

    def __call__(self, d_first: int, row_bytes: int, r0: int, r1: int, stream: int = 0) -> None:
        """Rows ``r0 .. r1 - 1`` of the request's row space, row ``r0`` at device address ``d_first``."""
        a, b = max(r0, self.lo), min(r1, self.hi)
        if b <= a:
            return
        if self.corrected:
            # decode first, then XOR every prediction into its row's raw observables: the readers below, on the same stream, see
            # corrected rows and apply the xor mask themselves (the rows are the sampler's output and are not read again)
            d_pred = self._pred_room(b - a)
            self._pairs_stream = stream
            self._decode(d_first + (a - r0) * row_bytes, b - a, row_bytes, stream, d_pred=d_pred)
            if self.n_cols > self.nd:
                self.hp.pred_rows_device(self._d_pred.ptr, b - a, self.n_cols - self.nd, d_first + (a - r0) * row_bytes, row_bytes, self.nd,
                                         "xor", stream=stream)
        self.hp.tally_rows_device(d_first + (a - r0) * row_bytes, b - a, row_bytes, self.n_cols, self.d_counts.ptr,
                                  d_xor=self.d_xor.ptr if self.d_xor is not None else 0,
                                  d_test=self.d_test.ptr if self.d_test is not None else 0,
                                  observables=(self.nd, self.n_cols), histogram_columns=self.hc, stream=stream)
        if self._pairs is not None:
            self._pairs_stream = stream
            self.hp.pairs_add_device(self._pairs, d_first + (a - r0) * row_bytes, b - a, row_bytes,
                                     d_xor=self.d_xor.ptr if self.d_xor is not None else 0,
                                     d_test=self.d_test.ptr if self.d_test is not None else 0, stream=stream)
        if self._table is not None or self._dec is not None:
            self._pairs_stream = stream
            masks = dict(d_xor=self.d_xor.ptr if self.d_xor is not None else 0, d_test=self.d_test.ptr if self.d_test is not None else 0,
                         stream=stream)
            if self._table is not None:
                self.hp.rowtab_add_device(self._table, d_first + (a - r0) * row_bytes, b - a, row_bytes, **masks)
            if self._dec is not None and not self.corrected:
                self._dec[1](self._dec[0], d_first + (a - r0) * row_bytes, b - a, row_bytes, (self.nd, self.n_cols), self.d_decoded.ptr, **masks)

    def _decode(self, d_rows: int, n: int, row_bytes: int, stream: int, d_pred: int) -> None:
        """``corrected``: the decoder's call with an outlet for the predictions (it writes every row's, 0 for a row that is not kept)."""
        self._dec[1](self._dec[0], d_rows, n, row_bytes, (self.nd, self.n_cols), self.d_decoded.ptr, d_pred=d_pred,
                     d_xor=self.d_xor.ptr if self.d_xor is not None else 0, d_test=self.d_test.ptr if self.d_test is not None else 0,
                     stream=stream)

    def _pred_room(self, n: int) -> int:
        """The scratch buffer of the predictions, for ``n`` rows at least."""
        if self._d_pred_rows < n:
            if self._d_pred is not None:  # (the launches of the call before may still use it)
                self.hp.stream_synchronize(self._pairs_stream)
                self._d_pred.free()
                self._d_pred, self._d_pred_rows = None, 0
            self._d_pred = self.hp.malloc(8 * n + 16)
            self._d_pred_rows = n
        return self._d_pred.ptr

    def result(self, shots: int) -> ShotCounts:
        """The counters, once every tally launch has completed (the caller has synchronised their streams)."""
        c = np.zeros(counters_length(self.n_cols, len(self.hc)), dtype=np.uint64)
        self.hp.d2h(c, self.d_counts)
        out = ShotCounts.from_counters(c, shots=shots, n_cols=self.n_cols, num_detectors=self.nd, histogram_columns=self.hc)
        if self._pairs is None and self._table is None and self._dec is None:
            return out
        pairs = self.hp.pairs_read(self._pairs, len(self.pc), stream=self._pairs_stream) if self._pairs is not None else None
        patterns = pattern_counts = errors = misses = None
        overflow = 0
        if self._table is not None:
            keys, cnt, info = self.hp.rowtab_read(self._table, len(self.tc), stream=self._pairs_stream)
            patterns, pattern_counts = ordered_patterns(keys, cnt, len(self.tc))
            overflow = int(info[4])
        if self._dec is not None:
            self.hp.stream_synchronize(self._pairs_stream)
            d = np.zeros(3, dtype=np.uint64)
            self.hp.d2h(d, self.d_decoded)
            errors, misses = int(d[1]), int(d[2])
        soft = ()
        if self.soft:
            hist = np.zeros(2 * self.soft[1], dtype=np.uint64)
            self.hp.d2h(hist, self.d_soft_hist)
            hist = hist.astype(np.int64)
            soft = (self.soft[0], hist[:self.soft[1]].copy(), hist[self.soft[1]:].copy())
        return ShotCounts(out.shots, out.kept, out.kept_with_observable_flip, out.column_counts, out.num_detectors,
                          out.histogram_columns, out.histogram, self.pc, pairs, self.tc, patterns, pattern_counts, overflow,
                          errors, misses, *soft, corrected=self.corrected)

    def release(self) -> None:
        if self._d_pred is not None:
            self._d_pred.free()
            self._d_pred, self._d_pred_rows = None, 0
        if self._table is not None:
            self.hp.rowtab_destroy(self._table)
            self._table = None
        if self._dec is not None:
            self._dec[2](self._dec[0])
            self._dec = None
        if self._pairs is not None:
            self.hp.pairs_destroy(self._pairs)
            self._pairs = None
        for buf in self._bufs:
            buf.free()
        self._bufs = []
