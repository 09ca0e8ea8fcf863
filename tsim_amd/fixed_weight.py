"""Fixed-weight fault sampling (``CliffordCircuit.compile_detector_sampler(method="faults", fault_weight=k)``) and the
stratified logical error rate built on it (:func:`stratified_error_rate`).

At small ``p`` almost every shot of :mod:`tsim_amd.faults` is a row without a fault, which a decoder gets right; the shots
that can fail need several faults and are a vanishing share of the stream.  Here a shot is drawn CONDITIONED on exactly ``k``
noise sites firing; the failure fraction ``f_k`` of each weight is estimated on its own and the weights are put together with
their exact law, ``p_L = sum_k P(K = k) f_k``.

The law (float64 on the host)
-----------------------------
For a :class:`tsim_amd.faults.FaultForm`, class ``c`` has ``n_c`` sites of fire probability ``p_c = 1 - probs[0]`` of its
table (as ``build_form`` computes it) and odds ``o_c = p_c / (1 - p_c)``; a class with ``p_c = 1`` has no odds and is refused.
The WEIGHT ``K`` of a shot is the number of sites that fire: ``P(K = k) = prod_c (1 - p_c)^{n_c} E_0(k)``, where ``E_c(r)`` is
the coefficient of ``x^r`` in ``prod_{c' >= c} (1 + o_c' x)^{n_c'}``.  Conditioned on ``K = k`` the class counts ``(k_c)``
have probability proportional to ``prod_c C(n_c, k_c) o_c^{k_c}``, the firing set of a class is uniform over its
``k_c``-subsets, and every firing site takes its outcome from the class table as in :mod:`tsim_amd.faults`.

* :func:`weight_law`: ``P(K = k)`` for ``k = 0 .. kmax`` and the tail ``P(K > kmax)``, the tail summed from the coefficients
  beyond ``kmax`` (``1 - sum`` cancels when the tail is small).
* :func:`split_thresholds`: ``uint32[n_classes, kmax + 1, kmax + 1]``.  Row ``(c, r)`` is ``ceil(cdf 2^32)`` (at most
  ``2^32 - 1``) of ``P(k_c = m | r sites still to place in the classes c, c + 1, ...) = C(n_c, m) o_c^m E_{c+1}(r - m) /
  E_c(r)``; entries from the largest feasible ``m = min(r, n_c)`` upward are ``2^32 - 1``.  The draw ``x0`` picks the
  smallest ``m`` with ``x0 < thr[m]``, the largest feasible ``m`` when there is none (the convention of the outcome tables).
  An infeasible ``m`` (more than the class has, or leaving more than the later classes can take) has probability exactly 0,
  hence threshold 0 below the feasible range, and is never picked.  A row depends on ``(c, r)`` only: the table of ``kmax``
  serves every ``k <= kmax``.  A row no split can reach (``r`` beyond the sites of the classes ``c ..``) is all ``2^32 - 1``.
  Everything is computed with logarithms (``log C(n, m) o^m`` as a sum of ``m`` logarithms, coefficients by log-sum-exp), so
  that ``n_c`` up to ``2^25`` and ``p_c`` down to ``1e-9`` or up to ``1 - 1e-16`` neither overflow nor underflow.
* ``MAX_FAULT_WEIGHT = 32``: the most sites a request may ask for (the fired-position list of the kernel).

The random stream (exact integer arithmetic; a function of the request key, the weight and the global shot index ``g`` only)
-----------------------------------------------------------------------------------------------------------------------------
``(n0, n1) = threefry2x32(key, WEIGHT_COUNTER)`` is the noise key of the request - a stream of its own - and class ``c`` draws
under ``faults.class_key((n0, n1), c)`` with the counters of :mod:`tsim_amd.faults`: draw ``j`` of shot ``g`` is
``threefry2x32(key_c, (g mod 2^32, (g >> 32) | (j << 6)))``.  With ``r = k`` at the start, the classes in order:

* draw ``j = 0``: ``x0`` picks ``k_c`` from row ``(c, r)`` of the split table; the last class takes ``k_c = r`` without a
  draw.  Then ``r -= k_c``.
* draws ``j = 1, 2, ...`` give ``(x0, x1)``: ``t = x0 n_c`` (64 bits), ``pos = t >> 32``, ``lo = t mod 2^32``.  The draw is
  REJECTED when ``lo < 2^32 mod n_c`` (Lemire's rule: every position keeps exactly ``floor(2^32 / n_c)`` values of ``x0``) and
  when ``pos`` already fired in this shot and class.  Otherwise site ``pos`` of the class fires with the first outcome whose
  threshold exceeds ``x1`` (the last one when none does).  The class is done when ``k_c`` sites have fired.

:func:`fixed_weight_rows_host` is the numpy statement: the sampler's path without a device and the oracle of the GPU tests.
The kernel is ``csrc/tsim_faults_weight.hip.h`` behind ``tsim_faults_set_split`` / ``tsim_faults_sample_weight_device`` of
the ``tsim_faults`` handle.

Limits.  Stratifying by the total weight pays when the mean number of firing sites is at most a few.  The d = 15 memory
circuit at p = 1e-3 has a mean of 19.4: nearly all of its law lies within ``MAX_FAULT_WEIGHT``, but spread over some thirty
weights none of which fails often, and nothing here helps.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, prng
from .affine import threefry2x32_np
from .faults import CompiledFaultDetectorSampler, FaultForm, FaultHandle, _rows_host, class_key

__all__ = ["MAX_FAULT_WEIGHT", "WEIGHT_COUNTER", "weight_law", "split_thresholds", "class_odds", "position_of", "noise_key",
           "fixed_weight_rows_host", "FixedWeightHandle", "CompiledFixedWeightDetectorSampler", "StratifiedRate", "combine",
           "stratified_error_rate"]

MAX_FAULT_WEIGHT = 32
WEIGHT_COUNTER = (0x6E6F6973, 0x66697877)  # "nois", "fixw"
_NEG = -np.inf


# ---- the law and its tables ---------------------------------------------------------------------------------------------

def class_odds(form: FaultForm):
    """``(n_c int64[n_classes], p_c float64[n_classes])``; a class with ``p_c = 1`` is refused."""
    n = np.diff(form.class_ptr).astype(np.int64)
    p = np.empty(form.n_classes, np.float64)
    for c in range(form.n_classes):
        probs = np.asarray(form.channel_probs[int(form.site_chan[form.class_ptr[c]])], dtype=np.float64)
        p[c] = 1.0 - float(probs[0])
        if not p[c] < 1.0:
            raise NotImplementedError(f"class {c} fires with probability 1: an always-firing site has no odds")
    return n, p


def _log_terms(n: int, p: float, K: int) -> np.ndarray:
    """``log(C(n, m) o^m)`` for ``m = 0 .. K`` (``-inf`` beyond ``n``): a running sum of ``log((n - i + 1) / i) + log o``."""
    m = np.arange(1, K + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(m <= n, np.log(np.maximum(n - m + 1.0, 0.0) / m) + (np.log(p) - np.log1p(-p)), _NEG)
    return np.concatenate([[0.0], np.cumsum(step)])


def _log_conv(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """``log`` of the product of two polynomials given by the logs of their coefficients, truncated to ``len(a)`` terms."""
    K = len(a)
    r, m = np.arange(K)[:, None], np.arange(K)[None, :]
    with np.errstate(invalid="ignore"):
        t = np.where(m <= r, a[m] + b[np.maximum(r - m, 0)], _NEG)
    return np.logaddexp.reduce(t, axis=1)


def _log_coefficients(n, p, K: int):
    """``lE[c][r] = log E_c(r)`` for ``c = 0 .. n_classes`` (the last: the empty product) and the terms ``la[c][m]``."""
    la = [_log_terms(int(n[c]), float(p[c]), K) for c in range(len(n))]
    lE = [None] * (len(n) + 1)
    lE[len(n)] = np.concatenate([[0.0], np.full(K, _NEG)])
    for c in range(len(n) - 1, -1, -1):
        lE[c] = _log_conv(la[c], lE[c + 1])
    return la, lE


def _check_kmax(kmax) -> int:
    if int(kmax) != kmax or not 0 <= int(kmax) <= MAX_FAULT_WEIGHT:
        raise ValueError(f"kmax = {kmax!r}: an integer in 0 .. {MAX_FAULT_WEIGHT}")
    return int(kmax)


def weight_law(form: FaultForm, kmax: int):
    """``(float64[kmax + 1], tail)``: ``P(K = k)`` for ``k = 0 .. kmax`` and ``P(K > kmax)`` (module docstring).  The tail is
    the sum of the coefficients beyond ``kmax``, taken until they no longer count; when the mass of the law lies so far up
    that they never fall off in reach, ``P(K <= kmax) < 1e-30`` and ``1 - sum`` is exact."""
    kmax = _check_kmax(kmax)
    n, p = class_odds(form)
    log_p0 = float(np.sum(n * np.log1p(-p)))
    n_sites = int(n.sum())
    span = 64
    while True:
        K = min(n_sites, kmax + span)
        _, lE = _log_coefficients(n, p, max(K, kmax))
        law = np.exp(log_p0 + lE[0])
        beyond = law[kmax + 1:K + 1]
        tail = float(np.sum(np.sort(beyond))) if len(beyond) else 0.0
        if K == n_sites or (len(beyond) > 1 and beyond[-1] < beyond[-2] and beyond[-1] <= 1e-18 * tail):
            return law[:kmax + 1].copy(), tail
        head = float(law[:kmax + 1].sum())
        if head < 1e-30:
            return law[:kmax + 1].copy(), 1.0 - head
        span *= 2


def split_thresholds(form: FaultForm, kmax: int) -> np.ndarray:
    """``uint32[n_classes, kmax + 1, kmax + 1]``: the thresholds of the class counts (module docstring)."""
    kmax = _check_kmax(kmax)
    n, p = class_odds(form)
    la, lE = _log_coefficients(n, p, kmax)
    out = np.full((len(n), kmax + 1, kmax + 1), 0xFFFFFFFF, np.uint32)
    r, m = np.arange(kmax + 1)[:, None], np.arange(kmax + 1)[None, :]
    for c in range(len(n)):
        with np.errstate(invalid="ignore"):
            lp = np.where((m <= r) & np.isfinite(lE[c][r]), la[c][m] + lE[c + 1][np.maximum(r - m, 0)] - lE[c][r], _NEG)
        thr = np.minimum(np.ceil(np.minimum(np.cumsum(np.exp(lp), axis=1), 1.0) * 4294967296.0), 4294967295.0)
        keep = (m < np.minimum(r, int(n[c]))) & np.isfinite(lE[c][r])  # (from the largest feasible m upward: 2^32 - 1)
        out[c][keep] = thr[keep].astype(np.uint32)
    return out


def position_of(x0, n_c: int):
    """``(pos, accepted)`` of the draw ``x0`` in a class of ``n_c`` sites: ``t = x0 n_c``, ``pos = t >> 32``, accepted unless
    ``t mod 2^32 < 2^32 mod n_c``."""
    t = np.asarray(x0, dtype=np.uint64) * np.uint64(n_c)
    return (t >> np.uint64(32)).astype(np.int64), (t & np.uint64(0xFFFFFFFF)) >= np.uint64((1 << 32) % int(n_c))


def noise_key(key) -> tuple[int, int]:
    return prng.threefry2x32(int(key[0]), int(key[1]), *WEIGHT_COUNTER)


def _check_weight(form: FaultForm, k, kmax: int = MAX_FAULT_WEIGHT) -> int:
    if int(k) != k or int(k) < 0:
        raise ValueError(f"fault_weight = {k!r}: a non-negative integer")
    if int(k) > min(kmax, MAX_FAULT_WEIGHT):
        raise ValueError(f"fault_weight = {k} exceeds {min(kmax, MAX_FAULT_WEIGHT)} (MAX_FAULT_WEIGHT = {MAX_FAULT_WEIGHT})")
    if int(k) > form.n_sites:
        raise ValueError(f"fault_weight = {k} exceeds the {form.n_sites} noise sites of the circuit")
    return int(k)


# ---- the host statement -------------------------------------------------------------------------------------------------

def _fire(form: FaultForm, k: int, split: np.ndarray, nkey, g: np.ndarray):
    """The shots ``g`` (uint64) at weight ``k``: ``(shot index into g, error bit)`` of every error bit that fired."""
    c0, c1 = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32)
    r = np.full(len(g), k, np.int64)
    shots, bits = [], []
    for c in range(form.n_classes):
        s0, n_c = int(form.class_ptr[c]), int(form.class_ptr[c + 1] - form.class_ptr[c])
        lo, hi = int(form.table_ptr[c]), int(form.table_ptr[c + 1])
        vals, thr = form.out_vals[lo:hi], form.out_thr[lo:hi]
        e0 = form.site_e0[s0:s0 + n_c].astype(np.int64)
        k0, k1 = class_key(nkey, c)
        if c == form.n_classes - 1:
            k_c = r.copy()
        else:
            x0, _ = threefry2x32_np(k0, k1, c0, c1)
            rows = split[c][r]  # [shots, kmax + 1]
            k_c = np.minimum((rows <= x0[:, None]).sum(axis=1), np.minimum(r, n_c))  # (a row is non-decreasing)
        r = r - k_c
        fired = np.full((len(g), k), -1, np.int64)
        n_fired = np.zeros(len(g), np.int64)
        active = np.flatnonzero(n_fired < k_c)
        j = 1
        while len(active):
            x0, x1 = threefry2x32_np(k0, k1, c0[active], c1[active] | np.uint32((j << 6) & 0xFFFFFFFF))
            pos, ok = position_of(x0, n_c)
            ok &= ~(fired[active] == pos[:, None]).any(axis=1)
            who, pos = active[ok], pos[ok]
            fired[who, n_fired[who]] = pos
            n_fired[who] += 1
            o = vals[np.searchsorted(thr[:-1], x1[ok], side="right")]
            first = e0[pos]
            for b in range(int(form.table_bits[c])):
                sel = ((o >> np.uint32(b)) & np.uint32(1)).astype(np.bool_)
                shots.append(who[sel])
                bits.append(first[sel] + b)
            active = active[n_fired[active] < k_c[active]]
            j += 1
    if not shots:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(shots), np.concatenate(bits)


def fixed_weight_rows_host(form: FaultForm, k: int, first_shot: int, B: int, key, *, return_e: bool = False):
    """``uint8[B, n_out]`` (0/1): the outputs of the shots ``first_shot .. first_shot + B - 1`` (a multiple of 64 first) with
    exactly ``k`` noise sites fired, under the request key ``key``; ``return_e`` as in ``faults.fault_rows_host``."""
    k = _check_weight(form, k)
    split = split_thresholds(form, k)
    nkey = noise_key(key)
    return _rows_host(form, first_shot, B, lambda g: _fire(form, k, split, nkey, g), return_e)


# ---- the device handle --------------------------------------------------------------------------------------------------

class FixedWeightHandle(FaultHandle):
    """The ``tsim_faults`` handle with the split table of ``kmax`` uploaded; ``sample_device`` draws rows of ``self.weight``
    fired sites (any ``0 .. kmax``) through ``tsim_faults_sample_weight_device``."""

    WEIGHT_INFO = ("kmax", "waves", "lds_bytes", "tables_in_lds", "row_words", "window", "n_windows", "split_bytes")

    def __init__(self, form: FaultForm, kmax: int, *, weight: int | None = None, device: int = 0, pad_outputs: bool = False):
        super().__init__(form, device=device, pad_outputs=pad_outputs)
        self.kmax = _check_weight(form, kmax)
        self.weight = self.kmax if weight is None else _check_weight(form, weight, self.kmax)
        self._split = split_thresholds(form, self.kmax)

    def _handle(self):
        if self._h is None:
            h = super()._handle()
            try:
                _lib.check(_lib.load().tsim_faults_set_split(h, self.kmax, self._split.ctypes.data), "tsim_faults_set_split")
            except Exception:
                self.close()
                raise
        return self._h

    def weight_info(self) -> dict:
        return self._read_info("tsim_faults_weight_info", self.WEIGHT_INFO)

    def sample_device(self, B: int, d_out: int, *, key, first_shot: int = 0, out_row_bytes: int, out_packed: bool, col0: int = 0,
                      n_cols: int | None = None, stream: int = 0) -> None:
        """As ``FaultHandle.sample_device``; see ``tsim_faults_sample_weight_device`` in ``include/tsim_hip.h``."""
        self._request("tsim_faults_sample_weight_device", (int(self.weight),), B, d_out, key=key, first_shot=first_shot,
                      out_row_bytes=out_row_bytes, out_packed=out_packed, col0=col0, n_cols=n_cols, stream=stream)


# ---- the sampler --------------------------------------------------------------------------------------------------------

class CompiledFixedWeightDetectorSampler(CompiledFaultDetectorSampler):
    """The fault sampler conditioned on exactly ``fault_weight`` fired sites: ``sample()``, ``count()`` and
    ``sample_write()`` of the base class with every keyword, rows from this module's handle and statement.  ``kmax``: the
    split table to keep (default ``fault_weight``); :meth:`set_fault_weight` moves the weight inside ``0 .. kmax`` without a
    new handle."""

    def __init__(self, form: FaultForm, fault_weight: int, *, kmax: int | None = None, seed: int | None = None, device: int = 0,
                 noise: str = "host"):
        super().__init__(form, seed=seed, device=device, noise=noise)
        class_odds(form)
        self._kmax = _check_weight(form, fault_weight if kmax is None else kmax)
        self._weight = _check_weight(form, fault_weight, self._kmax)

    @property
    def fault_weight(self) -> int:
        return self._weight

    def set_fault_weight(self, k: int) -> None:
        self._weight = _check_weight(self._form, k, self._kmax)

    def weight_law(self, kmax: int | None = None):
        """:func:`weight_law` of the sampler's form (``kmax`` default: the sampler's own)."""
        return weight_law(self._form, self._kmax if kmax is None else kmax)

    def _frame_handle(self) -> FixedWeightHandle:
        if self._frame is None:
            self._frame = FixedWeightHandle(self._form, self._kmax, device=self._device, pad_outputs=True)
        self._frame.weight = self._weight
        return self._frame

    def _sample_direct(self, shots: int) -> np.ndarray:
        if self._direct_on_device(shots):
            return self._direct_device(shots, None)
        return fixed_weight_rows_host(self._form, self._weight, 0, shots, self._next_key()).view(np.bool_)

    def __repr__(self) -> str:
        return super().__repr__()[:-1] + f", exactly {self._weight} sites fire)"


# ---- the stratified logical error rate ----------------------------------------------------------------------------------

@dataclass
class StratifiedRate:
    """Per weight ``k = 0 .. kmax``: ``law[k] = P(K = k)``, ``shots[k]``, ``decoded_errors[k]``, ``decoder_misses[k]`` and
    ``f[k] = decoded_errors[k] / shots[k]``; ``estimate = sum law f``, ``std_error = sqrt(sum law^2 f (1 - f) / shots)`` and
    ``tail = P(K > kmax)``: the rate lies in ``[estimate, estimate + tail]``, up to sampling error."""

    law: np.ndarray
    shots: np.ndarray
    decoded_errors: np.ndarray
    decoder_misses: np.ndarray
    f: np.ndarray
    estimate: float
    std_error: float
    tail: float


def combine(law, tail: float, shots, wrong, misses=None) -> StratifiedRate:
    """The weights put together (a pure function): ``law`` and ``tail`` of :func:`weight_law`, per weight the shots taken and
    the shots decoded wrongly.  A weight without shots contributes nothing to the estimate; its ``f`` is 0."""
    law, shots, wrong = np.asarray(law, np.float64), np.asarray(shots, np.int64), np.asarray(wrong, np.int64)
    misses = np.zeros_like(wrong) if misses is None else np.asarray(misses, np.int64)
    if not law.shape == shots.shape == wrong.shape == misses.shape or law.ndim != 1:
        raise ValueError("law, shots, wrong (and misses) must be vectors of one length")
    if (shots < 0).any() or (wrong < 0).any() or (wrong > shots).any():
        raise ValueError("per weight 0 <= wrong <= shots")
    f = np.divide(wrong, shots, out=np.zeros(len(law)), where=shots > 0)
    var = np.divide(law * law * f * (1.0 - f), shots, out=np.zeros(len(law)), where=shots > 0)
    return StratifiedRate(law=law, shots=shots, decoded_errors=wrong, decoder_misses=misses, f=f, estimate=float(np.sum(law * f)),
                          std_error=float(np.sqrt(np.sum(var))), tail=float(tail))


def stratified_error_rate(circuit, decoder, shots: int, *, kmax: int, seed: int | None = None, device: int = 0,
                          postselection_mask=None) -> StratifiedRate:
    """The logical error rate of ``decoder`` on ``circuit`` (a :class:`tsim_amd.clifford.CliffordCircuit` or its text) by
    weight: ``count(shots, decoder=decoder)`` once per ``fault_weight = 0 .. kmax`` (at most the circuit's sites), on one
    form and one device handle, put together by :func:`combine`.  Post-selection is out of scope."""
    if postselection_mask is not None:
        raise ValueError("stratified_error_rate takes no post-selection mask: the weight law is that of all shots")
    if isinstance(circuit, str):
        from .clifford import CliffordCircuit

        circuit = CliffordCircuit(circuit)
    form = circuit.compile_faults()
    kmax = _check_weight(form, kmax)
    law, tail = weight_law(form, kmax)
    sampler = CompiledFixedWeightDetectorSampler(form, 0, kmax=kmax, seed=seed, device=device)
    wrong, misses = [], []
    for k in range(kmax + 1):
        sampler.set_fault_weight(k)
        got = sampler.count(shots, decoder=decoder)
        wrong.append(got.decoded_errors)
        misses.append(got.decoder_misses)
    return combine(law, tail, [shots] * (kmax + 1), wrong, misses)
