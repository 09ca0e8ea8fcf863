"""Fault-driven detector sampling of Clifford circuits (``CliffordCircuit.compile_detector_sampler(method="faults")``).

In a Clifford circuit with Pauli noise every deterministic detector and observable is ``const XOR (some error bits)``, and
:meth:`CliffordCircuit.analyze` has those masks.  The other detector routes either reduce the masks to a dense basis before
the first shot (``method="autoregressive"``) or carry a Pauli frame through the whole circuit for every 64 shots
(``method="frame"``).  Here a shot draws WHICH noise sites fire - by geometric skipping over the sites that share one outcome
table - and XORs each fired error bit's short list of outputs into its row: the work per shot is proportional to the faults
that happened, the compiled form is ``analyze()`` plus a transposition.

The compiled form (:class:`FaultForm`, from :meth:`CliffordCircuit.compile_faults`)
-----------------------------------------------------------------------------------
* Sites: one per channel of ``analyze()``'s ``channel_probs`` with fire probability > 0, in that order.  A site is an outcome
  table as in :mod:`tsim_amd.frame` (``outcome_thresholds``: outcome values as bitmasks over the site's error bits,
  ``ceil(cdf 2^32)`` thresholds over the firing outcomes, at most ``MAX_SITE_BITS`` bits) and the index of its first error
  bit; error bits keep ``analyze()``'s numbering.  Tables are stored once per distinct table.
* Classes: the sites of one table form a class; classes are numbered by first appearance, the sites of a class are ordered
  by channel index (``class_ptr``, ``site_chan``, ``site_e0`` are class-major).
* Columns: a CSR from error bit to the outputs it flips (``col_ptr``, ``cols``): detectors in order, then observables by
  index - the transpose of ``analyze()``'s masks.  An error bit that flips nothing has an empty list.
* ``out_const``: the noiseless values.
* Gap tables, one row per distinct ``p_fire``: ``gap_thr[k - 1] = floor((1 - p_fire)^k 2^32)`` for ``k = 1 .. K_GAP``
  (float64, on the host; at most ``2^32 - 1``).  ``K_GAP = 1024`` is a constant of the stream: at ``p = 1e-3`` a draw
  crosses 1024 quiet sites with probability 0.36, a row is 4 KiB (the tables of a circuit stay in LDS) and the binary
  search takes 10 steps.

The random stream (exact integer arithmetic; a function of the request key and the global shot index ``g`` only)
------------------------------------------------------------------------------------------------------------------
``(n0, n1) = threefry2x32(key, counter = NOISE_COUNTER)`` is the noise key of the request, and class ``c`` draws under
``(n0 ^ (c * 0x9E3779B9 mod 2^32), n1)`` - the fold the frame sites apply to their channel index.  For shot ``g`` and class
``c`` of ``n_c`` sites: ``pos = -1``; for draw ``j = 0, 1, ...`` take ``(x0, x1) = threefry2x32(key_c, (g mod 2^32,
(g >> 32) | (j << 6)))`` (``g < 2^38`` leaves 26 bits to ``j``; a class of more than ``MAX_CLASS_SITES = 2^25`` sites is
refused, it could need more draws) and ``skip = #{k in 1..K_GAP : x0 < gap_thr[k]}``.  ``skip == K_GAP``: nothing fired in
the next ``K_GAP`` sites, ``pos += K_GAP`` and draw again - the geometric law is memoryless, so this is exact for the
quantised thresholds: ``P(skip >= K_GAP + k) = gap_thr[K_GAP] gap_thr[k] / 2^64``.  Otherwise ``pos += skip + 1``; the class
is done when ``pos >= n_c``, else site ``pos`` of the class fires with the first outcome whose threshold exceeds ``x1`` (the
last one when none does).  A table with ``p_fire = 1`` has an all-zero gap row and fires at every site.  (A walk may stop as
soon as ``pos >= n_c - 1``: the next draw could only end it.)

:func:`fault_rows_host` is the numpy statement of all this: the sampler's path without a device and the oracle of the GPU
tests.  The kernel is ``csrc/tsim_faults.hip.h`` behind the ``tsim_faults_*`` handle of ``libtsim_hip.so``.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, prng
from .affine import MAX_SHOT, threefry2x32_np
from . import frame
from .frame import MAX_SITE_BITS, _FrameSampler, outcome_thresholds
from .sampler import CompiledDetectorSampler

__all__ = ["FaultForm", "FaultHandle", "CompiledFaultDetectorSampler", "build_form", "fault_rows_host", "gap_thresholds",
           "skip_of", "noise_key", "class_key", "K_GAP", "MAX_CLASS_SITES"]

K_GAP = 1024
MAX_CLASS_SITES = 1 << 25
NOISE_COUNTER = (0x6E6F6973, 0x66616C74)  # "nois", "falt"
CLASS_FOLD = 0x9E3779B9


# ---- the tables of the draw ---------------------------------------------------------------------------------------------

def gap_thresholds(p_fire: float) -> np.ndarray:
    """``uint32[K_GAP]``: ``frame.gap_thresholds`` with the ``K_GAP`` entries of this sampler's gap rows."""
    return frame.gap_thresholds(p_fire, K_GAP)


def skip_of(gap_row: np.ndarray, x0) -> np.ndarray:
    """``#{k in 1..K_GAP : x0 < gap_thr[k]}`` (``gap_row`` decreases: a binary search)."""
    return K_GAP - np.searchsorted(gap_row[::-1], np.asarray(x0, dtype=np.uint32), side="right")


def noise_key(key) -> tuple[int, int]:
    return prng.threefry2x32(int(key[0]), int(key[1]), *NOISE_COUNTER)


def class_key(nkey, c: int) -> tuple[int, int]:
    return (int(nkey[0]) ^ ((int(c) * CLASS_FOLD) & 0xFFFFFFFF), int(nkey[1]))


# ---- the form -----------------------------------------------------------------------------------------------------------

@dataclass
class FaultForm:
    """The compiled form (module docstring).  Every array is linear in the circuit."""

    num_e: int
    channel_probs: list
    class_ptr: np.ndarray    # int32[n_classes + 1]: class c holds the sites class_ptr[c] .. class_ptr[c + 1] - 1
    site_chan: np.ndarray    # int32[n_sites], class-major: the channel's index in channel_probs
    site_e0: np.ndarray      # int32[n_sites], class-major: its first error bit
    table_bits: np.ndarray   # int32[n_classes]: error bits of a site of the class
    table_ptr: np.ndarray    # int32[n_classes + 1]: outcomes of the class's table
    table_gap: np.ndarray    # int32[n_classes]: its row of gap_thr
    out_vals: np.ndarray     # uint32: outcome values (bit i = error bit e0 + i)
    out_thr: np.ndarray      # uint32: outcome thresholds
    gap_thr: np.ndarray      # uint32[n_gaps, K_GAP]
    col_ptr: np.ndarray      # int32[num_e + 1]: the outputs an error bit flips
    cols: np.ndarray         # int32
    out_const: np.ndarray    # uint8[n_out]
    num_detectors: int = 0
    kind: str = "detectors"

    @property
    def n_out(self) -> int:
        return len(self.out_const)

    @property
    def n_sites(self) -> int:
        return len(self.site_e0)

    @property
    def n_classes(self) -> int:
        return len(self.table_gap)

    def arrays(self) -> dict:
        return {k: v for k, v in vars(self).items() if isinstance(v, np.ndarray)}


def _mask_bits(mask: int, nbytes: int) -> np.ndarray:
    """Positions of the set bits of a Python-int bitmask, ascending, from its non-zero bytes."""
    b = np.frombuffer(int(mask).to_bytes(nbytes, "little"), dtype=np.uint8)
    nz = np.flatnonzero(b)
    r, c = np.nonzero(np.unpackbits(b[nz][:, None], axis=1, bitorder="little"))
    return nz[r] * 8 + c


def build_form(channel_probs, num_e: int, masks, consts, num_detectors: int) -> FaultForm:
    """``channel_probs`` (one outcome vector of length ``2^k`` per channel, ``num_e`` error bits in all) and, per output, the
    bitmask of the error bits that flip it (``masks``, Python ints) and its noiseless value (``consts``) -> the form."""
    tables: dict = {}
    gaps: dict = {}
    members: list = []   # per class: [(channel, first error bit)]
    table_bits, table_ptr, table_gap, out_vals, out_thr, gap_rows = [], [0], [], [], [], []
    e0 = 0
    for chan, probs in enumerate(channel_probs):
        probs = np.asarray(probs, dtype=np.float64)
        k = int(len(probs)).bit_length() - 1
        if 1 << k != len(probs):
            raise ValueError(f"channel {chan}: an outcome vector of length {len(probs)} is not 2^k")
        if k > MAX_SITE_BITS:
            raise NotImplementedError(f"a noise site of {k} error bits (at most {MAX_SITE_BITS})")
        if 1.0 - float(probs[0]) > 0.0:  # a site that cannot fire is dropped (its error bits stay zero)
            tkey = probs.tobytes()
            if tkey not in tables:
                p_fire, vals, thr = outcome_thresholds(probs)
                if p_fire not in gaps:
                    gaps[p_fire] = len(gap_rows)
                    gap_rows.append(gap_thresholds(p_fire))
                tables[tkey] = len(table_gap)
                table_gap.append(gaps[p_fire])
                table_bits.append(k)
                out_vals.extend(vals.tolist())
                out_thr.extend(thr.tolist())
                table_ptr.append(len(out_vals))
                members.append([])
            members[tables[tkey]].append((chan, e0))
        e0 += k
    if e0 != int(num_e):
        raise ValueError(f"the channels have {e0} error bits, num_e = {num_e}")
    for c, m in enumerate(members):
        if len(m) > MAX_CLASS_SITES:
            raise NotImplementedError(f"class {c} has {len(m)} sites (at most {MAX_CLASS_SITES}: the draw index has 26 bits)")
    # columns: the transpose of the masks, from their set bits
    nbytes = max(1, (int(num_e) + 7) // 8)
    per_out = [_mask_bits(m, nbytes) for m in masks]
    if any(len(b) and int(b[-1]) >= num_e for b in per_out):
        raise ValueError("an output's mask has an error bit beyond num_e")
    bit = np.concatenate(per_out) if per_out else np.zeros(0, np.int64)
    out = np.repeat(np.arange(len(per_out), dtype=np.int64), [len(b) for b in per_out])
    order = np.argsort(bit, kind="stable")  # (outputs stay ascending inside an error bit's list)
    col_ptr = np.zeros(int(num_e) + 1, np.int64)
    np.cumsum(np.bincount(bit.astype(np.int64), minlength=int(num_e)), out=col_ptr[1:])
    i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)  # noqa: E731
    flat = [s for m in members for s in m]
    return FaultForm(
        num_e=int(num_e), channel_probs=list(channel_probs),
        class_ptr=i32(np.concatenate([[0], np.cumsum([len(m) for m in members], dtype=np.int64)])),
        site_chan=i32([s[0] for s in flat]), site_e0=i32([s[1] for s in flat]), table_bits=i32(table_bits), table_ptr=i32(table_ptr),
        table_gap=i32(table_gap), out_vals=np.asarray(out_vals, np.uint32), out_thr=np.asarray(out_thr, np.uint32),
        gap_thr=np.asarray(gap_rows, np.uint32).reshape(-1, K_GAP), col_ptr=i32(col_ptr), cols=i32(out[order]),
        out_const=np.asarray([int(v) & 1 for v in consts], np.uint8), num_detectors=int(num_detectors))


# ---- the host statement -------------------------------------------------------------------------------------------------

def _walk_class(form: FaultForm, c: int, nkey, g: np.ndarray):
    """Class ``c`` over the shots ``g`` (uint64): ``(shot index into g, error bit)`` of every error bit that fired."""
    s0, n_c = int(form.class_ptr[c]), int(form.class_ptr[c + 1] - form.class_ptr[c])
    lo, hi = int(form.table_ptr[c]), int(form.table_ptr[c + 1])
    vals, thr = form.out_vals[lo:hi], form.out_thr[lo:hi]
    gap = form.gap_thr[int(form.table_gap[c])]
    e0 = form.site_e0[s0:s0 + n_c].astype(np.int64)
    k0, k1 = class_key(nkey, c)
    c0, c1 = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32)
    pos = np.full(len(g), -1, dtype=np.int64)
    active = np.flatnonzero(pos < n_c - 1)
    shots, bits = [], []
    j = 0
    while len(active):
        x0, x1 = threefry2x32_np(k0, k1, c0[active], c1[active] | np.uint32(j << 6))
        skip = skip_of(gap, x0)
        restart = skip == K_GAP
        p = pos[active] + np.where(restart, K_GAP, skip + 1)
        pos[active] = p
        fire = ~restart & (p < n_c)
        o = vals[np.searchsorted(thr[:-1], x1[fire], side="right")]
        first = e0[p[fire]]
        for b in range(int(form.table_bits[c])):
            sel = ((o >> np.uint32(b)) & np.uint32(1)).astype(np.bool_)
            shots.append(active[fire][sel])
            bits.append(first[sel] + b)
        active = active[p < n_c - 1]
        j += 1
    if not shots:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(shots), np.concatenate(bits)


def fault_rows_host(form: FaultForm, first_shot: int, B: int, key, *, return_e: bool = False):
    """``uint8[B, n_out]`` (0/1): the outputs of the shots ``first_shot .. first_shot + B - 1`` (a multiple of 64 first) under
    the request key ``key``.  ``return_e=True``: also ``uint64[num_e, ceil(B / 64)]``, every error bit (numbered as
    ``analyze()`` numbers them) over the shots, bit ``g % 64`` of word ``g // 64 - first_shot // 64`` (the layout of
    ``frame.frame_rows_host``; ``frame.e_rows`` packs it into rows)."""
    nkey = noise_key(key)

    def fire(g):
        fired = [_walk_class(form, c, nkey, g) for c in range(form.n_classes)] or [(np.zeros(0, np.int64),) * 2]
        return tuple(np.concatenate(x) for x in zip(*fired))

    return _rows_host(form, first_shot, B, fire, return_e)


def _rows_host(form: FaultForm, first_shot: int, B: int, fire, return_e: bool):
    """The rows of :func:`fault_rows_host` from ``fire(g) -> (shot index into g, error bit)`` of every error bit that fired in
    the shots ``g`` (uint64): the error bits through the column lists, XOR the constants."""
    B, first_shot = int(B), int(first_shot)
    if B < 0 or first_shot < 0 or first_shot % 64 or first_shot + B > MAX_SHOT:
        raise ValueError(f"shots {first_shot} .. {first_shot} + {B}: first_shot must be a multiple of 64, all inside 0 .. 2^38")
    n_out = form.n_out
    nw_all = (B + 63) // 64
    rows = np.empty((B, n_out), dtype=np.uint8)
    e_all = np.zeros((form.num_e, nw_all), np.uint64) if return_e else None
    lens = np.diff(form.col_ptr).astype(np.int64)
    step = max(1, (1 << 27) // max(1, 8 * (form.num_e + n_out)))  # words of shots at a time: 128 MiB of error and output words
    for w0 in range(0, nw_all, step):
        nw = min(step, nw_all - w0)
        n = min(64 * nw, B - 64 * w0)
        g = (first_shot + 64 * w0 + np.arange(n, dtype=np.int64)).astype(np.uint64)
        e = np.zeros((form.num_e, nw), np.uint64)
        shot, bit = fire(g)
        np.bitwise_or.at(e, (bit, shot >> 6), np.uint64(1) << (shot & 63).astype(np.uint64))
        if return_e:
            e_all[:, w0:w0 + nw] = e
        ow = np.zeros((n_out, nw), np.uint64)
        fired = np.flatnonzero(e.any(axis=1) & (lens > 0))
        if len(fired):
            n_f = lens[fired]
            at = np.repeat(form.col_ptr[fired].astype(np.int64) - (np.cumsum(n_f) - n_f), n_f) + np.arange(int(n_f.sum()))
            np.bitwise_xor.at(ow, form.cols[at], e[np.repeat(fired, n_f)])
        if n_out:
            bits = np.unpackbits(ow.view(np.uint8).reshape(n_out, nw * 8), axis=1, bitorder="little")  # [n_out, 64 nw]
            rows[64 * w0:64 * w0 + n] = bits[:, :n].T
    rows ^= form.out_const[None, :]
    return (rows, e_all) if return_e else rows


# ---- the device handle --------------------------------------------------------------------------------------------------

class FaultHandle(_lib.DeviceHandle):
    """``tsim_faults`` of one device: the form's arrays (outputs padded to whole uint64 words with constant zeros that
    nothing flips when ``pad_outputs``).  The device handle is created by the first launch."""

    CREATE, DESTROY = "tsim_faults_create", "tsim_faults_destroy"
    INFO = ("tsim_faults_info", ("n_out", "num_e", "n_sites", "n_classes", "device", "gap_k", "window", "n_windows", "row_words", "waves",
                                 "lds_bytes", "tables_in_lds", "n_gaps", "n_cols", "max_class_sites", "max_window"))

    def __init__(self, form: FaultForm, *, device: int = 0, pad_outputs: bool = False):
        self.form, self._device = form, int(device)
        pad = -form.n_out % 64 if pad_outputs else 0
        self.out_const = np.ascontiguousarray(np.concatenate([form.out_const, np.zeros(pad, np.uint8)]))
        self.n_out = len(self.out_const)

    def _create_args(self) -> tuple:
        f = self.form
        arrays = dict(f.arrays(), out_const=self.out_const)
        self._keep = {n: np.ascontiguousarray(arrays[n]) for n in _lib.FaultsDesc.ARRAYS}
        sizes = dict(n_out=self.n_out, num_e=f.num_e, n_sites=f.n_sites, n_classes=f.n_classes, n_outcomes=len(f.out_vals),
                     n_gaps=len(f.gap_thr), gap_k=f.gap_thr.shape[1] if f.gap_thr.ndim == 2 else 0, n_cols=len(f.cols))
        desc = _lib.FaultsDesc(**sizes, **{n: a.ctypes.data for n, a in self._keep.items()})
        return self._device, C.byref(desc)

    def sample_device(self, B: int, d_out: int, *, key, first_shot: int = 0, out_row_bytes: int, out_packed: bool, col0: int = 0,
                      n_cols: int | None = None, stream: int = 0) -> None:
        """Caller-owned output buffer, asynchronous on ``stream`` (0: the handle's own); see ``tsim_faults_sample_device`` in
        ``include/tsim_hip.h``."""
        self._request("tsim_faults_sample_device", (), B, d_out, key=key, first_shot=first_shot, out_row_bytes=out_row_bytes,
                      out_packed=out_packed, col0=col0, n_cols=n_cols, stream=stream)


# ---- the sampler --------------------------------------------------------------------------------------------------------

class CompiledFaultDetectorSampler(_FrameSampler, CompiledDetectorSampler):
    """A detector sampler over the fault form of a Clifford circuit: ``sample()``, ``count()`` and ``sample_write()`` of
    :class:`CompiledDetectorSampler` with every keyword.  It is wired as the frame samplers are (a component-free program
    whose rows come from ``_direct_on_device`` / ``_direct_device`` / ``_sample_direct``, one key per request, ``noise=``
    accepted and without effect); the handle and the host statement are this module's."""

    def __init__(self, form: FaultForm, *, seed: int | None = None, device: int = 0, noise: str = "host"):
        if form.kind != "detectors":
            raise ValueError("a detector sampler needs the form of compile_faults()")
        self._init_frame(form, seed, device, noise)

    def _frame_handle(self) -> FaultHandle:
        """Whole uint64 words per row: the padded rows the tally and the file sink read need no clearing."""
        if self._frame is None:
            self._frame = FaultHandle(self._form, device=self._device, pad_outputs=True)
        return self._frame

    def _bytes_per_shot(self) -> int:
        n_out = self._form.n_out
        return max(1, 8 * ((n_out + 63) // 64) + n_out)

    def _sample_direct(self, shots: int) -> np.ndarray:
        if self._direct_on_device(shots):  # (post-selected requests of a component-free program come here)
            return self._direct_device(shots, None)
        return fault_rows_host(self._form, 0, shots, self._next_key()).view(np.bool_)

    @property
    def num_detectors(self) -> int:
        return self._num_detectors

    @property
    def num_observables(self) -> int:
        return self._form.n_out - self._num_detectors

    def __repr__(self) -> str:
        f = self._form
        return (f"{type(self).__name__}({f.n_out} outputs, {f.num_e} error bits, {f.n_sites} noise sites in {f.n_classes} classes, "
                f"{len(f.cols)} flips)")
