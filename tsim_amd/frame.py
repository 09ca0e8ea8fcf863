"""Pauli-frame sampling of Clifford circuits (``CliffordCircuit.compile_sampler(method="frame")`` and
``compile_detector_sampler(method="frame")``).

A measurement record of a Clifford circuit with Pauli noise is ``const XOR (random symbols) XOR (frame flip)``.  The first two
terms come from the symbolic tableau run (``rec_vals``, ``rec_syms`` of :meth:`CliffordCircuit.analyze`); the last one is what
the noise did to this shot.  The other Clifford routes write the flip as a dense GF(2) function of all error bits before the
first shot is drawn; here a Pauli frame ``(x_q, z_q)`` per shot is carried through the circuit, 64 shots to a word, and the
noise is drawn where it acts.  Cost is linear in the circuit times shots / 64, the compiled form is linear in the circuit.

The compiled form (:class:`FrameForm`, from :meth:`CliffordCircuit.compile_frame`)
-----------------------------------------------------------------------------------
One walk over the instructions with a recorder that shares ``_Sim``'s gate decompositions logs primitive frame operations::

    H q            swap x_q and z_q                      MEASURE q -> i     flip word of record i := x_q (q = -1: := 0)
    S q            z_q ^= x_q                            FEEDBACK i -> q    x_q and / or z_q ^= flip word of record i
    CX c t         x_t ^= x_c, z_c ^= z_t                NOISE n            draw site n, XOR its bits into their targets
    RESET q        x_q = z_q = 0

(Paulis do nothing to a frame.)  A noise site is an outcome table (the helpers of :mod:`tsim_amd.channels`, Z bit before X bit)
and, per error bit, a list of targets: the ``x`` or the ``z`` of a qubit, or a record (the flip of ``M(p)``, the herald of
``HERALDED_*``, the bit of ``MPAD(p)``).  Sites that cannot fire are dropped.  The branches of a ``CORRELATED_ERROR`` chain
are the bits of ONE site drawn where the chain starts; each bit lands in a hidden record (numbered after the circuit's own)
and a FEEDBACK applies it where its branch stands.  Consecutive operations of one kind whose qubits and records are pairwise
disjoint form a batch, and an operation moves up to an earlier batch of its kind when nothing in between touches its qubits
and records (``MR 1 3 5`` is one MEASURE and one RESET batch): the items of a batch may run in any order, the batches run in
order.  Outputs (records, or detectors then
observables) are CSR lists over the columns ``[records | random symbols]`` plus a constant bit; outputs whose symbols do not
cancel (gauge detectors) are kept.

The random streams (exact integer arithmetic; a function of the request key and the global shot index ``g`` only)
------------------------------------------------------------------------------------------------------------------
* Symbols are :func:`tsim_amd.affine.random_words`: symbol ``s`` of shot ``g`` is bit ``g % 64`` of the Threefry block
  ``(s, g // 64)`` under the request key - a noiseless circuit gives the rows of ``method="affine"``.
* Noise: ``(n0, n1) = threefry2x32(key, counter = NOISE_COUNTER)`` is the noise key of the request, and site ``n`` (numbered
  as ``analyze()`` numbers its channels) draws under ``(n0 ^ (n * 0x9E3779B9 mod 2^32), n1)`` - the fold the device noise
  kernels apply to a channel index.  For the 64-shot word ``tau = g // 64``: ``pos = -1``; for draw ``j = 0, 1, ...`` take
  ``(x0, x1) = threefry2x32(key_n, (tau, j))``, ``skip = #{k in 1..64 : x0 < gap_thr[k]}`` with
  ``gap_thr[k] = floor((1 - p_fire)^k 2^32)`` (float64, on the host, one table per distinct ``p_fire``; clamped to
  ``2^32 - 1``), ``pos += skip + 1``; stop when ``pos > 63``, else shot ``64 tau + pos`` fires with the first outcome whose
  threshold ``ceil(cdf 2^32)`` exceeds ``x1`` (the last outcome when none does).  The host statement and the kernel read the
  same tables.

:func:`frame_rows_host` is the numpy statement of all this: the sampler's path without a device and the oracle of the GPU
tests.  The kernels are ``csrc/tsim_frame.hip.h`` behind the ``tsim_frame_*`` handle of ``libtsim_hip.so``.
"""

from __future__ import annotations

import bisect
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, prng
from .affine import MAX_SHOT, random_words, threefry2x32_np
from .channels import correlated_error_probs, error_probs, heralded_pauli_channel_1_probs, pauli_channel_1_probs
from .clifford import _Analysis, _Sim, _Tableau, pauli_channel_2_probs
from .program import CompiledProgram
from .sampler import CompiledDetectorSampler, CompiledMeasurementSampler, _check_request

__all__ = ["FrameForm", "FrameHandle", "CompiledFrameMeasurementSampler", "CompiledFrameDetectorSampler", "frame_rows_host",
           "noise_key", "site_key", "gap_thresholds", "outcome_thresholds", "e_rows"]

K_H, K_S, K_CX, K_RESET, K_MEASURE, K_FEEDBACK, K_NOISE = range(7)
KIND_NAMES = ("H", "S", "CX", "RESET", "MEASURE", "FEEDBACK", "NOISE")
T_X, T_Z, T_REC = 0, 1, 2          # target kinds; a target is 4 * index + kind
NOISE_COUNTER = (0x6E6F6973, 0x6672616D)  # "nois", "fram"
SITE_FOLD = 0x9E3779B9
MAX_SITE_BITS = 32


# ---- the recorder -------------------------------------------------------------------------------------------------------

class _FrameRecorder(_Sim):
    """``_Sim`` without the bigint error masks: the tableau runs as in ``analyze()`` (``rec_vals``, ``rec_syms``, ``n_random``
    come out the same), the frame part of every primitive is logged instead of applied."""

    allow_gauge = True

    def __init__(self, n_qubits: int, tableau=None):
        """``tableau``: anything with ``_Tableau``'s methods (the frame operations do not depend on it; default: a
        ``_Tableau`` of ``n_qubits + 1`` qubits, quadratic in memory)."""
        self.n = n_qubits + 1  # one auxiliary qubit for Pauli-product measurements
        self.aux = n_qubits
        self.tab = _Tableau(self.n) if tableau is None else tableau
        self.out = _Analysis()
        self.corr_probs: list = []
        self.ops: list = []     # (kind, a, b, c)
        self.sites: list = []   # dict(chan, e0, probs, targets: per error bit a list of (kind, index)); hidden records: index < 0
        self.n_hidden = 0
        self._chain_at = 0
        self._chain_hidden: list = []

    # primitives
    def _h(self, q):
        self.tab.h(q)
        self.ops.append((K_H, q, 0, 0))

    def _s(self, q):
        self.tab.s(q)
        self.ops.append((K_S, q, 0, 0))

    def _cx(self, c, t):
        self.tab.cx(c, t)
        self.ops.append((K_CX, c, t, 0))

    def _feedback_frame(self, rec_index, q, px, pz):
        self.ops.append((K_FEEDBACK, rec_index, q, (1 if px else 0) | (2 if pz else 0)))

    def _reset_frame(self, q):
        self.ops.append((K_RESET, q, 0, 0))

    def _new_record(self, q, val, sym) -> int:
        i = len(self.out.rec_sets)
        self.ops.append((K_MEASURE, q, i, 0))
        self.out.rec_sets.append(0)
        self.out.rec_vals.append(val)
        self.out.rec_syms.append(sym)
        return i

    # noise
    def _site(self, probs, targets, at: int | None = None) -> None:
        out = self.out
        probs = np.asarray(probs, dtype=np.float64)
        if len(targets) > MAX_SITE_BITS:
            raise NotImplementedError(f"a noise site of {len(targets)} error bits (at most {MAX_SITE_BITS})")
        site = dict(chan=len(out.channel_probs), e0=out.num_e, probs=probs, targets=targets)
        out.channel_probs.append(probs)
        out.num_e += len(targets)
        if 1.0 - float(probs[0]) > 0.0:  # a site that cannot fire is dropped (its error bits stay zero)
            self.sites.append(site)
            op = (K_NOISE, len(self.sites) - 1, 0, 0)
            if at is None:
                self.ops.append(op)
            else:
                self.ops.insert(at, op)

    def error1(self, q, x, z, p):
        self._site(error_probs(p), [([(T_X, q)] if x else []) + ([(T_Z, q)] if z else [])])

    def pauli_channel_1(self, q, px, py, pz):
        self._site(pauli_channel_1_probs(px, py, pz), [[(T_Z, q)], [(T_X, q)]])

    def pauli_channel_2(self, qi, qj, p15):
        self._site(pauli_channel_2_probs(*p15), [[(T_Z, qi)], [(T_X, qi)], [(T_Z, qj)], [(T_X, qj)]])

    def heralded_pauli_channel_1(self, q, pi, px, py, pz):
        i = self._new_record(-1, 0, 0)
        self._site(heralded_pauli_channel_1_probs(pi, px, py, pz), [[(T_REC, i)], [(T_Z, q)], [(T_X, q)]])

    def mpad(self, value, p=0.0):
        i = self._new_record(-1, value & 1, 0)
        if p > 0:
            self._site(error_probs(p), [[(T_REC, i)]])

    def correlated_error(self, paulis, p):
        if not self.corr_probs:
            self._chain_at, self._chain_hidden = len(self.ops), []
        hid = -1 - self.n_hidden  # the branch's bit: a hidden record, applied here by FEEDBACK
        self.n_hidden += 1
        self._chain_hidden.append(hid)
        for kind, q in paulis:
            self.ops.append((K_FEEDBACK, hid, q, (1 if kind in ("X", "Y") else 0) | (2 if kind in ("Z", "Y") else 0)))
        self.corr_probs.append(p)

    def finalize_correlated(self):
        if not self.corr_probs:
            return
        at = self._chain_at
        self._site(correlated_error_probs(self.corr_probs), [[(T_REC, h)] for h in self._chain_hidden], at=at)
        self.ops[at:at] = [(K_MEASURE, -1, h, 0) for h in self._chain_hidden]
        self.corr_probs = []

    # measurement
    def measure(self, q, basis="Z", p=0.0, invert=False, reset=False):
        self._basis_in(q, basis)
        val, sym = self.tab.measure_z(q)
        i = self._new_record(q, val ^ (1 if invert else 0), sym)
        if p > 0:
            self._site(error_probs(p), [[(T_REC, i)]])
        if reset:
            self._reset_z(q)
        self._basis_in(q, basis)


# ---- the tables of the draw ---------------------------------------------------------------------------------------------

def gap_thresholds(p_fire: float, n: int = 64) -> np.ndarray:
    """``uint32[n]``: entry ``k - 1`` is ``floor((1 - p_fire)^k 2^32)``, at most ``2^32 - 1``."""
    k = np.arange(1, n + 1, dtype=np.float64)
    t = np.floor(np.power(np.float64(1.0) - np.float64(p_fire), k) * 4294967296.0)
    return np.minimum(t, 4294967295.0).astype(np.uint32)


def outcome_thresholds(probs) -> tuple[float, np.ndarray, np.ndarray]:
    """``(p_fire, outcome values uint32[n], thresholds uint32[n])`` over the non-identity outcomes of non-zero probability:
    ``ceil(cdf 2^32)`` of the conditional CDF (``1 - p0``, ``cumsum(p / p_fire)``, renormalised by its last entry - the float
    sequence of ``ChannelSampler``), the last entry ``2^32 - 1``."""
    probs = np.asarray(probs, dtype=np.float64)
    p_fire = 1.0 - float(probs[0])
    vals = np.nonzero(probs[1:] > 0)[0] + 1
    cdf = np.cumsum(probs[vals] / p_fire, dtype=np.float64)
    cdf /= cdf[-1]
    thr = np.minimum(np.ceil(np.clip(cdf, 0.0, 1.0) * 4294967296.0), 4294967295.0).astype(np.uint32)
    thr[-1] = 0xFFFFFFFF
    return p_fire, vals.astype(np.uint32), thr


def noise_key(key) -> tuple[int, int]:
    return prng.threefry2x32(int(key[0]), int(key[1]), *NOISE_COUNTER)


def site_key(nkey, chan: int) -> tuple[int, int]:
    return (int(nkey[0]) ^ ((int(chan) * SITE_FOLD) & 0xFFFFFFFF), int(nkey[1]))


# ---- the form -----------------------------------------------------------------------------------------------------------

@dataclass
class FrameForm:
    """The compiled form (module docstring).  Every array is linear in the circuit."""

    n_qubits: int            # with the auxiliary qubit of the Pauli-product measurements
    n_records: int           # the circuit's records; hidden records follow: n_records .. n_records + n_hidden - 1
    n_hidden: int
    n_random: int
    num_e: int
    channel_probs: list
    op_kind: np.ndarray      # uint8[n_ops]
    op_a: np.ndarray         # int32[n_ops]: H/S/RESET q; CX c; MEASURE q or -1; FEEDBACK record; NOISE site
    op_b: np.ndarray         # int32[n_ops]: CX t; MEASURE record; FEEDBACK q
    op_c: np.ndarray         # int32[n_ops]: FEEDBACK 1 (x) | 2 (z)
    batch_ptr: np.ndarray    # int32[n_batches + 1]: batch b holds the operations batch_ptr[b] .. batch_ptr[b + 1] - 1
    site_chan: np.ndarray    # int32[n_sites]: the channel's index in channel_probs (folded into the site's key)
    site_e0: np.ndarray      # int32[n_sites]: its first error bit
    site_table: np.ndarray   # int32[n_sites]: its outcome table
    site_bit: np.ndarray     # int32[n_sites + 1]: its error bits are the rows site_bit[n] .. of bit_ptr
    bit_ptr: np.ndarray      # int32[n_bits + 1]: targets of an error bit
    targets: np.ndarray      # int32: 4 * index + kind (0: x of qubit, 1: z of qubit, 2: record)
    table_ptr: np.ndarray    # int32[n_tables + 1]: outcomes of a table
    table_gap: np.ndarray    # int32[n_tables]: its row of gap_thr
    out_vals: np.ndarray     # uint32: outcome values (bit i = error bit i of the site)
    out_thr: np.ndarray      # uint32: outcome thresholds
    gap_thr: np.ndarray      # uint32[n_gaps, 64]
    out_const: np.ndarray    # uint8[n_out]
    out_ptr: np.ndarray      # int32[n_out + 1]
    out_cols: np.ndarray     # int32: column c < n_records: record c; else random symbol c - n_records
    num_detectors: int = 0
    kind: str = "measurements"

    @property
    def n_out(self) -> int:
        return len(self.out_const)

    @property
    def n_ops(self) -> int:
        return len(self.op_kind)

    @property
    def n_batches(self) -> int:
        return len(self.batch_ptr) - 1

    def arrays(self) -> dict:
        return {k: v for k, v in vars(self).items() if isinstance(v, np.ndarray)}

    def describe(self) -> list:
        """The batches, readable: ``["H 0 2", "CX 0>1", "MEASURE 0>0 1>1", ...]``."""
        lines = []
        for b in range(self.n_batches):
            lo, hi = int(self.batch_ptr[b]), int(self.batch_ptr[b + 1])
            k = int(self.op_kind[lo])
            items = []
            for i in range(lo, hi):
                a, bb, c = int(self.op_a[i]), int(self.op_b[i]), int(self.op_c[i])
                if k in (K_H, K_S, K_RESET):
                    items.append(str(a))
                elif k in (K_CX, K_MEASURE):
                    items.append(f"{a}>{bb}")
                elif k == K_FEEDBACK:
                    items.append(f"{a}>{bb}{'x' if c & 1 else ''}{'z' if c & 2 else ''}")
                else:
                    items.append(str(a))
            lines.append(KIND_NAMES[k] + " " + " ".join(items))
        return lines


def _op_resources(kind, a, b, n_qubits, site_targets):
    if kind in (K_H, K_S, K_RESET):
        return (a,)
    if kind == K_CX:
        return (a, b)
    if kind == K_MEASURE:
        return ((a,) if a >= 0 else ()) + (n_qubits + b,)
    if kind == K_FEEDBACK:
        return (n_qubits + a, b)
    return site_targets[a]


def build_form(rec: _FrameRecorder, kind: str) -> FrameForm:
    """The recorder's log -> :class:`FrameForm` with the outputs of ``kind`` (``"measurements"`` or ``"detectors"``)."""
    an = rec.out
    nq, n_rec = rec.n, len(an.rec_sets)
    fix = lambda r: r if r >= 0 else n_rec + (-1 - r)  # noqa: E731 - hidden records follow the circuit's own
    ops = []
    for k, a, b, c in rec.ops:
        if k == K_MEASURE:
            b = fix(b)
        elif k == K_FEEDBACK:
            a = fix(a)
        ops.append((k, a, b, c))
    # sites, tables
    tables: dict = {}
    gaps: dict = {}
    table_ptr, table_gap, out_vals, out_thr, gap_rows = [0], [], [], [], []
    site_chan, site_e0, site_table, site_bit, bit_ptr, targets, site_res = [], [], [], [0], [0], [], []
    for s in rec.sites:
        tkey = s["probs"].tobytes()
        if tkey not in tables:
            p_fire, vals, thr = outcome_thresholds(s["probs"])
            if p_fire not in gaps:
                gaps[p_fire] = len(gap_rows)
                gap_rows.append(gap_thresholds(p_fire))
            tables[tkey] = len(table_gap)
            table_gap.append(gaps[p_fire])
            out_vals.extend(vals.tolist())
            out_thr.extend(thr.tolist())
            table_ptr.append(len(out_vals))
        site_chan.append(s["chan"])
        site_e0.append(s["e0"])
        site_table.append(tables[tkey])
        res = []
        for tl in s["targets"]:
            for tk, ti in tl:
                ti = fix(ti) if tk == T_REC else ti
                targets.append(4 * ti + tk)
                res.append(nq + ti if tk == T_REC else ti)
            bit_ptr.append(len(targets))
        site_bit.append(len(bit_ptr) - 1)
        site_res.append(tuple(set(res)))
    # batches: an operation joins the first batch of its kind that comes after every batch touching one of its qubits or
    # records (operations on other qubits and records commute with it), else it opens a new one.  Consecutive operations of
    # one kind on disjoint qubits and records share a batch; so do the MEASURE, RESET, MEASURE, RESET ... of ``MR 1 3 5``.
    last: dict = {}
    of_kind: list = [[] for _ in range(7)]
    where, n_batches = [], 0
    for k, a, b, _c in ops:
        res = _op_resources(k, a, b, nq, site_res)
        first = 1 + max((last.get(r, -1) for r in res), default=-1)
        at = bisect.bisect_left(of_kind[k], first)
        if at < len(of_kind[k]):
            bi = of_kind[k][at]
        else:
            bi = n_batches
            n_batches += 1
            of_kind[k].append(bi)
        where.append(bi)
        for r in res:
            last[r] = bi
    order = np.argsort(np.asarray(where, dtype=np.int64), kind="stable")
    ops = [ops[i] for i in order.tolist()]
    batch_ptr = np.searchsorted(np.asarray(where, dtype=np.int64)[order], np.arange(n_batches + 1)).tolist()
    # outputs
    n_random = max((int(y).bit_length() for y in an.rec_syms), default=0)  # (as the affine form counts them)
    if kind == "measurements":
        lists = [[i] for i in range(n_rec)]
        consts = [int(v) & 1 for v in an.rec_vals]
        syms = list(an.rec_syms)
        nd = 0
    elif kind == "detectors":
        keys = sorted(an.observables)
        lists = [list(r) for r in an.detector_records] + [sorted(an.observable_records.get(k, ())) for k in keys]
        consts = [int(v) & 1 for _, v in an.detectors] + [int(an.observables[k][1]) & 1 for k in keys]
        syms = list(an.detector_syms) + [an.observables[k][2] for k in keys]
        nd = len(an.detectors)
    else:
        raise ValueError(f"kind must be 'measurements' or 'detectors', got {kind!r}")
    from .clifford import _bits

    cols = [l + [n_rec + s for s in _bits(int(y))] for l, y in zip(lists, syms)]
    out_ptr = np.zeros(len(cols) + 1, np.int32)
    out_ptr[1:] = np.cumsum([len(l) for l in cols], dtype=np.int64)
    i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)  # noqa: E731
    opa = np.asarray(ops, dtype=np.int64).reshape(-1, 4)
    return FrameForm(
        n_qubits=nq, n_records=n_rec, n_hidden=rec.n_hidden, n_random=n_random, num_e=an.num_e, channel_probs=list(an.channel_probs),
        op_kind=opa[:, 0].astype(np.uint8), op_a=i32(opa[:, 1]), op_b=i32(opa[:, 2]), op_c=i32(opa[:, 3]), batch_ptr=i32(batch_ptr),
        site_chan=i32(site_chan), site_e0=i32(site_e0), site_table=i32(site_table), site_bit=i32(site_bit), bit_ptr=i32(bit_ptr),
        targets=i32(targets), table_ptr=i32(table_ptr), table_gap=i32(table_gap), out_vals=np.asarray(out_vals, np.uint32),
        out_thr=np.asarray(out_thr, np.uint32), gap_thr=np.asarray(gap_rows, np.uint32).reshape(-1, 64),
        out_const=np.asarray(consts, np.uint8), out_ptr=out_ptr, out_cols=i32([c for l in cols for c in l]), num_detectors=nd, kind=kind)


# ---- the host statement -------------------------------------------------------------------------------------------------

def draw_site(form: FrameForm, n: int, nkey, taus: np.ndarray) -> np.ndarray:
    """``uint64[k, len(taus)]``: the ``k`` error bits of site ``n`` over the 64 shots of each word ``tau`` (module docstring)."""
    t = int(form.site_table[n])
    lo, hi = int(form.table_ptr[t]), int(form.table_ptr[t + 1])
    vals, thr = form.out_vals[lo:hi], form.out_thr[lo:hi]
    gap_up = form.gap_thr[int(form.table_gap[t])][::-1]  # ascending
    k0, k1 = site_key(nkey, int(form.site_chan[n]))
    k = int(form.site_bit[n + 1] - form.site_bit[n])
    masks = np.zeros((k, len(taus)), dtype=np.uint64)
    pos = np.full(len(taus), -1, dtype=np.int64)
    active = np.arange(len(taus))
    j = 0
    while len(active):
        x0, x1 = threefry2x32_np(k0, k1, taus[active], np.uint32(j))
        skip = 64 - np.searchsorted(gap_up, x0, side="right")  # the entries above x0
        p = pos[active] + skip + 1
        pos[active] = p
        live = p <= 63
        active, p, x1 = active[live], p[live], x1[live]
        o = vals[np.searchsorted(thr[:-1], x1, side="right")]
        for b in range(k):
            sel = ((o >> np.uint32(b)) & np.uint32(1)).astype(np.bool_)
            masks[b, active[sel]] |= np.uint64(1) << p[sel].astype(np.uint64)
        j += 1
    return masks


def _run_words(form: FrameForm, key, tile0: int, nw: int, want_e: bool):
    """Flip words ``uint64[n_records + n_hidden, nw]`` of the words ``tile0 .. tile0 + nw - 1`` (and the error bits)."""
    nq = form.n_qubits
    x, z = np.zeros((nq, nw), np.uint64), np.zeros((nq, nw), np.uint64)
    F = np.zeros((form.n_records + form.n_hidden, nw), np.uint64)
    e = np.zeros((form.num_e, nw), np.uint64) if want_e else None
    taus = (int(tile0) + np.arange(nw, dtype=np.int64)).astype(np.uint32)
    nkey = noise_key(key)
    frames = (x, z)
    for b in range(form.n_batches):
        lo, hi = int(form.batch_ptr[b]), int(form.batch_ptr[b + 1])
        k, a, bb, c = int(form.op_kind[lo]), form.op_a[lo:hi], form.op_b[lo:hi], form.op_c[lo:hi]
        if k == K_H:
            x[a], z[a] = z[a], x[a]
        elif k == K_S:
            z[a] ^= x[a]
        elif k == K_CX:
            x[bb] ^= x[a]
            z[a] ^= z[bb]
        elif k == K_RESET:
            x[a] = 0
            z[a] = 0
        elif k == K_MEASURE:
            real = a >= 0
            F[bb[real]] = x[a[real]]
            F[bb[~real]] = 0
        elif k == K_FEEDBACK:
            fx, fz = (c & 1) != 0, (c & 2) != 0
            x[bb[fx]] ^= F[a[fx]]
            z[bb[fz]] ^= F[a[fz]]
        else:
            for n in a.tolist():
                bits = draw_site(form, n, nkey, taus)
                r0 = int(form.site_bit[n])
                for i in range(len(bits)):
                    for t in form.targets[form.bit_ptr[r0 + i]:form.bit_ptr[r0 + i + 1]].tolist():
                        (F if t & 3 == T_REC else frames[t & 3])[t >> 2] ^= bits[i]
                if want_e:
                    e[int(form.site_e0[n]):int(form.site_e0[n]) + len(bits)] = bits
    return F, e


def frame_rows_host(form: FrameForm, B: int, first_shot: int, key, *, return_e: bool = False):
    """``uint8[B, n_out]`` (0/1): the outputs of the shots ``first_shot .. first_shot + B - 1`` (a multiple of 64 first) under
    the request key ``key``.  ``return_e=True``: also ``uint64[num_e, ceil(B / 64)]``, every error bit (numbered as
    ``analyze()`` numbers them) over the shots, bit ``g % 64`` of word ``g // 64 - first_shot // 64``."""
    B, first_shot = int(B), int(first_shot)
    if B < 0 or first_shot < 0 or first_shot % 64 or first_shot + B > MAX_SHOT:
        raise ValueError(f"shots {first_shot} .. {first_shot} + {B}: first_shot must be a multiple of 64, all inside 0 .. 2^38")
    n_out, n_rec = form.n_out, form.n_records
    out = np.empty((B, n_out), dtype=np.uint8)
    nw_all = (B + 63) // 64
    e_all = np.zeros((form.num_e, nw_all), np.uint64) if return_e else None
    per_word = 16 * form.n_qubits + 8 * (n_rec + form.n_hidden + form.num_e * bool(return_e)) + 8 * form.n_random + 72 * n_out + 64
    step = max(1, (1 << 28) // per_word)
    # S[c, j] = 1 iff column c occurs an odd number of times in the list of output j
    for w0 in range(0, nw_all, step):
        nw = min(step, nw_all - w0)
        F, e = _run_words(form, key, first_shot // 64 + w0, nw, return_e)
        if return_e:
            e_all[:, w0:w0 + nw] = e
        sym = random_words(key, form.n_random, first_shot // 64 + w0, nw).T if form.n_random else None  # [n_random, nw]
        ow = np.zeros((n_out, nw), np.uint64)
        for j in range(n_out):
            for c in form.out_cols[form.out_ptr[j]:form.out_ptr[j + 1]].tolist():
                ow[j] ^= F[c] if c < n_rec else sym[c - n_rec]
        bits = np.unpackbits(ow.view(np.uint8).reshape(n_out, nw * 8), axis=1, bitorder="little")  # [n_out, 64 nw]
        r0 = 64 * w0
        n = min(64 * nw, B - r0)
        out[r0:r0 + n] = bits[:, :n].T
    out ^= form.out_const[None, :]
    return (out, e_all) if return_e else out


def e_rows(e_words: np.ndarray, B: int) -> np.ndarray:
    """The error bits of :func:`frame_rows_host` as packed rows ``uint64[B, ceil(num_e / 64)]`` (bit ``i`` of a row = ``e_i``)."""
    num_e, nw = e_words.shape
    bits = np.unpackbits(np.ascontiguousarray(e_words).view(np.uint8).reshape(num_e, nw * 8), axis=1, bitorder="little")[:, :B]
    W = max(1, (num_e + 63) // 64)
    rows = np.zeros((B, W * 64), np.uint8)
    rows[:, :num_e] = bits.T
    return np.packbits(rows, axis=1, bitorder="little").view(np.uint64).reshape(B, W)


# ---- the device handle --------------------------------------------------------------------------------------------------

class FrameHandle(_lib.DeviceHandle):
    """``tsim_frame`` of one device: the form's arrays (outputs padded to whole uint64 words with constant zeros when
    ``pad_outputs``).  The device handle is created by the first launch."""

    CREATE, DESTROY = "tsim_frame_create", "tsim_frame_destroy"
    INFO = ("tsim_frame_info", ("n_qubits", "n_records", "n_hidden", "n_random", "n_out", "n_ops", "n_batches", "n_sites", "device", "T",
                                "lds_bytes", "max_qubits", "window", "n_windows", "max_words", "max_batch_items"))

    def __init__(self, form: FrameForm, *, device: int = 0, pad_outputs: bool = False):
        self.form, self._device = form, int(device)
        pad = -form.n_out % 64 if pad_outputs else 0
        self.out_ptr = np.ascontiguousarray(np.concatenate([form.out_ptr, np.full(pad, form.out_ptr[-1], np.int32)]))
        self.out_const = np.ascontiguousarray(np.concatenate([form.out_const, np.zeros(pad, np.uint8)]))
        self.n_out = len(self.out_const)

    def _create_args(self) -> tuple:
        f = self.form
        arrays = dict(f.arrays(), out_const=self.out_const, out_ptr=self.out_ptr)
        self._keep = {n: np.ascontiguousarray(arrays[n]) for n in _lib.FrameDesc.ARRAYS}
        sizes = dict(n_qubits=f.n_qubits, n_records=f.n_records, n_hidden=f.n_hidden, n_random=f.n_random, n_out=self.n_out,
                     n_ops=f.n_ops, n_batches=f.n_batches, n_sites=len(f.site_chan), n_bits=len(f.bit_ptr) - 1,
                     n_targets=len(f.targets), n_tables=len(f.table_gap), n_outcomes=len(f.out_vals), n_gaps=len(f.gap_thr),
                     n_cols=len(f.out_cols))
        desc = _lib.FrameDesc(**sizes, **{n: a.ctypes.data for n, a in self._keep.items()})
        return self._device, C.byref(desc)

    def sample_device(self, B: int, d_out: int, *, key, first_shot: int = 0, out_row_bytes: int, out_packed: bool, col0: int = 0,
                      n_cols: int | None = None, stream: int = 0) -> None:
        """Caller-owned output buffer, asynchronous on ``stream`` (0: the handle's own); see ``tsim_frame_sample_device`` in
        ``include/tsim_hip.h``.  The record-flip scratch belongs to the handle and grows to what ``B`` needs."""
        self._request("tsim_frame_sample_device", (), B, d_out, key=key, first_shot=first_shot, out_row_bytes=out_row_bytes,
                      out_packed=out_packed, col0=col0, n_cols=n_cols, stream=stream)


# ---- the samplers -------------------------------------------------------------------------------------------------------

class _FrameSampler:
    """What the two frame samplers share.  They are component-free programs whose rows come from the hook such programs use
    (``_direct_on_device`` / ``_direct_device`` / ``_sample_direct``): ``count()`` and ``sample_write()`` work as they do for
    every sampler.  No ``ChannelSampler`` exists: the noise is part of the rows' own stream, so ``noise=`` changes nothing."""

    def _init_frame(self, form: FrameForm, seed, device: int, noise: str) -> None:
        if noise not in ("host", "device"):
            raise ValueError("noise must be 'host' or 'device'")
        if seed is None:
            seed = int(np.random.default_rng().integers(0, 2**30))
        n_out = form.n_out
        self._form = form
        self._noise, self._mode, self._device = noise, "auto", int(device)
        self._key = prng.key(seed)
        self._program = CompiledProgram(components=(), direct_f_indices=np.zeros(0, np.int32), direct_flips=np.zeros(0, np.bool_),
                                        output_order=np.arange(n_out, dtype=np.int32), output_reindex=None, num_outputs=n_out,
                                        num_detectors=form.num_detectors)
        self._channel_sampler = None
        self._noise_key = None
        self._num_detectors = int(form.num_detectors)
        self._direct = None
        self._direct_detector_mask = np.zeros(self._num_detectors, dtype=np.bool_)
        self._init_route_state()
        self._frame = None
        self._carrier = None

    def _hip(self):
        """Device buffers and streams hang off a program handle: a one-output direct program carries them."""
        if self._carrier is None:
            from .backend import get_hip_program
            from .program import make_program

            self._carrier = get_hip_program(make_program([], [(0, 0, False)], 1, 0), self._device, self._mode)
        return self._carrier

    def _frame_handle(self) -> FrameHandle:
        """Whole uint64 words per row: the padded rows the tally and the file sink read need no clearing."""
        if self._frame is None:
            self._frame = FrameHandle(self._form, device=self._device, pad_outputs=True)
        return self._frame

    def _bytes_per_shot(self) -> int:
        n_out = self._form.n_out
        return max(1, 8 * ((n_out + 63) // 64) + n_out + (self._form.n_records + self._form.n_hidden) // 8)

    def _compute_reference_sample(self) -> np.ndarray:
        """The outputs with every error bit and every random symbol zero; costs no key."""
        return self._form.out_const.astype(np.bool_)

    def _direct_on_device(self, shots: int) -> bool:
        """Whenever a device is there - the rows are the same either way."""
        if self._seam_replaced() or not self._form.n_out:
            return False
        try:
            _lib.load(build=False)
            return _lib.device_count() > 0
        except Exception:  # noqa: BLE001 - no library / no device: the host statement is complete on its own
            return False

    def _sample_direct(self, shots: int) -> np.ndarray:
        if self._direct_on_device(shots):  # (post-selected requests of a component-free program come here)
            return self._direct_device(shots, None)
        return frame_rows_host(self._form, shots, 0, self._next_key()).view(np.bool_)

    def _direct_device(self, shots: int, batch_size: int | None, packed_columns: int | None = None, sink=None):
        """The request in chunks of whole 64-shot words (at most ``batch_size``, default 2^20, shots) under ONE key,
        ``first_shot`` running over the request; the handle cuts a chunk further where its record-flip scratch asks for it.
        ``sink`` (``count()``, ``sample_write()``) takes each chunk's padded bit-packed rows where they are; otherwise the
        leading ``packed_columns`` columns bit-packed, or all columns a byte each, are downloaded."""
        hp = self._hip()
        form = self._form
        n_out = form.n_out
        wo = (n_out + 63) // 64
        if packed_columns is not None and not 0 < packed_columns <= n_out:
            raise ValueError(f"packed_columns = {packed_columns} of {n_out} outputs")
        chunk = -(-min(shots, batch_size or (1 << 20), 1 << 20) // 64) * 64
        key = self._next_key()
        handle = self._frame_handle()
        if sink is not None:
            out, row_bytes, n_cols, packed = None, wo * 8, wo * 64, True
            s_sink = hp.aux_stream(1)
        elif packed_columns is not None:
            row_bytes, n_cols, packed = (packed_columns + 7) // 8, packed_columns, True
            out = np.empty((shots, row_bytes), dtype=np.uint8)
        else:
            row_bytes, n_cols, packed = n_out, n_out, False
            out = np.empty((shots, n_out), dtype=np.uint8)
        d_rows = self._scratch(hp, "frame_rows", chunk * row_bytes + 16)
        stream = hp.stream_ptr()
        for lo in range(0, shots, chunk):
            n = min(chunk, shots - lo)
            handle.sample_device(n, d_rows.ptr, key=key, first_shot=lo, out_row_bytes=row_bytes, out_packed=packed, n_cols=n_cols,
                                 stream=stream)
            hp.stream_synchronize(stream)
            if sink is not None:  # (the next chunk overwrites the rows: the sink finishes first)
                sink(d_rows.ptr, row_bytes, lo, lo + n, s_sink)
                hp.stream_synchronize(s_sink)
            else:
                hp.d2h(out[lo:lo + n], d_rows.ptr)
        if out is None:
            return None
        return out if packed_columns is not None else out.view(np.bool_)

    def __repr__(self) -> str:
        f = self._form
        return (f"{type(self).__name__}({f.n_out} outputs, {f.n_qubits} qubits, {f.n_records} records, {f.n_ops} frame operations in "
                f"{f.n_batches} batches, {len(f.site_chan)} noise sites, {f.n_random} random symbols)")


class CompiledFrameMeasurementSampler(_FrameSampler, CompiledMeasurementSampler):
    """A measurement sampler over the Pauli-frame form of a Clifford circuit (module docstring)."""

    def __init__(self, form: FrameForm, *, seed: int | None = None, device: int = 0, noise: str = "host"):
        if form.kind != "measurements":
            raise ValueError("a measurement sampler needs the form of compile_frame('measurements')")
        self._init_frame(form, seed, device, noise)

    def sample(self, shots: int, batch_size: int | None = None, bit_packed: bool = False) -> np.ndarray:
        """``bool[shots, num_measurements]``, or - ``bit_packed=True`` - ``uint8[shots, ceil(num_measurements / 8)]``
        little-endian bit rows.  For a fixed seed the rows do not depend on ``batch_size``."""
        _check_request(shots, batch_size)
        n_out = self._form.n_out
        if shots == 0:
            return np.empty((0, (n_out + 7) // 8), np.uint8) if bit_packed else np.empty((0, n_out), np.bool_)
        if self._direct_on_device(shots):
            return self._direct_device(shots, batch_size, packed_columns=n_out if bit_packed else None)
        rows = self._sample_direct(shots)
        return np.packbits(rows.view(np.uint8), axis=1, bitorder="little") if bit_packed else rows


class CompiledFrameDetectorSampler(_FrameSampler, CompiledDetectorSampler):
    """A detector sampler over the Pauli-frame form of a Clifford circuit: ``sample()``, ``count()`` and ``sample_write()`` of
    :class:`CompiledDetectorSampler` with every keyword; detectors whose random outcomes do not cancel are sampled too."""

    def __init__(self, form: FrameForm, *, seed: int | None = None, device: int = 0, noise: str = "host"):
        if form.kind != "detectors":
            raise ValueError("a detector sampler needs the form of compile_frame('detectors')")
        self._init_frame(form, seed, device, noise)

    @property
    def num_detectors(self) -> int:
        return self._num_detectors

    @property
    def num_observables(self) -> int:
        return self._form.n_out - self._num_detectors
