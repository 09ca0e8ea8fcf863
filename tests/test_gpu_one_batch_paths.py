"""The routes of the one-batch launcher (``launch_sample``, ``launch_hw``, ``launch_over``, ``flush_batch``), one
case per route.  The steps tests send almost every batch through a group launcher; here a batch goes through
``sample_batch_device`` (rows padded) or one ``sample_batch_device_begin`` / ``_end`` (rows bit-packed: the entry that writes
them), the deferred cases through several slots of ``_begin`` before their ``_end``, the row-index case through
``sample_rows_device``.

Every case: B = 2500 shots (three row blocks of 1024 with the last partial, 40 tiles of 64 with the last partial), shot offsets
0 and 3 << 20 (check row present and absent), rows bit-packed and padded.  The rows equal the C oracle's with the same subkey
and shot offset, and ``path_counts()`` of the measured call(s) equals the literal dictionary in ROUTES, recorded on the parent
commit of the refactor that made launch_sample its stages (three consecutive runs, equal in every case).  The tables are pinned
as in tests/test_gpu_steps_groups.py (``_handle`` there says why) and the plan is warmed by three calls of the very kind that
is measured, so it does not move.

Not reachable from these entries: the component-parallel hard rows (``partial``), which only a fused group of
``k_sample_lw_fastm`` leaves (tests/test_gpu_steps_protocol.py, ``lw_fastm``); C4 here is the three-component program on
``k_sample_lw_reg`` and the block-per-row kernel."""

import os
import warnings

import numpy as np
import pytest

from tsim_amd import synth

pytestmark = pytest.mark.gpu

B = 2500
OFFSETS = [0, 3 << 20]
KEYS = [(4321 + i, 17 + i) for i in range(8)]
WARM = 3
N_LISTED = 100

# route -> (program, TSIM_AMD_TUNE, constructor arguments, other environment, entry, path counts of the measured call(s))
# entry: "batch" - one call; "defer" - two slots of _begin, then their _end; "rows" - sample_rows_device with 100 listed rows.
# "batch" cases get defer_hard=0 besides: their bit-packed variant enters through _begin, which must not park its hard rows.
ROUTES = {
    "wide_group_of_one": ("1wide", "", {}, {}, "batch", {'wide': 1}),
    "lw_fast1_hw": ("C2", "", {}, {}, "batch", {'lw_fast1': 1, 'hw': 1}),
    "lw_reg": ("C2", "lw_fast=0", {}, {}, "batch", {'lw_reg': 1, 'hw': 1}),
    "lw_lds_f160": ("f160", "gen=0", {}, {}, "batch", {'lw_lds': 1, 'hw': 1}),
    "lw_lds_out65": ("out65", "gen=0", {}, {}, "batch", {'lw_lds': 1, 'hw': 1}),
    "lw_lds_wide_sample4w_lists": ("2wide", "wide_fused=0", {}, {}, "batch", {'lw_lds_wide': 1, 'sample4w': 1, 'rows': 1}),
    "sample4w_every_row": ("2wide", "", {"pattern_tables": False}, {}, "batch", {'sample4w': 1, 'rows': 1}),
    "gen_one_n13": ("n13", "", {}, {}, "batch", {'hw': 1, 'gen': 1}),
    "sample4_alone": ("C2", "", {"pattern_tables": False}, {}, "batch", {'sample4': 1}),
    "sample4h_over": ("C2", "hard_wave=0", {}, {}, "batch", {'lw_fast1': 1, 'sample4h': 1, 'over': 1}),
    "sample4h_alone": ("C2", "hard_wave=0,hard_overflow=0", {}, {}, "batch", {'lw_fast1': 1, 'sample4h': 1}),
    "sample4h_sample4": ("C2", "hard_wave=0", {}, {"TSIM_AMD_ADAPTIVE": "0"}, "batch", {'lw_fast1': 1, 'sample4': 1, 'sample4h': 1}),  # no feedback: the overflow launch stays
    "defer_4h_multi_group1": ("C2", "hard_wave=0,defer_group=1", {}, {}, "defer", {'lw_fast1': 2, 'sample4h_multi': 2}),
    "defer_4h_multi": ("C2", "hard_wave=0", {}, {}, "defer", {'lw_fast1': 2, 'sample4h_multi': 1}),
    "defer_hw_group1": ("C2", "hard_wave=1,defer_group=1", {}, {}, "defer", {'lw_fast1': 2, 'hw': 2}),
    "defer_hw": ("C2", "hard_wave=1", {}, {}, "defer", {'lw_fast1': 2, 'hw': 1}),
    "three_components_C4": ("C4", "", {}, {}, "batch", {'lw_reg': 1, 'hw': 1}),
    "many_hard_rows_F70": ("F70", "defer_group=8", {}, {}, "defer", {'over': 1, 'sample4h_multi': 1, 'gen': 8}),
    "hw_4_20_F60": ("F60", "", {}, {}, "batch", {'lw_fast1': 1, 'hw': 1}),
    "hw_8_0_F140": ("F140", "", {}, {}, "batch", {'lw_lds_wide': 1, 'sample4w': 1, 'hw': 1}),
    "row_kernel": ("C2", "", {"mode": "faithful"}, {"TSIM_AMD_KERNEL": "rows"}, "batch", {'rows': 1}),
    "row_index": ("C2", "", {}, {}, "rows", {'lw_fast1': 1, 'hw': 1}),
}
# F70: hard rows are "many" beyond 16384 per batch of launches (flush_batch: k_sample4_over as a grid of its own), which
# 2 x 2500 rows cannot hold: eight slots of 2^15 rows, and p_bit raised from 0.02 until the parent took the branch (0.024 and
# 0.028 do; at 0.02 the workers stay inside the latency grid, from 0.032 the plan no longer parks the rows)
SHAPE = {"many_hard_rows_F70": dict(B=1 << 15, slots=8, p_bit=0.026)}


def _program(name):
    if name in synth.CONFIGS:
        return synth.config_program(name)
    return synth.shape_class_program(name)


_RIGS = {}
_ORACLE = {}


class _Rig:
    """One handle with an f buffer and an output buffer per slot."""

    def __init__(self, hip, route):
        name, tune, ctor, extra, self.entry, self.paths = ROUTES[route]
        if self.entry == "batch":
            tune = (tune + "," if tune else "") + "defer_hard=0"
        env = dict(extra, TSIM_AMD_TUNE=(tune + "," if tune else "") + "shallow=0", TSIM_AMD_DEEP_TABLES="-1", TSIM_AMD_PATTERN_TABLE_MB="64")
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.prog, cfg = _program(name)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.hp = hip.HipProgram(self.prog, **ctor)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.route = route
        self.name = name
        self.nf = cfg["num_f"]
        shape = SHAPE.get(route, {})
        self.B = shape.get("B", B)
        self.slots = shape.get("slots", 2) if self.entry == "defer" else 1
        self.p_bit = shape.get("p_bit") or cfg["p_bit"]
        self.wf = max(1, (self.nf + 63) // 64)
        self.rb = (self.prog.num_outputs + 7) // 8
        self.wo = (self.prog.num_outputs + 63) // 64
        self.f = [synth.synth_f(self.B, self.nf, self.p_bit, seed=6100 + i) for i in range(self.slots)]
        self.d_f = [self.hp.malloc(self.B * self.wf * 8) for _ in range(self.slots)]
        self.d_o = [self.hp.malloc(self.B * self.wo * 8) for _ in range(self.slots)]
        for d, f in zip(self.d_f, self.f):
            p = np.packbits(f, axis=1, bitorder="little")
            self.hp.h2d(d, np.ascontiguousarray(np.pad(p, ((0, 0), (0, self.wf * 8 - p.shape[1])))))
        rng = np.random.default_rng(77)
        self.listed = np.sort(np.concatenate([[0], 1 + rng.choice(self.B - 1, N_LISTED - 1, replace=False)])).astype(np.uint32)
        self.d_idx = self.hp.malloc(N_LISTED * 4)
        self.d_cnt = self.hp.malloc(4)
        self.hp.h2d(self.d_idx, self.listed)
        self.hp.h2d(self.d_cnt, np.array([N_LISTED], np.uint32))

    def call(self, shot_offset, packed):
        """The route's call(s); the rows of the batches it made."""
        hp = self.hp
        n = self.slots
        zero = np.zeros((self.B, self.wo * 8), np.uint8)
        for i in range(n):
            hp.h2d(self.d_o[i], zero)
        if self.entry == "rows":
            hp.sample_rows_device(self.d_f[0].ptr, self.B, self.nf, KEYS[0], self.d_o[0].ptr, self.d_idx.ptr, self.d_cnt.ptr, shot_offset=shot_offset)
        elif self.entry == "batch" and not packed:
            hp.sample_batch_device(self.d_f[0].ptr, self.B, self.nf, KEYS[0], self.d_o[0].ptr, shot_offset=shot_offset)
        else:
            for i in range(n):
                hp.sample_batch_device_begin(i, self.d_f[i].ptr, self.B, self.nf, KEYS[i], self.d_o[i].ptr, shot_offset=shot_offset,
                                             out_bit_packed=packed)
            for i in range(n):
                hp.sample_batch_device_end(i)
        hp.synchronize()
        rows = []
        for i in range(n):
            got = np.zeros((self.B, self.rb if packed else self.wo * 8), np.uint8)
            hp.d2h(got, self.d_o[i])
            rows.append(got)
        return rows

    def measure(self, shot_offset, packed):
        for _ in range(WARM):  # launch-plan feedback of this very call
            self.call(shot_offset, packed)
        self.hp.path_counts(reset=True)
        rows = self.call(shot_offset, packed)
        return rows, self.hp.path_counts()


def _rig(hip, route):
    if route not in _RIGS:
        _RIGS[route] = _Rig(hip, route)
    return _RIGS[route]


def _oracle_rows(rig, i, shot_offset):
    from oracle import oracle_c as OC

    k = (rig.name, rig.p_bit, i, shot_offset)
    if k not in _ORACLE:
        if rig.name not in _ORACLE:
            _ORACLE[rig.name] = OC.OracleProgram(rig.prog)
        want = _ORACLE[rig.name].sample_program(rig.f[i], KEYS[i], shot_offset=shot_offset)
        _ORACLE[k] = np.packbits(want, axis=1, bitorder="little")
    return _ORACLE[k]


def _variants(route):
    # the row-index entry writes padded rows only
    return [False] if ROUTES[route][4] == "rows" else [True, False]


@pytest.mark.parametrize("route,shot_offset,packed", [(r, o, pk) for r in ROUTES for o in OFFSETS for pk in _variants(r)],
                         ids=lambda v: {True: "packed", False: "padded"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_one_batch_route_equals_the_oracle_and_keeps_its_launches(hip, route, shot_offset, packed):
    rig = _rig(hip, route)
    rows, paths = rig.measure(shot_offset, packed)
    print(f"ROUTE {route!r} {(shot_offset != 0, packed)!r} {paths!r}")
    for i, got in enumerate(rows):
        want = _oracle_rows(rig, i, shot_offset)
        if rig.entry == "rows":  # the listed rows only (the register first pass writes the others too, as the oracle has them)
            keep = np.zeros(rig.B, bool)
            keep[rig.listed] = True
            np.testing.assert_array_equal(got[keep][:, :rig.rb], want[keep], err_msg=f"listed rows of batch {i}")
        else:
            np.testing.assert_array_equal(got[:, :rig.rb], want, err_msg=f"batch {i} against the oracle")
        assert not got[:, rig.rb:].any()
    assert paths == rig.paths, paths
