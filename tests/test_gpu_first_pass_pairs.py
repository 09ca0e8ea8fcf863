"""The edges of k_sample_lw_fast's row walk (tsim_lw_fast.hip.h): row pairs, row blocks, counters and stores.

Written for a form of the kernel that held two adjacent rows per lane (row blocks of 2048 rows; measured slower than one row per
lane and not merged: profiles/first_pass_pairs.txt).  What it checks holds for either form, so it stays: one-component synthetic
programs through ``tsim_sample_steps_device`` and through the one-batch API, bit for bit against the C oracle and against the same
call on a handle made under ``TSIM_AMD_TUNE=lw_fast=0`` (k_sample_lw_multi / k_sample_lw_reg).

Shapes (SHAPES): n_out in {1, 2, 3, 5, 8} - every remainder of the three-level threshold walk, whose threshold reads the kernel
requests in front of its draws -, f rows of one and two 64-bit words, out_rb in {1, 3, 8} - odd row sizes, 8 for the second
word -, rows padded and bit_packed.  Batches: B in {1, 2, 3, 2047, 2048, 2049, 4097} (a lone row, a pair, an odd tail, one row
short of two row blocks of 1024, exactly two, one more, four and a row), 1 and 3 steps, shot offsets 0, 1 (odd first counter)
and 2^32 - B (the range ends at the 32-bit boundary).

The tables stop at weight 2 (``pattern_tables=2``: that depth, never deepened) under p_bit = 0.037 on 24 selected bits: about
6 rows in 100 are heavier than the tables go - as many as the launch plan still calls "short lists" (at most 192 rows per list),
so the group launcher stays in use - and the test counts on the host (popcount of f & f_sel against the depth) that every batch
holds pairs of adjacent rows with only the even row hard, only the odd row hard and both hard.  Every output buffer ends in
sentinel bytes behind row B; the parked-rows test reads a batch between its first pass and its hard-row kernel: the hard rows'
bytes are still the sentinel's."""

import ctypes as C
import os

import numpy as np
import pytest

from tsim_amd import prng, synth

# name -> (n_out, num_f, n_direct): outputs = n_direct + n_out
SHAPES = {
    "n1_f40_rb1": (1, 40, 3),     # 4 outputs: 1 byte; a pair is one short
    "n2_f100_rb3": (2, 100, 20),  # 22 outputs: 3 bytes, f rows of two words
    "n3_f64_rb8": (3, 64, 61),    # 64 outputs: 8 bytes, the second output word
    "n5_f64_rb3": (5, 64, 15),    # the benchmark's shape: 20 outputs, a pair is a word and a short
    "n8_f128_rb8": (8, 128, 56),  # 64 outputs, f rows of two words
}
OUT_RB = {"n1_f40_rb1": 1, "n2_f100_rb3": 3, "n3_f64_rb8": 8, "n5_f64_rb3": 3, "n8_f128_rb8": 8}
F_SEL, DEPTH, P_BIT = 24, 2, 0.037
BATCHES = [1, 2, 3, 2047, 2048, 2049, 4097]
BMAX = max(BATCHES)
STEPS = 3
KEY = prng.key(20260)
SENTINEL, TAIL = 0xA5, 64


def _offsets(B):
    return [0, 1, (1 << 32) - B]


_PROG, _RIGS, _ORACLE, _FS = {}, {}, {}, {}


def _program(shape):
    if shape not in _PROG:
        n, nf, nd = SHAPES[shape]
        top = 6
        G = [max(1, round(top * (k + 1) / (n + 1))) for k in range(n + 1)]
        prog = synth.physical_program(num_f=nf, n_direct=nd, components=[dict(n=n, F=F_SEL, G=G)], seed=300 + n,
                                      direct_flip_fraction=0.3)
        assert (prog.num_outputs + 7) // 8 == OUT_RB[shape]
        _PROG[shape] = prog
    return _PROG[shape]


def _f_batches(shape):
    """STEPS batches of BMAX rows; a run of B rows takes their first B rows."""
    if shape not in _FS:
        nf = SHAPES[shape][1]
        _FS[shape] = [synth.synth_f(BMAX, nf, P_BIT, seed=7000 + 10 * SHAPES[shape][0] + i) for i in range(STEPS)]
    return _FS[shape]


def _hard_rows(shape, f, check_row):
    """Rows the first pass must leave to the hard-row kernel: more selected bits than the tables hold, and the check row."""
    sel = np.asarray(_program(shape).components[0].f_selection)
    hard = f[:, sel].sum(axis=1) > DEPTH
    if check_row and len(hard):
        hard = hard.copy()
        hard[0] = True
    return hard


def _packed_f(f, wf):
    p = np.packbits(f, axis=1, bitorder="little")
    return np.ascontiguousarray(np.pad(p, ((0, 0), (0, wf * 8 - p.shape[1]))))


class _Rig:
    """A handle of the shape with tables of depth DEPTH; `pairs`: the default (k_sample_lw_fast), else lw_fast=0."""

    def __init__(self, hip, shape, pairs):
        env = {"TSIM_AMD_TUNE": "shallow=0" + ("" if pairs else ",lw_fast=0"), "TSIM_AMD_DEEP_TABLES": "-1"}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.prog = _program(shape)
            self.hp = hip.HipProgram(self.prog, pattern_tables=DEPTH)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        assert self.hp.info()["pattern_max_weight"] == [DEPTH]
        self.nf = SHAPES[shape][1]
        self.wf = (self.nf + 63) // 64
        self.rb = OUT_RB[shape]
        fs = _f_batches(shape)
        self.d_f = {}
        for B in BATCHES:  # a buffer of exactly B rows: what the kernel's descriptor ends with
            self.d_f[B] = [self.hp.malloc(B * self.wf * 8) for _ in range(STEPS)]
            for d, f in zip(self.d_f[B], fs):
                self.hp.h2d(d, _packed_f(f[:B], self.wf))
        self.d_o = [self.hp.malloc(BMAX * 8 + TAIL) for _ in range(STEPS)]
        # launch-plan feedback: the group launcher runs once earlier launches have reported short hard-row lists
        for _ in range(3):
            self.steps(2049, 3, 0, True)
        self.hp.path_counts(reset=True)

    def _fill(self, n):
        blank = np.full(BMAX * 8 + TAIL, SENTINEL, np.uint8)
        for d in self.d_o[:n]:
            self.hp.h2d(d, blank)

    def _read(self, n, B, packed):
        """Rows of the first n buffers as bit-packed rows; the bytes behind row B must be the sentinel's."""
        rows = []
        width = self.rb if packed else 8
        for d in self.d_o[:n]:
            raw = np.zeros(BMAX * 8 + TAIL, np.uint8)
            self.hp.d2h(raw, d)
            assert (raw[B * width:] == SENTINEL).all(), f"bytes behind row {B} were written"
            rows.append(raw[:B * width].reshape(B, width)[:, :self.rb].copy())
            if not packed:
                assert not raw[:B * 8].reshape(B, 8)[:, self.rb:].any()  # the padding of a padded row is zero
        return rows

    def steps(self, B, n, shot_offset, packed):
        self._fill(n)
        ks = (C.c_uint32 * 2)(int(KEY[0]) & 0xFFFFFFFF, int(KEY[1]) & 0xFFFFFFFF)
        self.hp.sample_steps_device([d.ptr for d in self.d_f[B][:n]], B, self.nf, ks, [d.ptr for d in self.d_o[:n]],
                                    shot_offset=shot_offset, out_bit_packed=packed)
        self.hp.synchronize()
        return self._read(n, B, packed)

    def one_batch(self, B, sub, shot_offset, packed):
        self._fill(1)
        if packed:
            self.hp.sample_batch_device_begin(0, self.d_f[B][0].ptr, B, self.nf, sub, self.d_o[0].ptr, shot_offset=shot_offset,
                                              out_bit_packed=True)
            self.hp.sample_batch_device_end(0)
        else:
            self.hp.sample_batch_device(self.d_f[B][0].ptr, B, self.nf, sub, self.d_o[0].ptr, shot_offset=shot_offset)
        self.hp.synchronize()
        return self._read(1, B, packed)[0]


def _rig(hip, shape, pairs):
    if (shape, pairs) not in _RIGS:
        _RIGS[(shape, pairs)] = _Rig(hip, shape, pairs)
    return _RIGS[(shape, pairs)]


def _subkeys():
    key, subs = KEY, []
    for _ in range(STEPS):
        key, sub = prng.split(key)
        subs.append(sub)
    return subs


def _oracle_rows(shape, B, shot_offset):
    """The STEPS batches of B rows at this offset, bit-packed rows (shared by both output forms and both step counts)."""
    from oracle import oracle_c as OC

    k = (shape, B, shot_offset)
    if k not in _ORACLE:
        if shape not in _ORACLE:
            _ORACLE[shape] = OC.OracleProgram(_program(shape))
        rows = []
        for f, sub in zip(_f_batches(shape), _subkeys()):
            want = _ORACLE[shape].sample_program(f[:B], sub, shot_offset=shot_offset)
            rows.append(np.packbits(want, axis=1, bitorder="little"))
        _ORACLE[k] = rows
    return _ORACLE[k]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_batches_hold_every_kind_of_pair(shape):
    """Host only: the rows the runs below go through hold pairs with only row A hard, only row B hard, both and neither - in
    the first 2047 rows already, and the odd last row of 2049 and 4097 is decided on its own."""
    for f in _f_batches(shape):
        hard = _hard_rows(shape, f[:2046], False)
        a, b = hard[0::2], hard[1::2]
        kinds = {"A": int((a & ~b).sum()), "B": int((~a & b).sum()), "both": int((a & b).sum()), "neither": int((~a & ~b).sum())}
        print(shape, kinds)
        assert all(v >= 1 for v in kinds.values()), kinds
    hard = _hard_rows(shape, _f_batches(shape)[0], False)
    assert 0.03 < hard.mean() < 0.08  # (2048 x 0.08 = 164 rows in a list: the plan's "short lists" end at 192)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["bit_packed", "padded"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pairs_equal_the_oracle_and_one_row_per_lane(hip, shape, packed):
    rig, ref = _rig(hip, shape, True), _rig(hip, shape, False)
    subs = _subkeys()
    rig.hp.path_counts(reset=True)
    ref.hp.path_counts(reset=True)
    for B in BATCHES:
        for shot_offset in _offsets(B):
            want = _oracle_rows(shape, B, shot_offset)
            for n in (1, 3):
                got = rig.steps(B, n, shot_offset, packed)
                other = ref.steps(B, n, shot_offset, packed)
                for j in range(n):
                    tag = f"B {B} offset {shot_offset} steps {n} batch {j}"
                    np.testing.assert_array_equal(got[j], want[j], err_msg=tag + " against the oracle")
                    np.testing.assert_array_equal(got[j], other[j], err_msg=tag + " against lw_fast=0")
            got = rig.one_batch(B, subs[0], shot_offset, packed)
            tag = f"B {B} offset {shot_offset} one batch"
            np.testing.assert_array_equal(got, want[0], err_msg=tag + " against the oracle")
            np.testing.assert_array_equal(got, ref.one_batch(B, subs[0], shot_offset, packed), err_msg=tag + " against lw_fast=0")
    paths, ref_paths = rig.hp.path_counts(), ref.hp.path_counts()
    print(shape, "paths", paths, "lw_fast=0:", ref_paths)
    # the kernel under test ran, as a group and as a group of one, and the other handle never ran it
    assert paths.get("lw_fast", 0) > 0 and paths.get("lw_fast1", 0) > 0, paths
    assert not {"lw_multi", "lw_reg", "lw_lds", "gen"} & set(paths), paths
    assert not {"lw_fast", "lw_fast1"} & set(ref_paths), ref_paths


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["bit_packed", "padded"])
@pytest.mark.parametrize("shape", ["n5_f64_rb3", "n8_f128_rb8"])
def test_the_first_pass_leaves_the_hard_rows_alone(hip, shape, packed):
    """A pipelined launch whose plan parks the hard rows (tsim_sample_batch_device_begin without its _end): once the first
    pass is through, every easy row holds its result and every hard row - alone in its pair, or both rows of it - still holds
    the sentinel; _end brings the hard rows."""
    rig = _rig(hip, shape, True)
    hp, B = rig.hp, 4097
    sub = _subkeys()[0]
    width = rig.rb if packed else 8
    want = _oracle_rows(shape, B, 0)[0]
    hard = _hard_rows(shape, _f_batches(shape)[0][:B], True)
    a, b = hard[0:B - 1:2], hard[1:B:2]
    assert (a & ~b).any() and (~a & b).any() and (a & b).any()

    def launch():
        rig._fill(1)
        hp.path_counts(reset=True)
        hp.sample_batch_device_begin(0, rig.d_f[B][0].ptr, B, rig.nf, sub, rig.d_o[0].ptr, out_bit_packed=packed)
        hp.stream_synchronize(hp.pipeline_lane_stream(0))  # slot 0's first pass runs on lane 0
        paths = hp.path_counts()
        raw = np.zeros(BMAX * 8 + TAIL, np.uint8)
        hp.d2h(raw, rig.d_o[0])
        hp.sample_batch_device_end(0)
        hp.synchronize()
        return paths, raw[:B * width].reshape(B, width), raw[B * width:]

    for _ in range(3):  # launch-plan feedback of this very call
        launch()
    paths, mid, tail = launch()
    print(shape, "paths before _end:", paths, "hard rows:", int(hard.sum()))
    assert paths == {"lw_fast1": 1}, paths  # the first pass alone: the hard rows wait for _end
    assert (tail == SENTINEL).all()
    assert (mid[hard] == SENTINEL).all(), "the first pass wrote into a hard row"
    np.testing.assert_array_equal(mid[~hard][:, :rig.rb], want[~hard])
    done = rig._read(1, B, packed)[0]
    np.testing.assert_array_equal(done, want)
