"""The draws of k_sample_lw_fast (tsim_lw_fast.hip.h) at every place where their key, counter or position in the row loop
changes: written with the kernel's Threefry block (profiles/threefry_schedule.txt) and true of any form of it.

Everything goes through ``tsim_sample_steps_device`` and is compared bit for bit with the C oracle and with the same call on a
handle made under ``TSIM_AMD_TUNE=lw_fast=0`` (k_sample_lw_multi, whose draws run the other asm block, threefry_bits32 of
tsim_kernels.hip.h).

  * keys by step: one call of 32 batches of B = 2500 rows under ``fused_max=16:2500`` - the schedule's groups are 16, 8, 8
    (checked on the host), every batch has its own subkey, a batch is three row blocks of 1024 and the last is partial;
  * B = 1 (one lane) and B = 1025 (one full block and one row);
  * components of 1, 2, 3, 5 and 8 outputs - the three-level threshold walk leaves 1, 2, 0, 2, 2 draws to its remainder - on f rows
    of 64 and of 128 bits, 3000 rows;
  * shot offsets 0 (the check row is there), 2^32 + 5 (the counter's high word is not zero) and 2^32 - B - 1 (the largest low
    word with which shot_offset + B still stays below the next 2^32, which is what this kernel is launched for);
  * a key base that is not zero: the packer gives a program's only component key base 0 (lay_out_component, tsim_finalize.hip),
    so k_sample_lw_fast never sees another; a program with a component of three outputs in front of one of five has key base 3
    in its second record and runs the several-component pass on the same draw (threefry_bits32_lo).

The tables stop at weight 2 under p_bit = 0.037 on 24 selected bits (16 per component in the two-component program), as in
tests/test_gpu_first_pass_pairs.py: some 6 rows in 100 are hard, the group launcher stays in use."""

import ctypes as C
import os

import numpy as np
import pytest

from tsim_amd import _lib, prng, synth

# name -> (n_out, num_f, n_direct)
SHAPES = {
    "n1_f40": (1, 40, 3),
    "n2_f100": (2, 100, 20),
    "n3_f64": (3, 64, 61),
    "n5_f64": (5, 64, 15),  # the benchmark's shape
    "n8_f128": (8, 128, 56),
}
F_SEL, DEPTH, P_BIT = 24, 2, 0.037
KEY = prng.key(50211)
B_GROUP, N_GROUP, NF_BUFS = 2500, 32, 4
B_WIDTH = 3000
TUNE_GROUPS = "fused_max=16:2500,shallow=0"
TUNE_PLAIN = "shallow=0"

_PROG, _RIGS, _ORACLE, _F = {}, {}, {}, {}


def _graphs(n, top=6):
    return [max(1, round(top * (k + 1) / (n + 1))) for k in range(n + 1)]


def _program(shape):
    if shape not in _PROG:
        if shape == "two_components":
            _PROG[shape] = synth.physical_program(num_f=64, n_direct=12, seed=411, direct_flip_fraction=0.3,
                                                  components=[dict(n=3, F=16, G=_graphs(3)), dict(n=5, F=16, G=_graphs(5))])
        else:
            n, nf, nd = SHAPES[shape]
            _PROG[shape] = synth.physical_program(num_f=nf, n_direct=nd, components=[dict(n=n, F=F_SEL, G=_graphs(n))],
                                                  seed=300 + n, direct_flip_fraction=0.3)
    return _PROG[shape]


def _num_f(shape):
    return 64 if shape == "two_components" else SHAPES[shape][1]


def _f_batches(shape, B, count):
    """`count` batches of B rows (the same arrays for every handle and for the oracle)."""
    k = (shape, B)
    if k not in _F or len(_F[k]) < count:
        _F[k] = [synth.synth_f(B, _num_f(shape), P_BIT, seed=9100 + 17 * i + B) for i in range(count)]
    return _F[k][:count]


def _subkeys(n):
    key, subs = KEY, []
    for _ in range(n):
        key, sub = prng.split(key)
        subs.append(sub)
    return subs


def _oracle_rows(shape, B, shot_offset, n, nf_bufs):
    """Batches 0 .. n - 1 of the key chain, batch j on f batch j % nf_bufs, as bit-packed rows; computed once."""
    from oracle import oracle_c as OC

    k = (shape, B, shot_offset, n, nf_bufs)
    if k not in _ORACLE:
        if shape not in _ORACLE:
            _ORACLE[shape] = OC.OracleProgram(_program(shape))
        fs = _f_batches(shape, B, nf_bufs)
        _ORACLE[k] = [np.packbits(_ORACLE[shape].sample_program(fs[j % nf_bufs], sub, shot_offset=shot_offset), axis=1,
                                  bitorder="little") for j, sub in enumerate(_subkeys(n))]
    return _ORACLE[k]


class _Rig:
    """One handle of the shape with tables of depth DEPTH, made under `tune`; buffers per (B, count) on demand."""

    def __init__(self, hip, shape, tune):
        env = {"TSIM_AMD_TUNE": tune, "TSIM_AMD_DEEP_TABLES": "-1"}
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
        self.shape = shape
        self.nf = _num_f(shape)
        self.wf = (self.nf + 63) // 64
        self.rb = (self.prog.num_outputs + 7) // 8
        self.d_f, self.d_o = {}, {}
        for _ in range(3):  # launch-plan feedback: the group launcher runs once earlier launches have reported short lists
            self.steps(2049, 3, 3, 0)
        self.hp.path_counts(reset=True)

    def steps(self, B, n, nf_bufs, shot_offset):
        """One call of n batches of B rows, batch j on f batch j % nf_bufs; the n batches' bit-packed rows."""
        if (B, nf_bufs) not in self.d_f:
            bufs = [self.hp.malloc(B * self.wf * 8) for _ in range(nf_bufs)]  # exactly B rows: what the kernel's descriptor ends with
            for d, f in zip(bufs, _f_batches(self.shape, B, nf_bufs)):
                p = np.packbits(f, axis=1, bitorder="little")
                self.hp.h2d(d, np.ascontiguousarray(np.pad(p, ((0, 0), (0, self.wf * 8 - p.shape[1])))))
            self.d_f[(B, nf_bufs)] = bufs
        while len(self.d_o.setdefault(B, [])) < n:
            self.d_o[B].append(self.hp.malloc(B * 8))
        ks = (C.c_uint32 * 2)(int(KEY[0]) & 0xFFFFFFFF, int(KEY[1]) & 0xFFFFFFFF)
        self.hp.sample_steps_device([self.d_f[(B, nf_bufs)][j % nf_bufs].ptr for j in range(n)], B, self.nf, ks,
                                    [d.ptr for d in self.d_o[B][:n]], shot_offset=shot_offset, out_bit_packed=True)
        self.hp.synchronize()
        rows = []
        for d in self.d_o[B][:n]:
            got = np.zeros((B, self.rb), np.uint8)
            self.hp.d2h(got, d)
            rows.append(got)
        return rows


def _rig(hip, shape, tune):
    if (shape, tune) not in _RIGS:
        _RIGS[(shape, tune)] = _Rig(hip, shape, tune)
    return _RIGS[(shape, tune)]


def _compare(hip, shape, tune, B, n, nf_bufs, shot_offset, fast_paths=("lw_fast", "lw_fast1")):
    rig, ref = _rig(hip, shape, tune), _rig(hip, shape, tune + ",lw_fast=0")
    rig.hp.path_counts(reset=True)
    ref.hp.path_counts(reset=True)
    got = rig.steps(B, n, nf_bufs, shot_offset)
    other = ref.steps(B, n, nf_bufs, shot_offset)
    want = _oracle_rows(shape, B, shot_offset, n, nf_bufs)
    paths, ref_paths = rig.hp.path_counts(), ref.hp.path_counts()
    print(f"{shape} B {B} batches {n} offset {shot_offset}: paths {paths}, lw_fast=0: {ref_paths}")
    for j in range(n):
        tag = f"{shape} B {B} offset {shot_offset} batch {j} of {n}"
        np.testing.assert_array_equal(got[j], want[j], err_msg=tag + " against the oracle")
        np.testing.assert_array_equal(got[j], other[j], err_msg=tag + " against lw_fast=0")
    if fast_paths:
        assert set(fast_paths) & set(paths), paths  # the kernel under test ran ...
        assert not {"lw_multi", "lw_reg", "lw_lds", "gen"} & set(paths), paths
    assert not {"lw_fast", "lw_fast1"} & set(ref_paths), ref_paths  # ... and the other handle never ran it
    return paths


def test_the_schedule_of_the_group_case():
    """Host only: 32 batches of 2500 rows under fused_max=16:2500 are groups of 16, 8 and 8; the 32 subkeys are distinct."""
    lib = _lib.load()
    groups, left = [], N_GROUP
    while left > 0:
        g = lib.tsim_steps_next_group(left, B_GROUP, 16, 2500)
        groups.append(g)
        left -= g
    assert groups == [16, 8, 8], groups
    subs = {(int(s[0]), int(s[1])) for s in _subkeys(N_GROUP)}
    assert len(subs) == N_GROUP
    assert B_GROUP % 1024 not in (0, 1)  # the last row block is partial and holds more than a row


@pytest.mark.gpu
def test_groups_of_sixteen_batches_draw_with_their_own_keys(hip):
    paths = _compare(hip, "n5_f64", TUNE_GROUPS, B_GROUP, N_GROUP, NF_BUFS, 0, fast_paths=("lw_fast",))
    assert "lw_fast" in paths, paths  # as a group, not batch by batch


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 1025])
@pytest.mark.parametrize("shape", ["n5_f64", "n8_f128"])
def test_one_lane_and_one_block_and_a_row(hip, shape, B):
    for n in (1, 3):
        _compare(hip, shape, TUNE_PLAIN, B, n, 3, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_component_widths_and_row_widths(hip, shape):
    n_out, nf, _ = SHAPES[shape]
    assert (n_out % 3, (nf + 63) // 64) == {"n1_f40": (1, 1), "n2_f100": (2, 2), "n3_f64": (0, 1), "n5_f64": (2, 1),
                                            "n8_f128": (2, 2)}[shape]
    _compare(hip, shape, TUNE_PLAIN, B_WIDTH, 3, 3, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", ["high_word", "largest_low_word", "zero"])
@pytest.mark.parametrize("shape", ["n5_f64", "n8_f128"])
def test_shot_offsets(hip, shape, offset):
    B = 2500
    shot_offset = {"high_word": (1 << 32) + 5, "largest_low_word": (1 << 32) - B - 1, "zero": 0}[offset]
    assert shot_offset + B < ((shot_offset >> 32) + 1) << 32  # the whole batch inside one value of the high word
    _compare(hip, shape, TUNE_PLAIN, B, 3, 3, shot_offset)


@pytest.mark.gpu
def test_a_key_base_that_is_not_zero(hip):
    """Two components: the second one's keys start behind the first one's three.  Not k_sample_lw_fast (see the module's text)."""
    prog = _program("two_components")
    assert [len(c.output_indices) for c in prog.components] == [3, 5]
    for shot_offset in (0, (1 << 32) + 5):
        paths = _compare(hip, "two_components", TUNE_PLAIN, 2500, 3, 3, shot_offset, fast_paths=())
        assert not {"lw_fast", "lw_fast1"} & set(paths), paths
