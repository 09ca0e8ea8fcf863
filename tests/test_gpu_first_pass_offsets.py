"""Row offsets and row stores of k_sample_lw_fast (tsim_lw_fast.hip.h): every row size, both f widths, every walk remainder.

The kernel splits a row's byte offsets into the thread's part, formed once per block, and the row block's part, formed on the
scalar unit in every trip and given to the stores as their scalar offset; the bit-packed store is straight-line code per row
size (out_rb = 1 .. 8: pieces of 4, 2 and 1 bytes at constant offsets), picked by a wave-uniform branch; the threshold walk
adds the compares' masks into `node` as carries.  A wrong piece, a wrong constant or a wrong split writes a byte it should not
or leaves one out: every output buffer carries sentinel bytes behind row B, and every row is compared bit for bit with the C
oracle and with the same call on a handle made under ``TSIM_AMD_TUNE=lw_fast=0`` (k_sample_lw_multi / k_sample_lw_reg) -
through ``tsim_sample_steps_device`` (1 and 3 steps: a block's consecutive trips change batch) and through the one-batch API.

Shapes (SHAPES): every out_rb 1 .. 8, chosen through n_direct, each with f rows of one and of two 64-bit words; n_out in
{1, 2, 3, 4, 5, 8} (every remainder of the three-level walk, and two full groups) spread over them; rows bit_packed and padded.
Batches: B in {1, 1023, 1024, 1025, 2049, 4097} (a lone row; one short of a row block of 1024, exactly one, one more; two and
a row; four and a row), shot offsets 0 (the batch has a check row), 1 and 2^32 - B (the range ends at the 32-bit boundary).

Tables of depth 2 (``pattern_tables=2``, never deepened) under p_bit = 0.037 on 24 selected bits, as in
test_gpu_first_pass_pairs.py: about 6 rows in 100 are hard.  Rows 1024, 2048 and 4096 - alone in the last row block of B = 1025,
2049 and 4097 - are made hard by hand (three selected bits set), and the host test below counts that every batch of every B has
a hard row in its first and in its last row block."""

import ctypes as C
import os

import numpy as np
import pytest

from tsim_amd import prng, synth

# name -> (n_out, num_f, n_direct): outputs = n_direct + n_out, out_rb = ceil(outputs / 8); num_f <= 64: one word, else two
SHAPES = {
    "rb1_f40_n1": (1, 40, 3),
    "rb2_f64_n4": (4, 64, 8),
    "rb3_f64_n5": (5, 64, 15),    # the benchmark's shape
    "rb4_f64_n2": (2, 64, 27),
    "rb5_f64_n3": (3, 64, 33),
    "rb6_f64_n8": (8, 64, 36),
    "rb7_f64_n1": (1, 64, 52),
    "rb8_f64_n4": (4, 64, 57),
    "rb1_f100_n2": (2, 100, 5),
    "rb2_f128_n3": (3, 128, 10),
    "rb3_f128_n8": (8, 128, 12),
    "rb4_f100_n5": (5, 100, 25),
    "rb5_f128_n1": (1, 128, 39),
    "rb6_f128_n4": (4, 128, 41),
    "rb7_f100_n5": (5, 100, 47),
    "rb8_f128_n8": (8, 128, 56),
}
F_SEL, DEPTH, P_BIT = 24, 2, 0.037
BATCHES = [1, 1023, 1024, 1025, 2049, 4097]
BMAX = max(BATCHES)
BLOCK = 1024  # rows of a row block
PLANTED = [1024, 2048, 4096]  # the lone rows of a last row block
STEPS = 3
KEY = prng.key(20261)
SENTINEL, TAIL = 0xA5, 64


def _out_rb(shape):
    return int(shape[2:3])


def _offsets(B):
    return [0, 1, (1 << 32) - B]


_PROG, _RIGS, _ORACLE, _FS = {}, {}, {}, {}


def _program(shape):
    if shape not in _PROG:
        n, nf, nd = SHAPES[shape]
        top = 6
        G = [max(1, round(top * (k + 1) / (n + 1))) for k in range(n + 1)]
        prog = synth.physical_program(num_f=nf, n_direct=nd, components=[dict(n=n, F=F_SEL, G=G)], seed=400 + n,
                                      direct_flip_fraction=0.3)
        assert (prog.num_outputs + 7) // 8 == _out_rb(shape)
        _PROG[shape] = prog
    return _PROG[shape]


def _f_batches(shape):
    """STEPS batches of BMAX rows, the PLANTED rows hard; a run of B rows takes their first B rows."""
    if shape not in _FS:
        n, nf, _ = SHAPES[shape]
        sel = np.asarray(_program(shape).components[0].f_selection)
        fs = []
        for i in range(STEPS):
            f = synth.synth_f(BMAX, nf, P_BIT, seed=8000 + 10 * n + nf + i).copy()
            for r in PLANTED:
                f[r, sel[i:i + DEPTH + 1]] = 1
            fs.append(f)
        _FS[shape] = fs
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
    """A handle of the shape with tables of depth DEPTH; `fast`: the default (k_sample_lw_fast), else lw_fast=0."""

    def __init__(self, hip, shape, fast):
        env = {"TSIM_AMD_TUNE": "shallow=0" + ("" if fast else ",lw_fast=0"), "TSIM_AMD_DEEP_TABLES": "-1"}
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
        self.rb = _out_rb(shape)
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


def _rig(hip, shape, fast):
    if (shape, fast) not in _RIGS:
        _RIGS[(shape, fast)] = _Rig(hip, shape, fast)
    return _RIGS[(shape, fast)]


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


def test_the_shapes_cover_what_they_claim():
    """Host only: every row size with both f widths, every walk remainder and two full groups."""
    seen = {(_out_rb(s), (nf + 63) // 64) for s, (_, nf, _) in SHAPES.items()}
    assert seen == {(rb, wf) for rb in range(1, 9) for wf in (1, 2)}
    assert {n for n, _, _ in SHAPES.values()} == {1, 2, 3, 4, 5, 8}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_batch_has_hard_rows_in_its_first_and_last_row_block(shape):
    """Host only: popcount of f & f_sel against the depth.  The lone row of B = 1 is hard where the batch has a check row."""
    for f in _f_batches(shape):
        heavy = _hard_rows(shape, f, False)
        assert 0.03 < heavy.mean() < 0.08  # (2048 x 0.08 = 164 rows in a list: the plan's "short lists" end at 192)
        for B in BATCHES:
            hard = _hard_rows(shape, f[:B], B == 1)
            last = (B - 1) // BLOCK * BLOCK
            assert hard[:BLOCK].any() and hard[last:B].any(), (shape, B)
            assert B == 1 or not hard[:B].all(), (shape, B)  # and easy rows beside them


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["bit_packed", "padded"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_equal_the_oracle_and_the_generic_pass(hip, shape, packed):
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
