"""Fused groups of up to 16 batches with ONE hard-row grid, and the group schedule of ``tsim_sample_steps_device``
(``tsim_steps_next_group``): whatever the call pattern, the rows and the key state are those of the groups of at most 8
(``TSIM_AMD_TUNE=fused_max=8``), of the batch-by-batch path (``TSIM_AMD_FUSED_STEPS=0``) and of the C oracle.

Every GPU case: the C2 program, B = 2500 shots (three row blocks of 1024, the last one partial), 32 rotating output buffers,
4 rotating f buffers, bit-packed rows.  ``fused_max=16:1`` lowers the schedule's shot threshold (2^23 by default) so that
groups of 16 x 2500 shots count as long ones.  Two noise levels: p_bit = 0.02 (hardly a hard row but the check row) and 0.08
(some 3 % of the rows are heavier than the tables go: hundreds of hard rows per group of 16).  The tables stay what they are
(``TSIM_AMD_PATTERN_TABLE_MB=64``, ``TSIM_AMD_DEEP_TABLES=-1``, ``shallow=0``): see ``_handle`` for why that, and not
``TSIM_AMD_ADAPTIVE=0``, pins them."""

import ctypes as C
import os

import numpy as np
import pytest

from tsim_amd import _lib, prng, synth

B = 2500
NOUT_BUFS, NF_BUFS = 32, 4
KEY = prng.key(1234)
PATTERNS = [[1], [8], [9], [16], [17], [31], [32], [33], [48], [70], [4, 4, 16, 40, 3]]
OFFSETS = [0, 3 << 20]
TUNE_LONG = "fused_max=16:1,shallow=0"
TUNE_8 = "fused_max=8,shallow=0"


def _parent_groups(k, gmax=8):
    """The rule before the long groups: even groups, as few as possible, of at most gmax."""
    out, left = [], k
    while left > 0:
        groups = -(-left // gmax)
        n = -(-left // groups)
        out.append(n)
        left -= n
    return out


def _groups(lib, k, b, fused_max=16, long_shots=1 << 23):
    out, left = [], k
    while left > 0:
        n = lib.tsim_steps_next_group(left, b, fused_max, long_shots)
        assert 1 <= n <= left, (k, left, n)
        out.append(n)
        left -= n
    return out


def test_group_schedule():
    """CPU only.  The groups of a call sum to its batches; calls of fewer than 32 batches, small batches and fused_max <= 8
    get the groups of before; a long call of large batches: 16 while at least 32 batches are left, then even groups of <= 8."""
    lib = _lib.load()
    for k in range(1, 301):
        for b in (1_000_000, 2500, 100_000):
            g = _groups(lib, k, b)
            assert sum(g) == k, (k, b, g)
            if k < 32 or 16 * b < (1 << 23):
                assert g == _parent_groups(k), (k, b, g)
        assert _groups(lib, k, 1_000_000, fused_max=8) == _parent_groups(k)
        assert _groups(lib, k, 1_000_000, fused_max=3) == _parent_groups(k, 3)
        assert _groups(lib, k, 2500, long_shots=1) == _groups(lib, k, 1_000_000)
        g = _groups(lib, k, 1_000_000)
        if k >= 32:
            n16 = (k - 16) // 16  # 16 while at least 32 are left
            tail = k - 16 * n16
            assert 16 <= tail <= 31
            assert g == [16] * n16 + _parent_groups(tail), (k, g)
    assert _groups(lib, 20, 1_000_000) == [7, 7, 6]
    assert _groups(lib, 200, 1_000_000) == [16] * 11 + [8, 8, 8]
    assert _groups(lib, 200, 100_000) == [8] * 25  # C4 at 10^5 shots per batch: 16 x 10^5 < 2^23
    assert lib.tsim_steps_next_group(0, 1000, 16, 1) == 0


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------

_F = {}
_RIGS = {}
_ORACLE = {}


def _f_batches(p_bit):
    if p_bit not in _F:
        _, cfg = synth.config_program("C2")
        _F[p_bit] = [synth.synth_f(B, cfg["num_f"], p_bit, seed=4100 + i) for i in range(NF_BUFS)]
    return _F[p_bit]


def _handle(hip, env):
    """A C2 handle created under `env`.  Every handle keeps the tables it is built with - weight 5, 31 MB: a budget of 64 MB has
    no room for the next depth, so the planner never builds it, however many rows are hard (shallow=0: that depth from the start).
    (TSIM_AMD_ADAPTIVE=0 would pin the tables too, but a handle without launch-plan feedback never defers its hard rows, and
    tsim_sample_steps_device then launches batch by batch - k_sample_lw_fast as groups of one: no fused group to test.)"""
    env = dict(env, TSIM_AMD_DEEP_TABLES="-1", TSIM_AMD_PATTERN_TABLE_MB="64")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        prog, cfg = synth.config_program("C2")
        hp = hip.HipProgram(prog)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return hp, prog, cfg


class _Rig:
    """One handle with its rotating buffers; run() plays a call pattern and returns the rows of the last min(K, 32) steps."""

    def __init__(self, hip, env, p_bit):
        self.hp, self.prog, cfg = _handle(hip, env)
        self.nf = cfg["num_f"]
        self.rb = (self.prog.num_outputs + 7) // 8
        wf = (self.nf + 63) // 64
        self.d_f = [self.hp.malloc(B * wf * 8) for _ in range(NF_BUFS)]
        self.d_o = [self.hp.malloc(B * 8) for _ in range(NOUT_BUFS)]
        for d, f in zip(self.d_f, _f_batches(p_bit)):
            p = np.packbits(f, axis=1, bitorder="little")
            self.hp.h2d(d, np.ascontiguousarray(np.pad(p, ((0, 0), (0, wf * 8 - p.shape[1])))))
        self.run([4, 4, 8], 0)  # launch-plan feedback
        self.hp.path_counts(reset=True)

    def run(self, calls, shot_offset):
        ks = (C.c_uint32 * 2)(KEY[0] & 0xFFFFFFFF, KEY[1] & 0xFFFFFFFF)
        j = 0
        for n in calls:
            self.hp.sample_steps_device([self.d_f[(j + i) % NF_BUFS].ptr for i in range(n)], B, self.nf, ks,
                                        [self.d_o[(j + i) % NOUT_BUFS].ptr for i in range(n)], shot_offset=shot_offset,
                                        out_bit_packed=True)
            j += n
        self.hp.synchronize()
        rows = {}
        for s in range(max(0, j - NOUT_BUFS), j):
            got = np.zeros((B, self.rb), np.uint8)
            self.hp.d2h(got, self.d_o[s % NOUT_BUFS])
            rows[s] = got
        return rows, (int(ks[0]), int(ks[1]))


def _rig(hip, which, p_bit):
    if (which, p_bit) not in _RIGS:
        env = {"long": {"TSIM_AMD_TUNE": TUNE_LONG}, "eight": {"TSIM_AMD_TUNE": TUNE_8},
               "serial": {"TSIM_AMD_TUNE": "shallow=0", "TSIM_AMD_FUSED_STEPS": "0"}}[which]
        _RIGS[(which, p_bit)] = _Rig(hip, env, p_bit)
    return _RIGS[(which, p_bit)]


def _oracle_rows(prog, p_bit, shot_offset, step):
    """Step `step` of the key chain on its f batch (the same for every call pattern: one split per batch)."""
    from oracle import oracle_c as OC

    k = (p_bit, shot_offset, step)
    if k not in _ORACLE:
        if "op" not in _ORACLE:
            _ORACLE["op"] = OC.OracleProgram(prog)
        key = KEY
        for _ in range(step + 1):
            key, sub = prng.split(key)
        want = _ORACLE["op"].sample_program(_f_batches(p_bit)[step % NF_BUFS], sub, shot_offset=shot_offset)
        _ORACLE[k] = np.packbits(want, axis=1, bitorder="little")
    return _ORACLE[k]


@pytest.mark.gpu
@pytest.mark.parametrize("p_bit", [0.02, 0.08])
@pytest.mark.parametrize("shot_offset", OFFSETS)
@pytest.mark.parametrize("calls", PATTERNS, ids=lambda c: "+".join(map(str, c)))
def test_call_patterns_equal_groups_of_eight_the_serial_path_and_the_oracle(hip, calls, shot_offset, p_bit):
    total = sum(calls)
    long_rig = _rig(hip, "long", p_bit)
    long_rig.hp.path_counts(reset=True)
    got, key_after = long_rig.run(calls, shot_offset)
    paths = long_rig.hp.path_counts()
    print(f"calls {calls} offset {shot_offset} p_bit {p_bit}: paths {paths}")
    end = KEY
    for _ in range(total):
        end, _sub = prng.split(end)
    assert key_after == (end[0] & 0xFFFFFFFF, end[1] & 0xFFFFFFFF)
    assert sorted(got) == list(range(max(0, total - NOUT_BUFS), total))
    for which in ("eight", "serial"):
        want, key_ref = _rig(hip, which, p_bit).run(calls, shot_offset)
        assert key_ref == key_after
        for s in got:
            np.testing.assert_array_equal(got[s], want[s], err_msg=f"step {s} against the '{which}' handle")
    for s in (min(got), max(got)):
        np.testing.assert_array_equal(got[s], _oracle_rows(long_rig.prog, p_bit, shot_offset, s), err_msg=f"step {s} against the oracle")
    # the launches are the schedule's: one fused first pass per group and ONE hard-row grid behind it, the groups of 16 included
    # (block per row, or 64 rows per block where the group's lists are long: 16 x 75 rows at p_bit = 0.08)
    lib = _lib.load()
    groups = sum(len(_groups(lib, n, B, 16, 1)) for n in calls)
    assert paths.get("lw_fast", 0) == groups and "lw_fast1" not in paths, (paths, groups)
    assert paths.get("hw", 0) + paths.get("sample4h_multi", 0) == groups, (paths, groups)
    assert long_rig.hp.info()["pattern_max_weight"] == [5]


@pytest.mark.gpu
def test_device_noise_over_forty_steps_equals_groups_of_eight(hip):
    """tsim_sample_steps_noise_device, 40 batches in one call: a group of 16 and three of 8 against five groups of 8 - the f rows
    the noise wrote and the outputs."""
    from tsim_amd.channels import ChannelSampler, error_probs

    n = 40
    res = []
    for tune in (TUNE_LONG, TUNE_8):
        hp, prog, cfg = _handle(hip, {"TSIM_AMD_TUNE": tune})
        nf = cfg["num_f"]
        dn = hip.DeviceNoiseSampler(hp, ChannelSampler([error_probs(0.05)] * nf, np.eye(nf, dtype=np.uint8), seed=5))
        wf, rb = (nf + 63) // 64, (prog.num_outputs + 7) // 8
        d_f = [hp.malloc(B * wf * 8) for _ in range(n)]
        d_o = [hp.malloc(B * 8) for _ in range(n)]
        for rep in range(2):  # launch-plan feedback, then the run that counts
            ks = (C.c_uint32 * 2)(KEY[0] & 0xFFFFFFFF, KEY[1] & 0xFFFFFFFF)
            nks = (C.c_uint32 * 2)(77, 78)
            hp.path_counts(reset=True)
            hp.sample_steps_noise_device(dn, [d.ptr for d in d_f], B, nf, ks, nks, [d.ptr for d in d_o], out_bit_packed=True)
            hp.synchronize()
        paths = hp.path_counts()
        fs, outs = [], []
        for j in range(n):
            f = np.zeros((B, wf * 8), np.uint8)
            hp.d2h(f, d_f[j])
            o = np.zeros((B, rb), np.uint8)
            hp.d2h(o, d_o[j])
            fs.append(f)
            outs.append(o)
        res.append((fs, outs, (int(ks[0]), int(ks[1])), (int(nks[0]), int(nks[1])), paths))
        hp.close()
    a, b = res
    print("device noise, paths:", a[4], b[4])
    assert a[2] == b[2] and a[3] == b[3]
    assert a[4].get("noise_fast", 0) == 4 and b[4].get("noise_fast", 0) == 5, (a[4], b[4])
    for j in range(n):
        np.testing.assert_array_equal(a[0][j], b[0][j], err_msg=f"f rows of batch {j}")
        np.testing.assert_array_equal(a[1][j], b[1][j], err_msg=f"outputs of batch {j}")
