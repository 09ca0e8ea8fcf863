"""The group protocol of ``tsim_sample_steps_device``, one group launcher per case: the lane and slot
bookkeeping around the first pass - taking slots off the rotating ring of 32, ordering a slot behind its previous launch, the
key split per batch, parking the group's hard rows or marking its slots done - is the same code under ``k_sample_lw_fast``,
``k_sample_lw_multi``, ``k_sample_lw_fastm``, ``k_sample_gen`` (groups that leave hard-row lists) and under ``k_sample_wide``
and ``k_direct_multi`` (groups that leave nothing).

Every case: B = 2500 shots (three row blocks of 1024 with the last partial, 40 chunks of 64 with the last partial), the call
pattern [3, 8, 1, 9, 16] - 37 batches behind a warm-up of 16, so the 32 slots wrap, and the 9 and the 16 split into more than
one group - with shot offsets 0 and 3 << 20 (check row present and absent) and rows bit-packed and padded.  The rows of all
37 batches equal those of a handle created with ``TSIM_AMD_FUSED_STEPS=0`` (batch by batch), the first and the last batch
equal the C oracle, the key state is 37 splits on, and the family's launch count is the number of groups the schedule gives.
The tables are pinned as in tests/test_gpu_steps_groups.py (``_handle`` there says why)."""

import ctypes as C
import os
import warnings

import numpy as np
import pytest

from tsim_amd import _lib, prng, synth

pytestmark = pytest.mark.gpu

B = 2500
CALLS = [3, 8, 1, 9, 16]
TOTAL = sum(CALLS)
NF_BUFS = 4
KEY = prng.key(4321)
OFFSETS = [0, 3 << 20]
ONE_BATCH = ("lw_fast1", "lw_reg", "lw_lds")

# family -> (program, TSIM_AMD_TUNE, path name, launches per group, cap of the even groups - None: tsim_steps_next_group)
FAMILIES = {
    "lw_fast": ("C2", "fused_max=16:1,shallow=0", "lw_fast", 1, None),
    "lw_multi": ("C2", "lw_fast=0,shallow=0", "lw_multi", 1, 8),
    "lw_fastm": ("C4", "shallow=0", "lw_fastm", 1, 8),  # component-parallel hard rows
    "gen": ("C2", "gen=2,shallow=0", "gen", 1, 8),
    "wide": ("2wide", "shallow=0", "wide", 2, 8),  # one pass per component
    "direct": ("C1", "shallow=0", "direct_multi", 1, 8),
}


def _program(name):
    if name in synth.CONFIGS:
        return synth.config_program(name)
    return synth.shape_class_program(name)


def _n_groups(family):
    """Groups the schedule makes of the call pattern: tsim_steps_next_group for the register first pass with its long
    groups allowed, even groups - as few as possible - of at most the family's cap for the others."""
    cap = FAMILIES[family][4]
    lib = _lib.load()
    count = 0
    for n in CALLS:
        left = n
        while left > 0:
            if cap is None:
                g = lib.tsim_steps_next_group(left, B, 16, 1)
            else:
                groups = -(-left // cap)
                g = -(-left // groups)
            assert 1 <= g <= left
            left -= g
            count += 1
    return count


_F = {}
_RIGS = {}
_ORACLE = {}


def _f_batches(family):
    if family not in _F:
        _, cfg = _program(FAMILIES[family][0])
        _F[family] = [synth.synth_f(B, cfg["num_f"], cfg["p_bit"], seed=5200 + i) for i in range(NF_BUFS)]
    return _F[family]


class _Rig:
    """One handle with 4 rotating f buffers and one output buffer per batch (both row layouts fit it)."""

    def __init__(self, hip, family, serial):
        name, tune = FAMILIES[family][:2]
        env = {"TSIM_AMD_TUNE": tune, "TSIM_AMD_DEEP_TABLES": "-1", "TSIM_AMD_PATTERN_TABLE_MB": "64"}
        if serial:
            env["TSIM_AMD_FUSED_STEPS"] = "0"
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.prog, cfg = _program(name)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.hp = hip.HipProgram(self.prog)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.family = family
        self.nf = cfg["num_f"]
        self.p_bit = cfg["p_bit"]
        self.wf = (self.nf + 63) // 64
        self.rb = (self.prog.num_outputs + 7) // 8
        self.wo = (self.prog.num_outputs + 63) // 64
        self.d_f = [self.hp.malloc(B * self.wf * 8) for _ in range(NF_BUFS)]
        self.d_o = [self.hp.malloc(B * self.wo * 8) for _ in range(TOTAL)]
        for d, f in zip(self.d_f, _f_batches(family)):
            p = np.packbits(f, axis=1, bitorder="little")
            self.hp.h2d(d, np.ascontiguousarray(np.pad(p, ((0, 0), (0, self.wf * 8 - p.shape[1])))))
        self.run([4, 4, 8], 0, True)  # launch-plan feedback
        self.noise = None
        self.d_nf = None

    def rows(self, n, packed):
        out = []
        for s in range(n):
            got = np.zeros((B, self.rb if packed else self.wo * 8), np.uint8)
            self.hp.d2h(got, self.d_o[s])
            out.append(got)
        return out

    def run(self, calls, shot_offset, packed):
        ks = (C.c_uint32 * 2)(KEY[0] & 0xFFFFFFFF, KEY[1] & 0xFFFFFFFF)
        j = 0
        for n in calls:
            self.hp.sample_steps_device([self.d_f[(j + i) % NF_BUFS].ptr for i in range(n)], B, self.nf, ks,
                                        [self.d_o[j + i].ptr for i in range(n)], shot_offset=shot_offset, out_bit_packed=packed)
            j += n
        self.hp.synchronize()
        return self.rows(j, packed), (int(ks[0]), int(ks[1]))

    def run_noise(self, hip, calls):
        """The pattern through sample_steps_noise_device: the f rows the noise wrote, the outputs, both key states."""
        from tsim_amd.channels import ChannelSampler, error_probs

        if self.noise is None:
            self.noise = hip.DeviceNoiseSampler(self.hp, ChannelSampler([error_probs(self.p_bit)] * self.nf, np.eye(self.nf, dtype=np.uint8), seed=5))
            self.d_nf = [self.hp.malloc(B * self.wf * 8) for _ in range(TOTAL)]
        ks = (C.c_uint32 * 2)(KEY[0] & 0xFFFFFFFF, KEY[1] & 0xFFFFFFFF)
        nks = (C.c_uint32 * 2)(77, 78)
        j = 0
        for n in calls:
            self.hp.sample_steps_noise_device(self.noise, [d.ptr for d in self.d_nf[j:j + n]], B, self.nf, ks, nks,
                                              [d.ptr for d in self.d_o[j:j + n]], out_bit_packed=True)
            j += n
        self.hp.synchronize()
        fs = []
        for s in range(j):
            f = np.zeros((B, self.wf * 8), np.uint8)
            self.hp.d2h(f, self.d_nf[s])
            fs.append(f)
        return fs, self.rows(j, True), (int(ks[0]), int(ks[1])), (int(nks[0]), int(nks[1]))


def _rig(hip, family, serial=False):
    if (family, serial) not in _RIGS:
        _RIGS[(family, serial)] = _Rig(hip, family, serial)
    return _RIGS[(family, serial)]


def _oracle_rows(rig, shot_offset, step):
    """Step `step` of the key chain on its f batch, bit-packed."""
    from oracle import oracle_c as OC

    k = (rig.family, shot_offset, step)
    if k not in _ORACLE:
        if rig.family not in _ORACLE:
            _ORACLE[rig.family] = OC.OracleProgram(rig.prog)
        key = KEY
        for _ in range(step + 1):
            key, sub = prng.split(key)
        want = _ORACLE[rig.family].sample_program(_f_batches(rig.family)[step % NF_BUFS], sub, shot_offset=shot_offset)
        _ORACLE[k] = np.packbits(want, axis=1, bitorder="little")
    return _ORACLE[k]


def _key_after(n):
    end = KEY
    for _ in range(n):
        end, _sub = prng.split(end)
    return (end[0] & 0xFFFFFFFF, end[1] & 0xFFFFFFFF)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("shot_offset", OFFSETS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_group_launcher_equals_the_serial_path_and_the_oracle(hip, family, shot_offset, packed):
    rig = _rig(hip, family)
    rig.hp.path_counts(reset=True)
    got, key_after = rig.run(CALLS, shot_offset, packed)
    paths = rig.hp.path_counts()
    groups = _n_groups(family)
    print(f"{family} offset {shot_offset} packed {packed}: paths {paths}, groups {groups}")
    assert key_after == _key_after(TOTAL)
    want, key_ref = _rig(hip, family, serial=True).run(CALLS, shot_offset, packed)
    assert key_ref == key_after
    assert len(got) == len(want) == TOTAL
    for s in range(TOTAL):
        np.testing.assert_array_equal(got[s], want[s], err_msg=f"batch {s} against the batch-by-batch handle")
    for s in (0, TOTAL - 1):
        np.testing.assert_array_equal(got[s][:, :rig.rb], _oracle_rows(rig, shot_offset, s), err_msg=f"batch {s} against the oracle")
        assert not got[s][:, rig.rb:].any()
    _, _, path, per_group, _ = FAMILIES[family]
    assert paths.get(path, 0) == per_group * groups, (paths, groups)
    assert not set(ONE_BATCH) & set(paths), paths


@pytest.mark.parametrize("family", list(FAMILIES))
def test_group_launcher_with_device_noise_equals_the_serial_path(hip, family):
    rig = _rig(hip, family)
    rig.hp.path_counts(reset=True)
    fs, outs, key_after, nkey_after = rig.run_noise(hip, CALLS)
    paths = rig.hp.path_counts()
    print(f"{family} with device noise: paths {paths}")
    wfs, wouts, key_ref, nkey_ref = _rig(hip, family, serial=True).run_noise(hip, CALLS)
    assert key_after == key_ref == _key_after(TOTAL)
    assert nkey_after == nkey_ref and nkey_after != (77, 78)
    for s in range(TOTAL):
        np.testing.assert_array_equal(fs[s], wfs[s], err_msg=f"f rows of batch {s}")
        np.testing.assert_array_equal(outs[s], wouts[s], err_msg=f"outputs of batch {s}")
    assert any(f.any() for f in fs)
    # the group launcher ran (the register first pass of one component draws the noise itself: k_noise_sample_fast)
    path = "noise_fast" if family == "lw_fast" else FAMILIES[family][2]
    assert paths.get(path, 0) >= 1 and not set(ONE_BATCH) & set(paths), paths


def test_steps_call_meets_a_parked_slot(hip):
    """A launch of the per-batch API parked on the slot the next steps call takes first, left without its _end: the steps
    call runs its hard rows first (the entry flush; the pre-loop of the group would, were it still parked there)."""
    res = []
    for serial in (False, True):
        rig = _rig(hip, "lw_fast", serial)
        hp = rig.hp
        slot = hp.pipeline_next_slot()
        extra = hp.malloc(B * 8)
        hp.sample_batch_device_begin(slot, rig.d_f[1].ptr, B, rig.nf, (11, 12), extra.ptr, out_bit_packed=True)
        ks = (C.c_uint32 * 2)(KEY[0] & 0xFFFFFFFF, KEY[1] & 0xFFFFFFFF)
        hp.sample_steps_device([rig.d_f[i % NF_BUFS].ptr for i in range(8)], B, rig.nf, ks, [rig.d_o[i].ptr for i in range(8)],
                               out_bit_packed=True)
        hp.sample_batch_device_end(slot)
        hp.synchronize()
        first = np.zeros((B, rig.rb), np.uint8)
        hp.d2h(first, extra)
        res.append(([first] + rig.rows(8, True), (int(ks[0]), int(ks[1]))))
    assert res[0][1] == res[1][1] == _key_after(8)
    for s, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        np.testing.assert_array_equal(a, b, err_msg=f"batch {s} of nine (0: the parked launch)")
    assert res[0][0][0].any()
