"""The device noise sampler against the exact law of its f rows (tests/noise_law.py), for each of its three kernels.

``tsim_noise_sample_device`` has no bit-exact reference by design (numpy's PCG64 stream is sequential); what it must reproduce
is the distribution.  Every case here reads packed rows back from ``DeviceNoiseSampler.sample_into``, asserts which kernel
ran (``DeviceNoiseSampler.info``), and compares exact parities - marginals, pairs inside and across channels, triples across
words - at a Bonferroni bound, fixed rows bit for bit, position classes at the tile and segment seams, and independence
between shots and between batches.  Then the batch-by-batch pipeline that reuses a ring of f buffers, against the oracle."""

import ctypes as C
import os
import time

import numpy as np
import pytest

import noise_law as NL
from oracle import oracle_c as OC
from tsim_amd import prng, synth
from tsim_amd.channels import ChannelSampler, correlated_error_probs, error_probs, pauli_channel_1_probs

pytestmark = pytest.mark.gpu

LADDER = (1e-4, 1e-3, 0.01, 0.05, 0.1, 0.2, 0.5)
_T0 = time.time()


@pytest.fixture(scope="module")
def hp(hip):
    h = hip.HipProgram(synth.config_program("C2")[0])
    yield h
    h.close()
    print(f"\ntest_gpu_noise_law.py: {time.time() - _T0:.1f} s")


def sampler(hip, hp, probs, T, tune=None):
    old = os.environ.get("TSIM_AMD_TUNE")
    if tune is not None:
        os.environ["TSIM_AMD_TUNE"] = tune
    try:
        return hip.DeviceNoiseSampler(hp, ChannelSampler(probs, T, seed=1))
    finally:
        if tune is not None:
            if old is None:
                os.environ.pop("TSIM_AMD_TUNE", None)
            else:
                os.environ["TSIM_AMD_TUNE"] = old


def draw(hp, dn, B, key, fill=0xA5):
    """``uint64[B, WF]`` rows of one ``sample_into`` call, on a buffer filled with ``fill`` first (a row the kernel fails to
    write shows up)."""
    wf = max(1, (dn.num_f + 63) // 64)
    buf = hp.malloc(max(16, B * wf * 8))
    hp.h2d(buf, np.full(max(16, B * wf * 8), fill, np.uint8))
    dn.sample_into(buf.ptr, B, key)
    out = np.zeros((B, wf), np.uint64)
    hp.d2h(out, buf)
    buf.free()
    return out


def seam(info):
    """The shots per block (or per thread, for k_noise) of the kernel that ran."""
    return {"k_noise_wave": info["wave_tile"], "k_noise_tile": info["tile"], "k_noise": info["seg"]}[info["form"]]


def assert_padding_zero(rows, num_f):
    if num_f % 64:
        assert not (rows[:, -1] >> np.uint64(num_f % 64)).any(), "bits beyond num_f are set"


# ---- models -----------------------------------------------------------------------------------------------------------


def rich_model(num_f, rng, n_one_bit=None, dense=None):
    """One-bit channels over the p ladder on bits of their own, Pauli channels (three outcomes, distinct patterns), a
    correlated three-branch channel, a channel whose one fire flips bits 63, 64 and num_f - 1 (several pattern words), and
    optionally one dense channel (``dense``: its p)."""
    probs, cols = [], []

    def unit(*bits):
        c = np.zeros(num_f, np.uint8)
        c[list(bits)] = 1
        return c

    free = [i for i in range(num_f) if i not in (63, 64, num_f - 1)]
    n1 = min(len(free) - 8, n_one_bit if n_one_bit is not None else 40)
    for i in range(n1):
        probs.append(error_probs(LADDER[i % len(LADDER)]))
        cols.append(unit(free[i]))
    rest = free[n1:]
    probs.append(pauli_channel_1_probs(0.02, 0.03, 0.05))  # Z -> bit a, X -> bit b, Y both
    cols += [unit(rest[0]), unit(rest[1])]
    probs.append(pauli_channel_1_probs(0.15, 0.05, 0.25))
    cols += [unit(rest[2], rest[0]), unit(rest[3])]
    probs.append(correlated_error_probs([0.1, 0.05, 0.02]))
    cols += [unit(rest[4]), unit(rest[5], rest[3]), unit(rest[6])]
    if num_f > 65:
        probs.append(error_probs(0.3))
        cols.append(unit(63, 64, num_f - 1))
    if dense is not None:
        probs.append(error_probs(dense))
        cols.append(unit(rest[7]))
    T = np.stack(cols, axis=1)
    return probs, T


def one_bit_model(num_f, n_ch, p=None):
    """``n_ch`` one-bit channels on bits of their own (channel c on bit c * num_f // n_ch), p over the ladder or fixed."""
    bits = [c * num_f // n_ch for c in range(n_ch)]
    T = np.zeros((num_f, n_ch), np.uint8)
    T[bits, range(n_ch)] = 1
    probs = [error_probs(p if p is not None else LADDER[c % len(LADDER)]) for c in range(n_ch)]
    return probs, T, bits


def groups_of(probs, T):
    cols = NL._channel_columns(probs)
    return [sorted(set(np.nonzero(T[:, c].any(axis=1))[0].tolist())) for c in cols]


def check_law(rows, probs, T, rng, singles=None, n_groups=60):
    num_f = T.shape[0]
    groups = [g for g in groups_of(probs, T) if len(g) > 1][:n_groups]
    masks = NL.standard_masks(num_f, groups, rng, singles=singles)
    want = NL.parity_bias(probs, T, masks)
    got = NL.empirical_bias(rows, masks)
    NL.check_biases(got, want, rows.shape[0], masks)
    return len(masks)


# ---- 1. the law, per kernel form ----------------------------------------------------------------------------------------

LAW_CASES = [
    # name, num_f, model, tune, form, shots
    ("wave-64-dense", 64, dict(dense=0.9, n_one_bit=40), None, "k_noise_wave", 1 << 22),
    ("wave-70", 70, dict(dense=0.6), None, "k_noise_wave", 1 << 22),
    ("tile-70", 70, dict(dense=0.6), "noise_wave=0", "k_noise_tile", 1 << 22),
    ("wave-6144", 6144, dict(n_one_bit=900), None, "k_noise_wave", 1 << 17),
    ("tile-1100", 1100, dict(n_one_bit=1080), None, "k_noise_tile", 1 << 18),
    ("knoise-6145", 6145, dict(n_one_bit=600), None, "k_noise", 1 << 17),
    ("knoise-4097", 4097, dict(n_one_bit=1100), None, "k_noise", 1 << 17),
]


@pytest.mark.parametrize("name,num_f,kw,tune,form,shots", LAW_CASES, ids=[c[0] for c in LAW_CASES])
def test_rows_follow_the_exact_law(hip, hp, name, num_f, kw, tune, form, shots):
    rng = np.random.default_rng(num_f)
    probs, T = rich_model(num_f, rng, **kw)
    dn = sampler(hip, hp, probs, T, tune)
    info = dn.info()
    assert info["form"] == form, info
    if name == "wave-64-dense":  # a 64-lane group needs many rounds to cover a 4096-shot tile at p = 0.9
        assert info["wave_tile"] == 4096 and info["wave_g"] == 64, info
    n_ch = len(ChannelSampler(probs, T, seed=1)._sparse_data)
    if form == "k_noise_tile" and tune is None:
        assert n_ch > 1024
    if form == "k_noise":
        assert num_f > 6144 or n_ch > 1024
    rows = draw(hp, dn, shots, (num_f, 7))
    assert_padding_zero(rows, num_f)
    n_masks = check_law(rows, probs, T, rng)
    assert n_masks >= 100


@pytest.mark.parametrize("num_f,n_ch,form", [
    (1, 1, "k_noise_wave"), (63, 63, "k_noise_wave"), (65, 65, "k_noise_wave"), (4096, 1024, "k_noise_wave"),
    (4096, 1025, "k_noise_tile"), (4096, 3000, "k_noise_tile"), (6145, 1, "k_noise"), (6145, 3000, "k_noise"),
])
def test_boundaries_of_row_width_and_channel_count(hip, hp, num_f, n_ch, form):
    """num_f and channel counts at the seams of the kernel choice (WF = 1 / 2, 64 / 65 words, 96 / 97 words; 1024 / 1025
    channels), one-bit channels over the p ladder; B = 3 seams + 17."""
    probs, T, bits = one_bit_model(num_f, n_ch)
    dn = sampler(hip, hp, probs, T)
    info = dn.info()
    assert info["form"] == form, info
    B = max(3 * seam(info) + 17, min(1 << 20, (1 << 26) // max(1, (num_f + 63) // 64 * 8)))
    rows = draw(hp, dn, B, (n_ch, num_f))
    assert_padding_zero(rows, num_f)
    rng = np.random.default_rng(n_ch)
    # the driven bits all, a sample of the undriven ones (exactly zero: bias 1)
    quiet = sorted(set(range(num_f)) - set(bits))
    singles = sorted(set(bits) | set(rng.choice(quiet, size=min(len(quiet), 200), replace=False).tolist() if quiet else []))
    check_law(rows, probs, T, rng, singles=singles)


# ---- 2. fixed rows, exactly, over every B seam --------------------------------------------------------------------------

def fixed_model(num_f, with_noise):
    """Channels that always fire with one outcome: a one-bit channel, a correlated channel whose second branch is certain, a
    two-bit channel that always reads 11 - their row is the XOR of the patterns on every shot.  ``with_noise``: plus low-p
    channels on bits of their own (disjoint from the fixed ones)."""
    cols, probs = [], []

    def unit(*b):
        c = np.zeros(num_f, np.uint8)
        c[[x % num_f for x in b]] = 1
        return c

    probs.append(error_probs(1.0))
    cols.append(unit(0, num_f - 1))
    if num_f >= 4:
        probs.append(correlated_error_probs([0.0, 1.0]))
        cols += [unit(1), unit(2, 63, 64)]
        probs.append(np.array([0.0, 0.0, 0.0, 1.0]))
        cols += [unit(3, 64), unit(63, num_f // 2)]
    fixed = sorted(set(np.nonzero(np.stack(cols, 1).any(axis=1))[0].tolist()))
    free = [i for i in range(num_f) if i not in fixed]
    if with_noise:
        for j, i in enumerate(free[:200]):
            probs.append(error_probs((0.001, 0.01, 0.05)[j % 3]))
            cols.append(unit(i))
    return probs, np.stack(cols, axis=1), fixed


@pytest.mark.parametrize("num_f,tune,form", [
    (64, None, "k_noise_wave"), (70, None, "k_noise_wave"), (70, "noise_wave=0", "k_noise_tile"), (4096, None, "k_noise_wave"),
    (1100, "noise_wave=0", "k_noise_tile"), (6145, None, "k_noise"),
])
@pytest.mark.parametrize("with_noise", [False, True])
def test_fixed_rows_are_exact_on_every_row(hip, hp, num_f, tune, form, with_noise):
    probs, T, fixed = fixed_model(num_f, with_noise)
    want_row = NL.deterministic_row(probs[:3] if num_f >= 4 else probs[:1], T[:, : sum(int(np.log2(len(p))) for p in probs[:3 if num_f >= 4 else 1])])
    dn = sampler(hip, hp, probs, T, tune)
    info = dn.info()
    assert info["form"] == form, info
    t = seam(info)
    want = np.packbits(np.pad(want_row, (0, 64 * info["words"] - num_f)), bitorder="little").view(np.uint64)
    fmask = np.zeros(64 * info["words"], np.uint8)
    fmask[fixed] = 1
    fmask = np.packbits(fmask, bitorder="little").view(np.uint64)
    for B in (1, t - 1, t, t + 1, 3 * t + 17):
        rows = draw(hp, dn, B, (B, 5))
        assert_padding_zero(rows, num_f)
        got = rows & fmask
        bad = np.nonzero((got != (want & fmask)).any(axis=1))[0]
        assert len(bad) == 0, f"B = {B}: {len(bad)} rows differ from the fixed row, first {bad[:8]}"
        if not with_noise:
            assert np.array_equal(rows, np.broadcast_to(want, rows.shape)), f"B = {B}"


# ---- 3. position classes and independence --------------------------------------------------------------------------------

POS_CASES = [("k_noise_wave", 64, None), ("k_noise_tile", 64, "noise_wave=0"), ("k_noise", 6145, None)]


@pytest.mark.parametrize("form,num_f,tune", POS_CASES, ids=[c[0] for c in POS_CASES])
def test_position_classes_and_independence(hip, hp, form, num_f, tune):
    """64 channels at p = 0.5 on bits of their own: the fire rate in every class shot mod (tile or segment), in the first
    tile and in the last partial tile; shot-to-shot parities at distances 1, 63, 64 and the seam; consecutive batches."""
    bits = list(range(32)) + list(range(num_f - 32, num_f))
    T = np.zeros((num_f, 64), np.uint8)
    T[bits, range(64)] = 1
    probs = [error_probs(0.5)] * 64
    dn = sampler(hip, hp, probs, T, tune)
    info = dn.info()
    assert info["form"] == form, info
    M = seam(info)
    B = (256 if num_f <= 64 else 2048) * M + 17  # (1 M narrow rows; 131 k rows of 97 words)
    kn = prng.key(3)
    kn, sub = prng.split(kn)
    rows = draw(hp, dn, B, sub)
    NL.check_position_classes(rows, bits, 0.5, M)
    if form == "k_noise_tile" and info["tseg"] < M:
        NL.check_position_classes(rows, bits, 0.5, info["tseg"])
    # shot to shot: f_i(s) xor f_i(s + d) is a fair coin for every bit and distance (pairs of a p = 0.5 bit are uncorrelated)
    words = sorted({b >> 6 for b in bits})
    wmask = {w: np.uint64(sum(1 << (b & 63) for b in bits if b >> 6 == w)) for w in words}
    checks = []
    for d in (1, 63, 64, M):
        x = sum(int(np.bitwise_count((rows[:-d, w] ^ rows[d:, w]) & m).sum()) for w, m in wmask.items())
        checks.append((f"distance {d}", x, (B - d) * len(bits)))
    # batch to batch: the next split key gives rows independent of these
    kn, sub2 = prng.split(kn)
    rows2 = draw(hp, dn, B, sub2)
    x = sum(int(np.bitwise_count((rows[:, w] ^ rows2[:, w]) & m).sum()) for w, m in wmask.items())
    checks.append(("consecutive batches", x, B * len(bits)))
    z = NL.z_bound(len(checks))
    for what, x, n in checks:
        assert abs(x - n / 2) <= z * np.sqrt(n / 4), f"{what}: {x} of {n} differ, |z| = {abs(x - n / 2) / np.sqrt(n / 4):.1f}"


# ---- 4. the fused noise + first pass kernel ------------------------------------------------------------------------------

def test_fused_noise_rows_follow_the_exact_law(hip):
    """C2 through ``sample_steps_noise_device``: the rows come from the fused noise + first pass kernel (path_counts says
    so); read back from d_f, they follow the law of a rich 64-bit model."""
    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    rng = np.random.default_rng(5)
    # light noise, so that the launch plan stays on the fused tables: one-bit channels up to 0.02, a Pauli and a correlated
    # channel, a pair of bits flipped together
    probs = [error_probs(p) for p in (1e-4, 1e-3, 0.005, 0.01, 0.02) * 10]
    probs += [pauli_channel_1_probs(0.004, 0.003, 0.005), correlated_error_probs([0.01, 0.005, 0.002]), error_probs(0.01)]
    T = np.zeros((nf, 50 + 2 + 3 + 1), np.uint8)
    T[range(50), range(50)] = 1
    T[50, 50] = T[51, 51] = T[50, 51] = 1  # Z -> bit 50, X -> bits 50 and 51
    T[52, 52] = T[53, 53] = T[54, 54] = T[52, 54] = 1
    T[62, 55] = T[63, 55] = 1
    h = hip.HipProgram(prog)
    dn = hip.DeviceNoiseSampler(h, ChannelSampler(probs, T, seed=1))
    info = dn.info()
    assert info["form"] == "k_noise_wave" and info["fusable"], info
    B, n = 1 << 19, 8
    d_f = [h.malloc(B * 8) for _ in range(n)]
    d_o = [h.malloc(B * 8) for _ in range(n)]
    ks, nks = (C.c_uint32 * 2)(1, 2), (C.c_uint32 * 2)(3, 4)
    for _ in range(2):  # the first call feeds the launch plan
        h.path_counts(reset=True)
        h.sample_steps_noise_device(dn, [d.ptr for d in d_f], B, nf, ks, nks, [d.ptr for d in d_o], out_bit_packed=True)
        h.synchronize()
    assert h.path_counts().get("noise_fast", 0) >= 1, h.path_counts()
    rows = np.zeros((n * B, 1), np.uint64)
    for j in range(n):
        h.d2h(rows[j * B:(j + 1) * B], d_f[j])
    h.close()
    assert check_law(rows, probs, T, rng) >= 100


# ---- 5. the ring of f buffers, batch by batch, against the oracle ---------------------------------------------------------

FUSED_FAMILIES = ("lw_fast", "lw_multi", "lw_fastm", "gen", "noise_fast")


@pytest.mark.parametrize("cn,B", [("C2", 3000), ("C4", 2000)])
def test_slot_ring_batch_by_batch_equals_the_oracle(hip, monkeypatch, cn, B):
    """``TSIM_AMD_FUSED_STEPS=0`` and dense noise: every batch of ``sample_steps_noise_device`` goes through the batch-by-batch
    branch, with hard rows deferred.  The f buffers are a ring of ``PIPELINE_SLOTS`` as in the sampler - batch j of a call on
    ``ring[(pipeline_next_slot() + j) % 32]`` - over calls of 1-4 batches and one of 40, so the ring wraps twice and a slot is
    reused inside one call.  Each batch's rows are drawn again on a buffer of their own from its noise subkey, and its
    outputs must equal the oracle's on them.  The noise kernel that overwrites a slot's rows must wait for that slot's last
    launch, hard rows included; a race may not show on every run, so a pass is evidence, not proof."""
    monkeypatch.setenv("TSIM_AMD_FUSED_STEPS", "0")
    prog, cfg = synth.config_program(cn)
    nf = cfg["num_f"]
    probs, T = [error_probs(0.25)] * nf, np.eye(nf, dtype=np.uint8)
    h = hip.HipProgram(prog)
    monkeypatch.delenv("TSIM_AMD_FUSED_STEPS")
    dn = hip.DeviceNoiseSampler(h, ChannelSampler(probs, T, seed=1))
    nslot = h.PIPELINE_SLOTS
    WF, RB = max(1, (nf + 63) // 64), (prog.num_outputs + 7) // 8
    ring = [h.malloc(B * WF * 8) for _ in range(nslot)]
    calls = [1, 2, 3, 4] * 3 + [1, 4, 2, 3, 40, 2, 1, 3]
    total = sum(calls)
    assert total >= 70 and max(calls) > nslot
    d_o = [h.malloc(B * RB + 16) for _ in range(total)]
    key, nkey = prng.key(41), prng.key(42)
    ks = (C.c_uint32 * 2)(key[0] & 0xFFFFFFFF, key[1] & 0xFFFFFFFF)
    nks = (C.c_uint32 * 2)(nkey[0] & 0xFFFFFFFF, nkey[1] & 0xFFFFFFFF)
    h.path_counts(reset=True)
    b = 0
    for n in calls:
        first = h.pipeline_next_slot()
        h.sample_steps_noise_device(dn, [ring[(first + j) % nslot].ptr for j in range(n)], B, nf, ks, nks,
                                    [d.ptr for d in d_o[b:b + n]], out_bit_packed=True)
        b += n
    h.synchronize()
    paths = h.path_counts()
    assert not set(paths) & set(FUSED_FAMILIES), paths
    outs = []
    for j in range(total):
        o = np.zeros((B, RB), np.uint8)
        h.d2h(o, d_o[j])
        outs.append(o)
    # each batch's rows again, on a buffer of their own, from the split chain of the noise key
    kn, k, subs = nkey, key, []
    for j in range(total):
        kn, nsub = prng.split(kn)
        k, sub = prng.split(k)
        f = draw(h, dn, B, nsub)
        subs.append((np.unpackbits(f.view(np.uint8), axis=1, bitorder="little")[:, :nf], sub))
    assert (int(ks[0]), int(ks[1])) == (k[0] & 0xFFFFFFFF, k[1] & 0xFFFFFFFF)
    assert (int(nks[0]), int(nks[1])) == (kn[0] & 0xFFFFFFFF, kn[1] & 0xFFFFFFFF)
    h.close()
    op = OC.OracleProgram(prog)
    bad = []
    for j, (f, sub) in enumerate(subs):
        assert 0.2 < f.mean() < 0.3
        want = np.packbits(op.sample_program(f, sub), axis=1, bitorder="little")
        if not np.array_equal(outs[j], want):
            bad.append(j)
    assert not bad, f"batches {bad} differ from the oracle on their own rows"


def test_device_noise_sampler_beyond_the_ring_equals_the_oracle_twin(hip, monkeypatch):
    """``CompiledDetectorSampler(noise="device")`` over 40 batches batch by batch (``TSIM_AMD_FUSED_STEPS=0``, dense noise): its
    ring of 32 f buffers wraps.  The twin is the host route with the oracle's ``sample_program`` fed the rows the device
    sampler draws for each batch's noise subkey (the sampler's own key chain) - batches beyond the 32nd are judged by an
    independent reference, not by a second run."""
    import tsim_amd.sampler as sampler_module
    from tsim_amd.sampler import CompiledDetectorSampler

    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    kw = dict(channel_probs=[error_probs(0.25)] * nf, error_transform=np.eye(nf, dtype=np.uint8), seed=13)
    B, nb = 2000, 40
    monkeypatch.setenv("TSIM_AMD_FUSED_STEPS", "0")
    s = CompiledDetectorSampler(prog, noise="device", **kw)
    s._estimate_batch_size = lambda: B  # batches of B rows (the device route merges small batches up to this)
    got = s.sample(B * nb, batch_size=B, append_observables=True)
    hp = s._hip()
    assert not set(hp.path_counts()) & set(FUSED_FAMILIES), hp.path_counts()
    monkeypatch.delenv("TSIM_AMD_FUSED_STEPS")
    twin = CompiledDetectorSampler(synth.config_program("C2")[0], noise="host", **kw)
    dn = s._device_noise_sampler(hp)
    chain = {"k": twin._noise_key}

    def device_rows(n):
        chain["k"], sub = prng.split(chain["k"])
        f = draw(hp, dn, n, sub)
        return np.unpackbits(f.view(np.uint8), axis=1, bitorder="little")[:, :nf]

    twin._channel_sampler.sample = device_rows
    op = OC.OracleProgram(twin._program)
    monkeypatch.setattr(sampler_module, "sample_program", lambda program, f, key: op.sample_program(f, key))
    want = twin.sample(B * nb, batch_size=B, append_observables=True)
    assert got.shape == want.shape == (B * nb, prog.num_outputs)
    bad = [j for j in range(nb) if not np.array_equal(got[j * B:(j + 1) * B], want[j * B:(j + 1) * B])]
    assert not bad, f"batches {bad} differ from the oracle twin"


# ---- 6. a failed call moves neither key ----------------------------------------------------------------------------------

def test_a_failed_call_moves_neither_key(hip):
    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    probs, T = [error_probs(0.02)] * nf, np.eye(nf, dtype=np.uint8)
    B, n = 4096, 3

    def fresh():
        h = hip.HipProgram(prog)
        return h, hip.DeviceNoiseSampler(h, ChannelSampler(probs, T, seed=1)), [h.malloc(B * 8) for _ in range(n)], [h.malloc(B * 8) for _ in range(n)]

    h, dn, d_f, d_o = fresh()
    ks, nks = (C.c_uint32 * 2)(5, 6), (C.c_uint32 * 2)(7, 8)
    with pytest.raises(ValueError):
        h.sample_steps_noise_device(dn, [d.ptr for d in d_f], B, nf, ks, nks, [d_o[0].ptr, 0, d_o[2].ptr], out_bit_packed=True)
    assert (ks[0], ks[1], nks[0], nks[1]) == (5, 6, 7, 8)
    h.sample_steps_noise_device(dn, [d.ptr for d in d_f], B, nf, ks, nks, [d.ptr for d in d_o], out_bit_packed=True)
    h.synchronize()
    assert (ks[0], ks[1]) != (5, 6) and (nks[0], nks[1]) != (7, 8)

    def read(h, bufs, width):
        out = []
        for d in bufs:
            a = np.zeros((B, width), np.uint8)
            h.d2h(a, d)
            out.append(a)
        return out

    a_f, a_o = read(h, d_f, 8), read(h, d_o, (prog.num_outputs + 7) // 8)
    after = (ks[0], ks[1], nks[0], nks[1])
    h.close()
    h2, dn2, d_f2, d_o2 = fresh()
    ks2, nks2 = (C.c_uint32 * 2)(5, 6), (C.c_uint32 * 2)(7, 8)
    h2.sample_steps_noise_device(dn2, [d.ptr for d in d_f2], B, nf, ks2, nks2, [d.ptr for d in d_o2], out_bit_packed=True)
    h2.synchronize()
    b_f, b_o = read(h2, d_f2, 8), read(h2, d_o2, (prog.num_outputs + 7) // 8)
    assert (ks2[0], ks2[1], nks2[0], nks2[1]) == after
    h2.close()
    for j in range(n):
        np.testing.assert_array_equal(a_f[j], b_f[j])
        np.testing.assert_array_equal(a_o[j], b_o[j])
