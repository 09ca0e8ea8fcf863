"""The exact noise law of tests/noise_law.py, checked on the CPU before it judges the device sampler (test_gpu_noise_law.py):
against brute-force enumeration of the whole f distribution on tiny models, and against the host ``ChannelSampler`` - the
reference's stream bit for bit, pinned to golden vectors - on 10^6 shots."""

import itertools

import numpy as np
import pytest

import noise_law as NL
from tsim_amd.channels import ChannelSampler, correlated_error_probs, error_probs, pauli_channel_1_probs


def tiny_models():
    rng = np.random.default_rng(3)
    out = []
    # 3 channels over 4 f bits: a Pauli channel, a one-bit channel, a correlated pair, through a dense transform
    probs = [pauli_channel_1_probs(0.1, 0.05, 0.2), error_probs(0.3), correlated_error_probs([0.25, 0.4])]
    out.append((probs, (rng.random((4, 5)) < 0.5).astype(np.uint8)))
    # 4 channels over 8 f bits, some error bits on no f bit, one channel that always fires
    probs = [error_probs(0.1), pauli_channel_1_probs(0.02, 0.3, 0.07), error_probs(1.0), correlated_error_probs([0.1, 0.2, 0.3])]
    T = (rng.random((8, 7)) < 0.4).astype(np.uint8)
    T[:, 0] = 0
    out.append((probs, T))
    # two channels on the same column (they fold into one) and a bit nobody drives
    probs = [error_probs(0.2), error_probs(0.45), pauli_channel_1_probs(0.1, 0.1, 0.1)]
    T = np.array([[1, 1, 0, 1], [0, 0, 1, 0], [0, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 1]], np.uint8)
    out.append((probs, T))
    return out


@pytest.mark.parametrize("which", range(3))
def test_parity_formula_equals_brute_force_enumeration(which):
    probs, T = tiny_models()[which]
    nf = T.shape[0]
    law = NL.enumerate_law(probs, T)
    assert abs(sum(law.values()) - 1.0) < 1e-12
    masks = [tuple(i for i in range(nf) if (a >> i) & 1) for a in range(1, 1 << nf)]
    got = NL.parity_bias(probs, T, masks)
    for a, g in zip(range(1, 1 << nf), got):
        want = sum(p * (-1) ** bin(f & a).count("1") for f, p in law.items())
        assert abs(g - want) < 1e-12, (a, g, want)
    # the marginals, directly
    for i in range(nf):
        mu = sum(p for f, p in law.items() if (f >> i) & 1)
        assert abs((1 - NL.parity_bias(probs, T, [(i,)])[0]) / 2 - mu) < 1e-12


def test_deterministic_row_is_the_only_row_of_its_law():
    probs = [error_probs(1.0), correlated_error_probs([0.0, 1.0]), np.array([0.0, 0.0, 0.0, 1.0])]
    T = np.array([[1, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 0, 0, 1], [0, 0, 0, 1, 1]], np.uint8)
    row = NL.deterministic_row(probs, T)
    law = NL.enumerate_law(probs, T)
    assert law == {int(sum(int(b) << i for i, b in enumerate(row))): 1.0}
    with pytest.raises(ValueError):
        NL.deterministic_row([error_probs(0.5)], np.eye(1, dtype=np.uint8))


def host_model():
    """Pauli and correlated channels, a dense channel, one-bit channels down to p = 1e-3, patterns across the word boundary."""
    rng = np.random.default_rng(7)
    probs = [error_probs(p) for p in (0.5, 0.2, 0.05, 0.01, 0.001)]
    probs += [pauli_channel_1_probs(0.02, 0.03, 0.05), pauli_channel_1_probs(0.1, 0.0, 0.2),
              correlated_error_probs([0.1, 0.05, 0.02]), error_probs(0.9)]
    nbits = sum(int(np.log2(len(p))) for p in probs)
    T = (rng.random((80, nbits)) < 0.08).astype(np.uint8)
    T[63, 0] = T[64, 0] = 1  # one fire flips bits 63 and 64
    T[79, 5] = 1
    return probs, T


def groups_of(probs, T):
    """The f bits each channel can flip."""
    cols = NL._channel_columns(probs)
    return [sorted(set(np.nonzero(T[:, c].any(axis=1))[0].tolist())) for c in cols]


def test_exact_law_judges_the_host_sampler():
    """The host sampler is the reference's stream: its 10^6 rows pass the exact-law check over every singleton, the pairs
    inside each channel's pattern, pairs across channels and triples across the word boundary."""
    probs, T = host_model()
    n = 1_000_000
    rows = ChannelSampler(probs, T, seed=11).sample_packed(n)
    masks = NL.standard_masks(T.shape[0], groups_of(probs, T), np.random.default_rng(1))
    assert len(masks) >= 150
    want = NL.parity_bias(probs, T, masks)
    got = NL.empirical_bias(rows, masks)
    NL.check_biases(got, want, n, masks)
    # position classes of a bit of its own (channel 0: p = 0.5 on a bit no other channel touches)
    probs2 = [error_probs(0.5)] * 16
    rows2 = ChannelSampler(probs2, np.eye(16, dtype=np.uint8), seed=4).sample_packed(3 * 4096 + 17)
    NL.check_position_classes(rows2, list(range(16)), 0.5, 4096)


def test_empirical_bias_matches_unpacked_counts():
    rng = np.random.default_rng(5)
    bits = (rng.random((5000, 130)) < 0.3).astype(np.uint8)
    packed = np.packbits(np.pad(bits, ((0, 0), (0, 192 - 130))), axis=1, bitorder="little").view(np.uint64)
    masks = [(0,), (63,), (64,), (129,), (3, 70), (63, 64, 128), (1, 2, 3, 4), (5, 5)]
    got = NL.empirical_bias(packed, masks)
    for m, g in zip(masks, got):
        par = np.zeros(5000, np.uint8)
        for i in m:
            par ^= bits[:, i]
        assert g == 1.0 - 2.0 * par.mean(), m


def test_the_checks_have_teeth():
    """What the GPU tests rely on: a 1 % relative shift of one marginal of 0.1 over 2^22 rows, a pair correlation that the
    model does not have, a tile whose first row never fires and a partial tile left unwritten all fail."""
    n = 1 << 22
    mu = np.array([0.1, 0.1, 0.1])
    want = 1 - 2 * mu
    NL.check_biases(want.copy(), want, n)
    shifted = want.copy()
    shifted[1] = 1 - 2 * 0.101
    with pytest.raises(AssertionError):
        NL.check_biases(shifted, want, n)
    with pytest.raises(AssertionError):  # a parity the model fixes must come out exactly
        NL.check_biases(np.array([1.0 - 2.0 / n]), np.array([1.0]), n)
    with pytest.raises(AssertionError):  # two bits of independent channels (p = 0.1 each) that fire together 1 % too often
        NL.check_biases(np.array([0.64 * 1.01]), np.array([0.64]), n)
    # position classes: rows of p = 0.5 bits with the first row of every tile forced quiet
    rng = np.random.default_rng(8)
    B, M = 3 * 4096 + 17, 4096
    rows = rng.integers(0, 1 << 63, size=(B, 1), dtype=np.uint64) & np.uint64(0xFFFF)
    NL.check_position_classes(rows, list(range(16)), 0.5, M)
    bad = rows.copy()
    bad[::M] = 0
    with pytest.raises(AssertionError):
        NL.check_position_classes(bad, list(range(16)), 0.5, M)
    bad = rows.copy()
    bad[B - B % M:] = 0  # the last partial tile never written
    with pytest.raises(AssertionError):
        NL.check_position_classes(bad, list(range(16)), 0.5, M)


@pytest.mark.parametrize("num_f,n_groups", [(70, 5), (4097, 40)])
def test_standard_masks_cover_the_word_boundaries(num_f, n_groups):
    rng = np.random.default_rng(2)
    groups = [sorted(rng.choice(num_f, size=3, replace=False).tolist()) for _ in range(n_groups)]
    masks = NL.standard_masks(num_f, groups, rng)
    assert len(set(masks)) == len(masks)
    assert all(0 <= i < num_f for m in masks for i in m)
    assert sum(len(m) == 1 for m in masks) == num_f
    triples = [m for m in masks if len(m) == 3]
    assert triples and any(len({i >> 6 for i in m}) > 1 for m in triples)
    for g in groups:
        for a, b in itertools.combinations(g, 2):
            assert (a, b) in masks
