"""The exact law of the f rows a noise model produces, for judging samplers that have no bit-exact reference.

Works from the UNsimplified model - ``probs``: one outcome vector of length ``2**k`` per channel (bit ``i`` of an outcome =
the channel's error bit ``i``), ``T``: the error transform ``uint8[num_f, total error bits]`` (``f = T e mod 2``) - and never
reads ``ChannelSampler``'s simplified tables, so it stays independent of the code under test.

Channels are independent, so for any parity mask ``a`` over the f bits

    E[(-1)^(a.f)] = prod_c  sum_o probs_c[o] * (-1)^(a . (T_c bits(o)))

in float64.  That one formula gives every marginal (``mu = (1 - E) / 2`` for a singleton), every pairwise and higher
correlation, and the independence of bits driven by different channels.  A mask is a tuple of f-bit indices; rows are
packed ``uint64[B, ceil(num_f / 64)]`` (bit ``i`` of a row = ``f_i``), the layout every sampler here writes.
"""

from __future__ import annotations

import math

import numpy as np

# family-wise false-alarm rate of one check_biases / check_position_classes call: the device stream is deterministic for fixed
# keys, so a build either passes or fails every time - this bounds the chance that a correct build draws keys that fail
FAMILY_ALPHA = 1e-6


def _channel_columns(probs) -> list:
    """Per channel: the indices of its error bits' columns in T."""
    cols, at = [], 0
    for p in probs:
        k = int(round(math.log2(len(p))))
        if 1 << k != len(p):
            raise ValueError(f"outcome vector of length {len(p)} is not 2^k")
        cols.append(list(range(at, at + k)))
        at += k
    return cols


def parity_bias(probs, T, masks) -> np.ndarray:
    """``E[(-1)^(a.f)]`` for every mask (tuple of f-bit indices), exactly, in float64."""
    T = np.asarray(T, dtype=np.uint8) & 1
    cols = _channel_columns(probs)
    if T.shape[1] != sum(len(c) for c in cols):
        raise ValueError(f"T has {T.shape[1]} columns, the channels {sum(len(c) for c in cols)} error bits")
    by_k: dict = {}
    for c, p in enumerate(probs):
        by_k.setdefault(len(cols[c]), []).append(c)
    out = np.ones(len(masks), dtype=np.float64)
    for lo in range(0, len(masks), 256):  # (bounded memory for thousands of masks over thousands of channels)
        part = masks[lo:lo + 256]
        # s[m, j] = a_m . T[:, j] mod 2: whether error bit j flips the parity of mask m
        s = np.zeros((len(part), T.shape[1]), dtype=np.uint8)
        for m, a in enumerate(part):
            for i in a:
                s[m] ^= T[i]
        for k, chans in by_k.items():
            if k == 0:
                continue
            P = np.array([np.asarray(probs[c], dtype=np.float64) for c in chans])  # [Nc, 2^k]
            bits = ((np.arange(1 << k)[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint8)  # [2^k, k]
            idx = np.array([cols[c] for c in chans])  # [Nc, k]
            par = (s[:, idx] @ bits.T) & 1  # [M, Nc, 2^k]
            term = np.einsum("co,mco->mc", P, 1.0 - 2.0 * par)
            out[lo:lo + len(part)] *= np.prod(term, axis=1)
    return out


def mask_words(mask, words: int) -> dict:
    """``{word index: uint64 bit mask}`` of the words a mask touches."""
    d: dict = {}
    for i in mask:
        w = i >> 6
        if w >= words:
            raise ValueError(f"bit {i} beyond {words} words")
        d[w] = d.get(w, 0) ^ (1 << (i & 63))
    return {w: np.uint64(v) for w, v in d.items() if v}


def bit_counts(packed: np.ndarray) -> np.ndarray:
    """Number of rows in which each of the ``64 * words`` bits is set."""
    B, W = packed.shape
    cnt = np.zeros(64 * W, dtype=np.int64)
    by = packed.view(np.uint8).reshape(B, W * 8)
    chunk = max(1, (1 << 25) // (64 * W))  # (32 M unpacked bytes at a time)
    for lo in range(0, B, chunk):
        cnt += np.unpackbits(by[lo:lo + chunk], axis=1, bitorder="little").sum(axis=0, dtype=np.int64)
    return cnt


def empirical_bias(packed: np.ndarray, masks) -> np.ndarray:
    """Mean of ``(-1)^(a.f)`` over the rows, per mask.  Singletons come from one pass of bit counts; every other mask touches
    only the words it uses (an XOR of masked words, then ``np.bitwise_count``)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    B, W = packed.shape
    out = np.empty(len(masks), dtype=np.float64)
    singles = {m for m, a in enumerate(masks) if len(a) == 1}
    if singles:
        cnt = bit_counts(packed)
        for m in singles:
            out[m] = 1.0 - 2.0 * cnt[masks[m][0]] / B
    for m, a in enumerate(masks):
        if m in singles:
            continue
        mw = mask_words(a, W)
        if not mw:
            out[m] = 1.0
            continue
        acc = np.zeros(B, dtype=np.uint64)
        for w, v in mw.items():
            acc ^= packed[:, w] & v
        odd = int(np.count_nonzero(np.bitwise_count(acc) & 1))
        out[m] = 1.0 - 2.0 * odd / B
    return out


def z_bound(n_tests: int, alpha: float = FAMILY_ALPHA) -> float:
    """Two-sided normal quantile of ``alpha / n_tests`` (Bonferroni)."""
    from statistics import NormalDist

    return NormalDist().inv_cdf(1.0 - alpha / (2.0 * max(1, n_tests)))


def check_biases(got: np.ndarray, want: np.ndarray, n: int, masks=None, alpha: float = FAMILY_ALPHA) -> None:
    """Every empirical bias within the Bonferroni bound of its exact value, with the exact variance ``(1 - mu^2) / n`` of a
    mean of n independent +-1 draws.  A bias of exactly +-1 (a parity the model fixes) must come out exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    z = z_bound(len(want), alpha)
    var = np.maximum(1.0 - want * want, 0.0) / n
    fixed = var < 1e-15
    bad = []
    for m in np.nonzero(fixed)[0]:
        if got[m] != np.round(want[m]):
            bad.append((m, got[m], want[m], math.inf))
    sd = np.sqrt(np.where(fixed, 1.0, var))
    zz = np.abs(got - want) / sd
    for m in np.nonzero(~fixed & (zz > z))[0]:
        bad.append((m, got[m], want[m], zz[m]))
    if bad:
        lines = [f"mask {masks[m] if masks is not None else m}: got {g:.6f}, exact {w:.6f}, |z| = {s:.1f}" for m, g, w, s in bad[:12]]
        raise AssertionError(f"{len(bad)} of {len(want)} parities outside {z:.2f} sigma (n = {n}):\n" + "\n".join(lines))


def class_fire_counts(packed: np.ndarray, bits, M: int) -> tuple:
    """Fires of the given bits, summed over the bits, per position class ``shot mod M``; and the rows per class."""
    B = packed.shape[0]
    hits = np.zeros(B, dtype=np.int64)
    by_word: dict = {}
    for b in bits:
        by_word[b >> 6] = by_word.get(b >> 6, 0) | (1 << (b & 63))
    for w, v in by_word.items():
        hits += np.bitwise_count(packed[:, w] & np.uint64(v)).astype(np.int64)
    cls = np.arange(B) % M
    return np.bincount(cls, weights=hits, minlength=M).astype(np.int64), np.bincount(cls, minlength=M)


def check_position_classes(packed: np.ndarray, bits, rate: float, M: int, alpha: float = FAMILY_ALPHA) -> None:
    """The bits (each driven by a one-bit channel of its own, all with the same fire rate) fire at the exact rate in every
    position class ``shot mod M`` - tile or segment seams are where an off-by-one shifts a class - and in the last partial
    tile as a class of its own.  Fires of different bits are independent: a class of r rows over k bits is Binomial(r k, rate)."""
    B = packed.shape[0]
    k = len(bits)
    fires, rows = class_fire_counts(packed, bits, M)
    groups = [(f"class {c} (mod {M})", fires[c], rows[c]) for c in range(M) if rows[c]]
    tail = B % M
    if B > M and tail:
        f_tail, _ = class_fire_counts(packed[B - tail:], bits, tail)
        groups.append(("the last partial tile", int(f_tail.sum()), tail))
    # and the first tile's rows: a block that starts one row late or early shows here
    f_head, _ = class_fire_counts(packed[:min(B, M)], bits, min(B, M))
    groups.append(("the first tile", int(f_head.sum()), min(B, M)))
    z = z_bound(len(groups), alpha)
    bad = []
    for name, f, r in groups:
        n = r * k
        sd = math.sqrt(n * rate * (1 - rate))
        if sd == 0.0:
            if f != round(n * rate):
                bad.append(f"{name}: {f} fires of {n}, exactly {n * rate:.0f} expected")
        elif abs(f - n * rate) > z * sd:
            bad.append(f"{name}: {f} fires of {n}, {n * rate:.1f} expected, |z| = {abs(f - n * rate) / sd:.1f}")
    if bad:
        raise AssertionError(f"{len(bad)} of {len(groups)} position classes off (bound {z:.2f} sigma):\n" + "\n".join(bad[:12]))


def enumerate_law(probs, T) -> dict:
    """The full distribution of the f row by brute force over every joint outcome (tiny models only): ``{f as int: prob}``."""
    T = np.asarray(T, dtype=np.uint8) & 1
    cols = _channel_columns(probs)
    law = {0: 1.0}
    for c, p in enumerate(probs):
        nxt: dict = {}
        for o, po in enumerate(np.asarray(p, dtype=np.float64)):
            if po == 0.0:
                continue
            flip = 0
            for i, j in enumerate(cols[c]):
                if (o >> i) & 1:
                    flip ^= int(sum(int(T[r, j]) << r for r in range(T.shape[0])))
            for f, pf in law.items():
                nxt[f ^ flip] = nxt.get(f ^ flip, 0.0) + pf * po
        law = nxt
    return law


def deterministic_row(probs, T) -> np.ndarray:
    """The f row (``uint8[num_f]``) of a model whose every channel has one outcome of probability 1: the XOR of the patterns."""
    T = np.asarray(T, dtype=np.uint8) & 1
    cols = _channel_columns(probs)
    row = np.zeros(T.shape[0], dtype=np.uint8)
    for c, p in enumerate(probs):
        p = np.asarray(p, dtype=np.float64)
        nz = np.nonzero(p)[0]
        if len(nz) != 1 or p[nz[0]] != 1.0:
            raise ValueError(f"channel {c} is not deterministic: {p}")
        for i, j in enumerate(cols[c]):
            if (nz[0] >> i) & 1:
                row ^= T[:, j]
    return row


def standard_masks(num_f: int, groups, rng: np.random.Generator, n_cross: int = 40, n_triples: int = 30, singles=None) -> list:
    """Masks that a kernel gets wrong in different ways: every singleton bit (or ``singles``), pairs inside each channel's
    support (``groups``: lists of the f bits a channel drives), pairs across channels, and random triples across word
    boundaries."""
    masks = [(i,) for i in (range(num_f) if singles is None else singles)]
    for g in groups:
        g = sorted(set(g))
        for a in range(len(g)):
            for b in range(a + 1, len(g)):
                masks.append((g[a], g[b]))
    if num_f >= 2:
        for _ in range(n_cross):
            a, b = rng.choice(num_f, size=2, replace=False)
            masks.append((int(a), int(b)))
    if num_f >= 3:
        words = max(1, (num_f + 63) // 64)
        for t in range(n_triples):
            if words > 1:  # one bit each from (up to) three different words
                ws = rng.choice(words, size=min(3, words), replace=False)
                picks = [int(min(num_f - 1, w * 64 + rng.integers(64))) for w in ws]
                while len(set(picks)) < 3:
                    picks.append(int(rng.integers(num_f)))
                masks.append(tuple(sorted(set(picks)))[:3])
            else:
                masks.append(tuple(int(x) for x in sorted(rng.choice(num_f, size=3, replace=False))))
    seen, out = set(), []
    for m in masks:
        key = tuple(sorted(m))
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out
