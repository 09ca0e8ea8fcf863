"""Fixed-weight fault sampling without a device (``tsim_amd.fixed_weight``): the weight law and the split tables against exact
rational arithmetic, the position rule on the integers, the law of the numpy statement ``fixed_weight_rows_host`` (class
counts, site marginals, outcomes, whole rows against enumeration), full weight, independence from how a request is cut, the
first-order failures of the d = 3 memory circuit under the union-find decoder, ``combine`` and every refusal.

Statistical limits are the 1 - 1e-6 quantile of the chi-square law of the statistic; the keys are fixed and the statement is
integer arithmetic on tables fixed by float64 arithmetic, so a run that passes here passes everywhere."""

import ctypes as C
import dataclasses
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from test_frame import KEY, word_bits

from tsim_amd import _lib, circuits, faults
from tsim_amd import fixed_weight as fw
from tsim_amd.channels import error_probs, pauli_channel_1_probs
from tsim_amd.clifford import CliffordCircuit, pauli_channel_2_probs
from tsim_amd.decode import UnionFindDecoder

DEP2 = lambda p: pauli_channel_2_probs(*([p / 15] * 15))  # noqa: E731
ALPHA = 1e-6


# ---- helpers ----------------------------------------------------------------------------------------------------------------

def plain_form(classes, n_out: int = 3, seed: int = 0) -> faults.FaultForm:
    """``classes`` = ``[(outcome vector, sites)]`` in class order; every error bit flips one or two of ``n_out`` outputs."""
    rng = np.random.default_rng(seed)
    chans = [np.asarray(p, np.float64) for p, n in classes for _ in range(n)]
    masks, e = [0] * n_out, 0
    for p in chans:
        for _ in range(int(np.log2(len(p)))):
            for j in rng.choice(n_out, size=1 + int(rng.integers(min(2, n_out))), replace=False):
                masks[int(j)] |= 1 << e
            e += 1
    return faults.build_form(chans, e, masks, rng.integers(0, 2, size=n_out), n_out)


def exact_law(form):
    """``(n, p, a, E)`` in rationals: ``a[c][m] = C(n_c, m) o_c^m`` and ``E[c][r]`` for ``r = 0 .. n_sites``."""
    n, pf = fw.class_odds(form)
    n, p = [int(v) for v in n], [Fraction(float(v)) for v in pf]
    R = sum(n)
    a = [[math.comb(nc, m) * (pc / (1 - pc)) ** m for m in range(R + 1)] for nc, pc in zip(n, p)]
    E = [None] * (len(n) + 1)
    E[len(n)] = [Fraction(1)] + [Fraction(0)] * R
    for c in range(len(n) - 1, -1, -1):
        E[c] = [sum(a[c][m] * E[c + 1][r - m] for m in range(r + 1)) for r in range(R + 1)]
    return n, p, a, E


def gamma_q(a: float, x: float) -> float:
    """The regularised upper incomplete gamma function (series below ``a + 1``, continued fraction above)."""
    if x <= 0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1:
        term = total = 1.0 / a
        for i in range(1, 100000):
            term *= x / (a + i)
            total += term
            if term < total * 1e-17:
                break
        return 1.0 - lead * total
    b, c, d = x + 1 - a, 1e300, 1.0 / (x + 1 - a)
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2
        d = 1.0 / (an * d + b) if an * d + b else 1e300
        c = b + an / c if b + an / c else 1e-300
        h *= d * c
        if abs(d * c - 1) < 1e-16:
            break
    return lead * h


def chi2_limit(df: int, alpha: float = ALPHA) -> float:
    """The ``1 - alpha`` quantile of chi-square with ``df`` degrees of freedom, by bisection."""
    lo, hi = 0.0, df + 100.0 * math.sqrt(df) + 100.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if gamma_q(df / 2, mid / 2) > alpha else (lo, mid)
    return hi


def check_chi2(observed, probs, what) -> None:
    """Counts against cell probabilities (summing to 1); cells expecting fewer than 5 are pooled."""
    observed, probs = np.asarray(observed, np.float64), np.asarray([float(p) for p in probs])
    assert abs(probs.sum() - 1) < 1e-9, what
    n = observed.sum()
    big = probs * n >= 5
    obs, exp = list(observed[big]), list(probs[big] * n)
    if (~big).any() and probs[~big].sum() > 0:
        obs.append(observed[~big].sum())
        exp.append(probs[~big].sum() * n)
    else:
        assert observed[~big].sum() == 0, what
    obs, exp = np.array(obs), np.array(exp)
    stat, df = float(((obs - exp) ** 2 / exp).sum()), len(obs) - 1
    assert df >= 1 and stat <= chi2_limit(df), (what, stat, df, chi2_limit(df))


def test_chi2_limit_against_known_quantiles():
    assert abs(chi2_limit(1, 0.05) - 3.841459) < 1e-5 and abs(chi2_limit(10, 0.01) - 23.209251) < 1e-5
    assert abs(chi2_limit(1) - 23.92813) < 1e-4 and abs(chi2_limit(100, 0.001) - 149.4493) < 1e-3


def fired_sites(form, e_words, B) -> np.ndarray:
    """``bool[B, n_sites]`` (class-major) and the outcome value of every site, from the statement's error bits."""
    bits = word_bits(e_words, B).astype(np.int64)
    val = np.zeros((B, form.n_sites), np.int64)
    for c in range(form.n_classes):
        for s in range(form.class_ptr[c], form.class_ptr[c + 1]):
            for b in range(int(form.table_bits[c])):
                val[:, s] |= bits[:, form.site_e0[s] + b] << b
    return val


# ---- the tables against exact arithmetic ----------------------------------------------------------------------------------------

TABLE_FORMS = {"one class": [(error_probs(0.3), 5)],
               "three classes": [(error_probs(0.3), 1), (error_probs(1e-3), 7), (error_probs(0.05), 40)]}


@pytest.mark.parametrize("name", sorted(TABLE_FORMS))
def test_tables_against_exact_arithmetic(name):
    form, kmax = plain_form(TABLE_FORMS[name]), 6
    n, p, a, E = exact_law(form)
    R, n_cls = sum(n), len(n)
    # the weight law and its tail
    p0 = math.prod((1 - pc) ** nc for nc, pc in zip(n, p))
    law, tail = fw.weight_law(form, kmax)
    assert law.dtype == np.float64 and law.shape == (kmax + 1,)
    for k in range(kmax + 1):
        want = p0 * E[0][k] if k <= R else Fraction(0)
        assert abs(Fraction(float(law[k])) - want) <= want * Fraction(1, 10**12), (k, law[k], float(want))
    want = p0 * sum(E[0][kmax + 1:])
    assert abs(Fraction(tail) - want) <= want * Fraction(1, 10**9), (tail, float(want))
    assert sum(map(Fraction, map(float, law))) + Fraction(tail) - 1 < Fraction(1, 10**14)
    # the split thresholds
    thr = fw.split_thresholds(form, kmax)
    assert thr.dtype == np.uint32 and thr.shape == (n_cls, kmax + 1, kmax + 1)
    for c in range(n_cls):
        rest = sum(n[c + 1:])
        for r in range(kmax + 1):
            row = [int(v) for v in thr[c, r]]
            if r > rest + n[c]:  # no split can reach the row
                assert row == [0xFFFFFFFF] * (kmax + 1)
                continue
            hi = min(r, n[c])
            assert row == sorted(row) and row[hi:] == [0xFFFFFFFF] * (kmax + 1 - hi)
            cdf = [Fraction(v, 2**32) for v in row[:hi]] + [Fraction(1)]
            for m in range(hi + 1):
                got = cdf[m] - (cdf[m - 1] if m else 0)
                want = a[c][m] * E[c + 1][r - m] / E[c][r]
                assert abs(got - want) <= Fraction(1, 2**31), (c, r, m, float(got), float(want))
                if r - m > rest:  # it would leave more than the later classes can take: exactly 0
                    assert want == 0 and row[m] == 0
    # one table of kmax = 6 serves every k: the rows it shares with the table of kmax = 3 are the same
    assert np.array_equal(thr[:, :4, :4], fw.split_thresholds(form, 3))
    assert np.array_equal(fw.weight_law(form, 3)[0], law[:4])


def test_tables_of_huge_classes_and_tiny_rates_are_finite_and_ordered():
    small = plain_form([(error_probs(1e-9), 2), (error_probs(0.5), 2), (error_probs(1 - 1e-12), 2), (DEP2(1e-3), 2)])
    n = [1 << 25, 3, 1 << 25, 1000]
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    chan = np.repeat(np.array([0, 2, 4, 6], np.int8), n)  # (the first channel of every class of `small`)
    big = dataclasses.replace(small, class_ptr=ptr, site_chan=chan)
    for kmax in (0, 5, 32):
        thr = fw.split_thresholds(big, kmax).astype(np.int64)
        assert (np.diff(thr, axis=2) >= 0).all() and (thr[:, :, -1] == 0xFFFFFFFF).all()
        law, tail = fw.weight_law(big, kmax)
        assert np.isfinite(law).all() and (law >= 0).all() and 0 <= tail <= 1 and abs(law.sum() + tail - 1) < 1e-9
    # 2^25 sites at 1e-9 alone: a Poisson law of mean 2^25 1e-9
    one = dataclasses.replace(small, class_ptr=ptr[:2], site_chan=chan[:n[0]], table_bits=small.table_bits[:1],
                              table_ptr=small.table_ptr[:2], table_gap=small.table_gap[:1])
    law, tail = fw.weight_law(one, 4)
    mu = (1 << 25) * 1e-9
    want = [math.exp(-mu) * mu**k / math.factorial(k) for k in range(5)]
    assert np.allclose(law, want, rtol=1e-6, atol=0) and abs(tail - mu**5 / 120 * math.exp(-mu)) < 0.02 * tail
    # the mass far above kmax: the tail is all there is
    law, tail = fw.weight_law(plain_form([(error_probs(0.5), 3000)], n_out=1), 32)
    assert law.max() < 1e-300 and tail == 1.0


# ---- the position rule on the integers ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 7, 1000, 1 << 25])
def test_position_rule(n):
    keep, reject = (1 << 32) // n, (1 << 32) % n
    for pos in sorted({0, 1 % n, n // 2, n - 1}):
        first, last = -((-((pos << 32) + reject)) // n), (((pos + 1) << 32) - 1) // n  # t = x0 n in [pos 2^32 + reject, (pos + 1) 2^32)
        assert last - first + 1 == keep, (n, pos)
        x0 = [v for v in (first - 1, first, last, last + 1) if 0 <= v < 1 << 32]
        got_pos, ok = fw.position_of(np.array(x0, np.uint32), n)
        for v, gp, go in zip(x0, got_pos.tolist(), ok.tolist()):  # (the neighbours belong to another position or are rejected)
            assert (gp == pos and go) == (first <= v <= last), (n, pos, v)
    x0 = np.random.default_rng(n).integers(0, 1 << 32, size=1000, dtype=np.uint64)
    got_pos, ok = fw.position_of(x0.astype(np.uint32), n)
    t = [int(v) * n for v in x0]
    assert got_pos.tolist() == [v >> 32 for v in t] and ok.tolist() == [(v & 0xFFFFFFFF) >= reject for v in t]


# ---- the law of the statement ---------------------------------------------------------------------------------------------------

LAW_CLASSES = [(DEP2(0.3), 4), (error_probs(0.05), 40), (pauli_channel_1_probs(0.1, 0.2, 0.05), 7)]
LAW_K, LAW_B = 4, 1 << 16


@pytest.fixture(scope="module")
def law_rows():
    form = plain_form(LAW_CLASSES, n_out=5, seed=3)
    rows, e = fw.fixed_weight_rows_host(form, LAW_K, 64 * 3, LAW_B, (7, 11), return_e=True)
    val = fired_sites(form, e, LAW_B)
    val.setflags(write=False)
    return form, rows, val


def test_every_row_has_exactly_k_fired_sites(law_rows):
    form, rows, val = law_rows
    assert ((val != 0).sum(axis=1) == LAW_K).all()
    want = np.tile(form.out_const, (LAW_B, 1))  # the rows are the error bits through the column lists
    bits = np.zeros((LAW_B, form.num_e), np.uint8)
    for s in range(form.n_sites):
        c = int(np.searchsorted(form.class_ptr, s, side="right")) - 1
        for b in range(int(form.table_bits[c])):
            bits[:, form.site_e0[s] + b] = (val[:, s] >> b) & 1
    for e in range(form.num_e):
        for j in form.cols[form.col_ptr[e]:form.col_ptr[e + 1]]:
            want[:, j] ^= bits[:, e]
    assert np.array_equal(rows, want)


def test_law_of_the_class_counts(law_rows):
    form, _, val = law_rows
    n, p, a, E = exact_law(form)
    ptr = form.class_ptr
    k_c = np.stack([(val[:, ptr[c]:ptr[c + 1]] != 0).sum(axis=1) for c in range(3)], axis=1)
    cells = [kc for kc in itertools.product(range(LAW_K + 1), repeat=3) if sum(kc) == LAW_K]
    probs = [a[0][x] * a[1][y] * a[2][z] / E[0][LAW_K] for x, y, z in cells]
    observed = [int(((k_c == kc).all(axis=1)).sum()) for kc in cells]
    assert sum(observed) == LAW_B and sum(1 for q in probs if q * LAW_B >= 5) >= 8
    check_chi2(observed, probs, "class counts")


def test_law_of_the_sites_and_outcomes(law_rows):
    form, _, val = law_rows
    for c, (probs, n_c) in enumerate(LAW_CLASSES):
        mine = val[:, form.class_ptr[c]:form.class_ptr[c + 1]]
        # given how many sites of the class fire, every site is as likely as the others: marginal k_c / n_c
        check_chi2((mine != 0).sum(axis=0), [Fraction(1, n_c)] * n_c, f"sites of class {c}")
        # the outcomes of the sites that fired: the table's law given that the site fires
        probs = np.asarray(probs, np.float64)
        if len(probs) > 2:
            fired = mine[mine != 0]
            check_chi2(np.bincount(fired, minlength=len(probs))[1:], probs[1:] / probs[1:].sum(), f"outcomes of class {c}")
    # two sites of one class fire together as often as any other pair: the firing set is uniform over the subsets
    mine = val[:, form.class_ptr[1]:form.class_ptr[2]] != 0
    two = mine[mine.sum(axis=1) == 2]
    pairs = list(itertools.combinations(range(40), 2))
    index = {pq: i for i, pq in enumerate(pairs)}
    where = np.sort(np.argsort(~two, axis=1, kind="stable")[:, :2], axis=1)
    observed = np.bincount([index[tuple(w)] for w in where.tolist()], minlength=len(pairs))
    assert len(two) > 5 * len(pairs)
    check_chi2(observed, [Fraction(1, len(pairs))] * len(pairs), "pairs of class 1")


BRUTE_CLASSES = [(error_probs(0.2), 5), (error_probs(0.05), 4), (pauli_channel_1_probs(0.1, 0.2, 0.05), 3)]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_whole_rows_against_enumeration(k):
    """12 sites in 3 classes, 3 outputs: the law of the whole row given K = k, every k-subset with every outcome enumerated."""
    form = plain_form(BRUTE_CLASSES, n_out=3, seed=5)
    assert (form.n_sites, form.n_classes, form.n_out) == (12, 3, 3)
    cls = np.searchsorted(form.class_ptr, np.arange(12), side="right") - 1
    lists = [form.cols[form.col_ptr[e]:form.col_ptr[e + 1]].tolist() for e in range(form.num_e)]
    const = int(np.packbits(form.out_const, bitorder="little")[0])
    weight = [0.0] * 8
    for sites in itertools.combinations(range(12), k):
        tables = [np.asarray(BRUTE_CLASSES[cls[s]][0], np.float64) for s in sites]
        for outcome in itertools.product(*[range(1, len(t)) for t in tables]):
            w, row = 1.0, const
            for s, t, o in zip(sites, tables, outcome):
                w *= t[o] / t[0]  # odds of the class times the outcome's share
                for b in range(int(form.table_bits[cls[s]])):
                    if (o >> b) & 1:
                        for j in lists[form.site_e0[s] + b]:
                            row ^= 1 << j
            weight[row] += w
    B = 40000
    rows = fw.fixed_weight_rows_host(form, k, 0, B, (k, 99))
    observed = np.bincount(np.packbits(rows, axis=1, bitorder="little")[:, 0], minlength=8)
    assert sum(1 for w in weight if w > 0) >= 4
    check_chi2(observed, np.array(weight) / sum(weight), f"rows at k = {k}")


def test_full_weight_fires_every_site():
    """k = all 8 sites, among them classes of 1 and 2 sites: the rejection loop's worst case (the last free position)."""
    form = plain_form([(error_probs(0.3), 1), (DEP2(0.1), 2), (error_probs(0.01), 5)], n_out=4, seed=8)
    assert form.n_sites == 8
    rows, e = fw.fixed_weight_rows_host(form, 8, 0, 500, KEY, return_e=True)
    val = fired_sites(form, e, 500)
    assert (val != 0).all() and len(np.unique(val[:, 1:3], axis=0)) > 50 and len(np.unique(rows, axis=0)) > 1
    rows0, e0 = fw.fixed_weight_rows_host(form, 0, 0, 500, KEY, return_e=True)
    assert not e0.any() and (rows0 == form.out_const).all()


def test_rows_do_not_depend_on_how_the_request_is_cut():
    form = plain_form(LAW_CLASSES, n_out=5, seed=3)
    whole = fw.fixed_weight_rows_host(form, 3, 0, 1000, KEY)
    for m in (1, 63, 64, 65, 640):
        assert np.array_equal(fw.fixed_weight_rows_host(form, 3, 0, m, KEY), whole[:m]), m
    assert np.array_equal(fw.fixed_weight_rows_host(form, 3, 192, 1000 - 192, KEY), whole[192:])
    assert not np.array_equal(fw.fixed_weight_rows_host(form, 3, 0, 1000, (KEY[0], KEY[1] + 1)), whole)
    assert not np.array_equal(fw.fixed_weight_rows_host(form, 2, 0, 1000, KEY), whole)
    last = fw.fixed_weight_rows_host(form, 3, 2**38 - 64, 64, KEY)
    assert last.shape == (64, 5) and np.array_equal(fw.fixed_weight_rows_host(form, 3, 2**32 - 64, 128, KEY)[64:],
                                                    fw.fixed_weight_rows_host(form, 3, 2**32, 64, KEY))
    with pytest.raises(ValueError, match="multiple of 64"):
        fw.fixed_weight_rows_host(form, 3, 32, 10, KEY)
    with pytest.raises(ValueError, match="2\\^38"):
        fw.fixed_weight_rows_host(form, 3, 2**38 - 64, 65, KEY)
    assert fw.noise_key(KEY) != faults.noise_key(KEY)  # a stream of its own


# ---- the sampler and the first-order failures of the d = 3 memory circuit ----------------------------------------------------

D3 = dict(after_clifford_depolarization=1e-3, before_measure_flip_probability=1e-3)


def single_faults(form, uf):
    """Every single-site fault with its probability given K = 1 and whether the decoder gets it wrong:
    ``[(class, site, outcome value, probability, wrong)]``."""
    n, p = fw.class_odds(form)
    odds = n * p / (1 - p)
    nd = form.num_detectors
    lists = [form.cols[form.col_ptr[e]:form.col_ptr[e + 1]] for e in range(form.num_e)]
    out, rows = [], []
    for c in range(form.n_classes):
        table = np.asarray(form.channel_probs[int(form.site_chan[form.class_ptr[c]])], np.float64)
        for s in range(form.class_ptr[c], form.class_ptr[c + 1]):
            for o in range(1, len(table)):
                if table[o] > 0:
                    row = np.zeros(form.n_out, np.bool_)
                    for b in range(int(form.table_bits[c])):
                        if (o >> b) & 1:
                            row[lists[form.site_e0[s] + b]] ^= True
                    rows.append(row)
                    out.append((c, s, o, odds[c] / odds.sum() / n[c] * table[o] / table[1:].sum()))
    rows = np.array(rows)
    wrong = (uf.decode(rows[:, :nd]) != rows[:, nd:]).any(axis=1)
    return [(*f, bool(w)) for f, w in zip(out, wrong)]


def test_first_order_failures_of_the_d3_memory_circuit():
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3, **D3))
    form, uf = c.compile_faults(), UnionFindDecoder.from_circuit(c)
    assert (form.n_sites, form.n_classes) == (129, 3)
    singles = single_faults(form, uf)
    bad = [f for f in singles if f[4]]
    assert len(singles) == 1185 and abs(sum(f[3] for f in singles) - 1) < 1e-12
    # four outcomes of ONE two-qubit depolarising site are decoded wrongly: they flip detectors 1 and 2 and no observable
    assert len(bad) == 4 and len({f[1] for f in bad}) == 1 and form.table_bits[bad[0][0]] == 4
    f1 = sum(f[3] for f in bad)
    assert abs(f1 - 4 / 15 / 129) < 1e-9  # (every site fires with 1e-3: the sites are equally likely)
    law, _ = fw.weight_law(form, 4)
    assert np.allclose(law, [0.879, 0.113, 7.27e-3, 3.08e-4, 9.7e-6], rtol=5e-3)
    # the sampler at fault_weight = 1 fails at that rate
    s = c.compile_detector_sampler(seed=11, method="faults", fault_weight=1)
    assert isinstance(s, fw.CompiledFixedWeightDetectorSampler) and s.fault_weight == 1 and "exactly 1" in repr(s)
    assert np.array_equal(s.weight_law(4)[0], law) and np.array_equal(s.weight_law()[0], law[:2])
    n = 20000
    rows = fw.fixed_weight_rows_host(form, 1, 0, n, s._next_key()).view(np.bool_)
    nd = form.num_detectors
    wrong = int((uf.decode(rows[:, :nd]) != rows[:, nd:]).any(axis=1).sum())
    assert abs(wrong - n * f1) <= 5 * math.sqrt(n * f1 * (1 - f1)), (wrong, n * f1)
    # with data depolarisation before every round as well, every single fault is decoded correctly
    c3 = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3, before_round_data_depolarization=1e-3, **D3))
    singles = single_faults(c3.compile_faults(), UnionFindDecoder.from_circuit(c3))
    assert len(singles) == 1266 and not any(f[4] for f in singles)


def test_sampler_rows_are_the_statement():
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3, **D3))
    mk = lambda k: c.compile_detector_sampler(seed=5, method="faults", fault_weight=k)  # noqa: E731
    form = c.compile_faults()
    rows = fw.fixed_weight_rows_host(form, 3, 0, 640, mk(3)._next_key()).view(np.bool_)
    nd = form.num_detectors
    assert np.array_equal(mk(3).sample(640), rows[:, :nd])
    a, b = mk(3).sample(640, separate_observables=True)
    assert np.array_equal(a, rows[:, :nd]) and np.array_equal(b, rows[:, nd:])
    assert not np.array_equal(mk(2).sample(640), rows[:, :nd])
    assert not np.array_equal(c.compile_detector_sampler(seed=5, method="faults").sample(640), rows[:, :nd])  # today's sampler stays
    s = mk(3)
    s.set_fault_weight(0)
    assert not s.sample(64).any()
    with pytest.raises(ValueError, match="exceeds 3"):
        s.set_fault_weight(4)


# ---- combine ----------------------------------------------------------------------------------------------------------------------

def test_combine():
    got = fw.combine([0.5, 0.25, 0.125], 0.125, [100, 200, 400], [0, 20, 100], [0, 1, 2])
    assert got.f.tolist() == [0.0, 0.1, 0.25] and got.estimate == 0.25 * 0.1 + 0.125 * 0.25 and got.tail == 0.125
    assert abs(got.std_error - math.sqrt(0.25**2 * 0.1 * 0.9 / 200 + 0.125**2 * 0.25 * 0.75 / 400)) < 1e-15
    assert got.decoder_misses.tolist() == [0, 1, 2] and got.shots.tolist() == [100, 200, 400] and got.law.tolist() == [0.5, 0.25, 0.125]
    none = fw.combine([0.9, 0.1], 0.0, [0, 10], [0, 10])
    assert none.estimate == 0.1 and none.std_error == 0.0 and none.f.tolist() == [0.0, 1.0]
    for bad in (([0.5], 0, [1, 2], [0, 0]), ([0.5, 0.5], 0, [1, 2], [2, 0]), ([0.5, 0.5], 0, [1, -2], [0, 0])):
        with pytest.raises(ValueError):
            fw.combine(*bad)


# ---- every refusal ----------------------------------------------------------------------------------------------------------------

def test_refusals():
    form = plain_form(BRUTE_CLASSES)
    assert fw.MAX_FAULT_WEIGHT == 32
    with pytest.raises(ValueError, match="exceeds the 12 noise sites"):
        fw.fixed_weight_rows_host(form, 13, 0, 64, KEY)
    with pytest.raises(ValueError, match="MAX_FAULT_WEIGHT"):
        fw.fixed_weight_rows_host(plain_form([(error_probs(0.1), 40)]), 33, 0, 64, KEY)
    for k in (-1, 1.5):
        with pytest.raises(ValueError, match="non-negative integer"):
            fw.fixed_weight_rows_host(form, k, 0, 64, KEY)
    for kmax in (-1, 33):
        with pytest.raises(ValueError, match="kmax"):
            fw.weight_law(form, kmax)
        with pytest.raises(ValueError, match="kmax"):
            fw.split_thresholds(form, kmax)
    always = plain_form([(error_probs(0.1), 3), (error_probs(1.0), 1)])
    for call in (lambda: fw.weight_law(always, 2), lambda: fw.split_thresholds(always, 2),
                 lambda: fw.fixed_weight_rows_host(always, 1, 0, 64, KEY)):
        with pytest.raises(NotImplementedError, match="probability 1"):
            call()
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3, **D3))
    for method in ("autoregressive", "frame"):
        with pytest.raises(ValueError, match='fault_weight needs method="faults"'):
            c.compile_detector_sampler(method=method, fault_weight=1)
    with pytest.raises(ValueError, match="fault_weight needs"):
        c.compile_detector_sampler(fault_weight=0)
    with pytest.raises(ValueError, match="MAX_FAULT_WEIGHT"):
        c.compile_detector_sampler(method="faults", fault_weight=33)
    with pytest.raises(ValueError, match="noise sites"):
        CliffordCircuit("X_ERROR(0.1) 0 1\nM 0 1\nDETECTOR rec[-1]\nDETECTOR rec[-2]").compile_detector_sampler(method="faults", fault_weight=3)
    with pytest.raises(NotImplementedError, match="probability 1"):
        CliffordCircuit("X_ERROR(1) 0\nM 0\nDETECTOR rec[-1]").compile_detector_sampler(method="faults", fault_weight=1)
    uf = UnionFindDecoder.from_circuit(c)
    with pytest.raises(ValueError, match="post-selection"):
        fw.stratified_error_rate(c, uf, 100, kmax=2, postselection_mask=np.zeros(uf.num_detectors, np.bool_))
    with pytest.raises(ValueError, match="MAX_FAULT_WEIGHT"):
        fw.stratified_error_rate(c, uf, 100, kmax=40)


def test_c_side_checks_need_no_device():
    lib = _lib.load()
    table = np.zeros(4, np.uint32)
    assert lib.tsim_faults_set_split(None, 1, table.ctypes.data) == -22 and b"NULL" in lib.tsim_last_error()
    assert lib.tsim_faults_sample_weight_device(None, 1, 64, 0, 1, 2, None, 8, 1, 0, 1, None) == -22
    assert lib.tsim_faults_weight_info(None, (C.c_int64 * 8)()) == -22
