"""The affine measurement sampler without a device: the numpy statement of the affine map against a per-shot loop, the
affine form of ``CliffordCircuit.compile_affine_measurements()``, and ``compile_sampler(method=)``."""

import time

import numpy as np
import pytest

from tsim_amd import affine, circuits, prng
from tsim_amd.clifford import CliffordCircuit

B_SET = (1, 63, 64, 65, 200)
FIRST_SHOTS = (0, 64, 64 * (2**20 + 3))


def random_csr(num_f: int, n_random: int, n_out: int, seed: int):
    """Lists of 0 .. 40 columns: some empty, some with a column listed twice (it cancels)."""
    rng = np.random.default_rng(seed)
    n_col = num_f + n_random
    lists = []
    for j in range(n_out):
        k = 0 if (j % 6 == 2 or n_col == 0) else int(rng.integers(0, 41))
        cols = rng.integers(0, max(1, n_col), k).tolist()
        if n_col and j % 5 == 1:
            c = int(rng.integers(0, n_col))
            cols = cols[:38] + [c, c]
        lists.append(cols)
    row_ptr = np.zeros(n_out + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(l) for l in lists])
    cols = np.asarray([c for l in lists for c in l], np.int32)
    return row_ptr, cols, rng.integers(0, 2, n_out).astype(np.uint8)


def brute_force(flip, row_ptr, cols, num_f, f_bits, B, first_shot, key):
    """One shot, one output, one column at a time; random words from ``prng.threefry2x32``, one call per word."""
    words = {}
    out = np.zeros((B, len(flip)), np.uint8)
    for n in range(B):
        g = first_shot + n
        for j in range(len(flip)):
            v = int(flip[j])
            for c in cols[row_ptr[j]:row_ptr[j + 1]]:
                c = int(c)
                if c < num_f:
                    v ^= int(f_bits[n, c])
                else:
                    s, t = c - num_f, g // 64
                    if (s, t) not in words:
                        x0, x1 = prng.threefry2x32(key[0], key[1], s, t)
                        words[s, t] = x0 | (x1 << 32)
                    v ^= (words[s, t] >> (g % 64)) & 1
            out[n, j] = v
    return out


@pytest.mark.parametrize("num_f,n_random,n_out", [(0, 1, 1), (1, 0, 7), (0, 0, 5), (63, 64, 8), (64, 65, 9), (65, 1, 64), (70, 70, 70), (5, 70, 65)])
def test_host_statement_against_brute_force(num_f, n_random, n_out):
    row_ptr, cols, flip = random_csr(num_f, n_random, n_out, seed=1000 * num_f + 10 * n_random + n_out)
    rng = np.random.default_rng(n_out)
    key = (0x9E3779B9, 12345 + n_out)
    for i, B in enumerate(B_SET):
        for q, first_shot in enumerate(FIRST_SHOTS):
            if n_out > 9 and B == 200 and q != i % 3:  # the long loops once per size, each first_shot somewhere
                continue
            f_bits = rng.integers(0, 2, (B, num_f)).astype(np.uint8)
            f_packed = np.packbits(f_bits, axis=1, bitorder="little") if num_f else None
            got = affine.affine_rows_host(flip, row_ptr, cols, num_f, n_random, f_packed, B, first_shot, key)
            want = brute_force(flip, row_ptr, cols, num_f, f_bits, B, first_shot, key)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (B, first_shot)


def test_host_statement_reads_padded_uint64_rows():
    """The f rows as ``ChannelSampler.sample_packed`` gives them: uint64 words, pad bits ignored."""
    num_f, n_random, n_out = 70, 3, 20
    row_ptr, cols, flip = random_csr(num_f, n_random, n_out, seed=5)
    rng = np.random.default_rng(6)
    f_bits = rng.integers(0, 2, (100, num_f)).astype(np.uint8)
    padded = np.ones((100, 128), np.uint8)
    padded[:, :num_f] = f_bits
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint64)
    a = affine.affine_rows_host(flip, row_ptr, cols, num_f, n_random, words, 100, 128, (1, 2))
    b = affine.affine_rows_host(flip, row_ptr, cols, num_f, n_random, np.packbits(f_bits, axis=1, bitorder="little"), 100, 128, (1, 2))
    assert np.array_equal(a, b)


def test_vectorised_threefry_is_prng_threefry():
    rng = np.random.default_rng(0)
    c0, c1 = rng.integers(0, 2**32, 50, dtype=np.uint64), rng.integers(0, 2**32, 50, dtype=np.uint64)
    for key in ((0, 0), (0xFFFFFFFF, 0x12345678), (7, 0xDEADBEEF)):
        x0, x1 = affine.threefry2x32_np(key[0], key[1], c0, c1)
        for i in range(50):
            assert (int(x0[i]), int(x1[i])) == prng.threefry2x32(key[0], key[1], int(c0[i]), int(c1[i]))


def test_create_rejects_bad_descriptions_without_a_device():
    import ctypes as C

    from tsim_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    rp, cols, flip = np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32), np.zeros(2, np.uint8)
    args = lambda rp_, cols_, flip_: (_lib.ptr(rp_), _lib.ptr(cols_), _lib.ptr(flip_), C.byref(h))  # noqa: E731
    assert lib.tsim_affine_create(0, 2, 1, 2, *args(rp, cols, flip)) == -22 and b"cols[1] = 3" in lib.tsim_last_error()
    assert lib.tsim_affine_create(0, 2, 2, 2, *args(np.array([0, 2, 1], np.int32), cols, flip)) == -22
    assert b"decreases" in lib.tsim_last_error()
    assert lib.tsim_affine_create(0, 2, 2, 2, *args(None, cols, flip)) == -22
    assert lib.tsim_affine_create(0, -1, 2, 2, *args(rp, cols, flip)) == -22
    assert lib.tsim_affine_info(None, (C.c_int64 * 8)()) == -22
    with pytest.raises(ValueError):
        affine.AffineHandle(2, 1, rp, cols, flip)


# ---- the affine form ------------------------------------------------------------------------------------------------

WORKED = "H 0 2\nCX 0 1\nM 0 1 2\nCX 2 1\nM 1 !0"


def lists_of(form) -> list:
    return [sorted(form["cols"][form["row_ptr"][i]:form["row_ptr"][i + 1]].tolist()) for i in range(len(form["flip"]))]


def test_worked_example():
    c = CliffordCircuit(WORKED)
    an = c.analyze()
    assert [int(v) for v in an.rec_vals] == [0, 0, 0, 0, 1]
    assert [int(y) for y in an.rec_syms] == [0b01, 0b01, 0b10, 0b11, 0b01]  # {0}, {0}, {1}, {0, 1}, {0}
    form = c.compile_affine_measurements()
    assert form["num_f"] == 0 and form["n_random"] == 2 and form["flip"].tolist() == [0, 0, 0, 0, 1]
    assert lists_of(form) == [[0], [0], [1], [0, 1], [0]]
    assert form["error_transform"].shape == (0, 0) and form["channel_probs"] == []


def affine_space(c: CliffordCircuit) -> set:
    """``{val + S r}`` straight from ``analyze()``: every assignment of the random symbols."""
    an = c.analyze()
    n = max((int(y).bit_length() for y in an.rec_syms), default=0)
    assert n <= 8
    return {bytes((int(v) ^ (bin(int(y) & r).count("1") & 1)) for v, y in zip(an.rec_vals, an.rec_syms)) for r in range(1 << n)}


def symbol_rank(c: CliffordCircuit) -> int:
    basis = []
    for y in c.analyze().rec_syms:
        y = int(y)
        for b in basis:
            y = min(y, y ^ b)
        if y:
            basis.append(y)
    return len(basis)


EXHAUSTIVE = {
    "worked": WORKED,
    "ghz": "H 0\nCX 0 1 1 2 2 3\nM 0 1 2 3",
    "bases": "RX 0\nRX 0\nM 0\nRX 0\nM 0\nR 0\nM 0",
    "mixed": "H 0 1 2\nCX 0 3 1 4\nM 0 3\nH 3\nM 3 1 4 2\nMX 0 1\nM !2",
    "deterministic": "X 0\nM 0 1",
    "surface": circuits.rotated_surface_code_memory(3, 3),
}


@pytest.mark.parametrize("name", sorted(EXHAUSTIVE))
def test_noiseless_rows_fill_the_affine_space(name):
    c = CliffordCircuit(EXHAUSTIVE[name])
    rows = c.compile_sampler(seed=17, method="affine").sample(2**14)
    assert rows.dtype == np.bool_ and rows.shape == (2**14, c.num_measurements)
    got = {r.tobytes() for r in np.unique(rows.view(np.uint8), axis=0)}
    want = affine_space(c)
    assert len(want) == 2 ** symbol_rank(c)
    assert got == want


def test_noiseless_surface_code_rows_convert_to_zero_events():
    c = CliffordCircuit(circuits.rotated_surface_code_memory(3, 3))
    rows = c.compile_sampler(seed=3, method="affine").sample(5000).astype(np.uint8)
    assert (rows.any(axis=0) & ~rows.all(axis=0)).any(), "the records should carry random outcomes"
    row_ptr, cols, ref = c.compile_m2d_converter().csr()  # the converter's map, applied in numpy
    for j in range(len(ref)):
        ev = rows[:, cols[row_ptr[j]:row_ptr[j + 1]]].sum(axis=1) & 1
        assert not (ev ^ ref[j]).any(), j


# ---- compile_sampler(method=) ---------------------------------------------------------------------------------------

def test_method_switch():
    from tsim_amd.sampler import CompiledMeasurementSampler

    c = CliffordCircuit("H 0\nM(0.01) 0\nM 0")
    with pytest.raises(ValueError, match="method"):
        c.compile_sampler(method="bogus")
    a, b = c.compile_sampler(seed=1), c.compile_sampler(seed=1, method="autoregressive")
    assert type(a) is type(b) is CompiledMeasurementSampler
    assert a._program is b._program and a._key == b._key and repr(a) == repr(b)
    s = c.compile_sampler(seed=1, method="affine")
    assert isinstance(s, affine.CompiledAffineMeasurementSampler) and isinstance(s, CompiledMeasurementSampler)
    assert not s._program.components and s._program.num_outputs == 2


def test_same_basis_as_the_autoregressive_form():
    text = circuits.rotated_surface_code_memory(3, 2, after_clifford_depolarization=0.01, before_measure_flip_probability=0.01)
    c = CliffordCircuit(text)
    _prog, probs, et = c.compile_measurements()
    form = c.compile_affine_measurements()
    assert form["num_f"] == et.shape[0] and np.array_equal(form["error_transform"], et)
    assert len(form["channel_probs"]) == len(probs) and all(np.array_equal(p, q) for p, q in zip(form["channel_probs"], probs))


def test_eleven_hundred_records_compile():
    """``H 0`` then 1100 noisy measurements of the qubit: one component of 1100 outputs, 2200 parameters at its last level -
    beyond the 2048 the autoregressive program can have.  The affine form has no levels."""
    c = CliffordCircuit("H 0\n" + "M(0.01) 0\n" * 1100)
    t0 = time.perf_counter()
    form = c.compile_affine_measurements()
    assert time.perf_counter() - t0 < 1.0
    assert form["num_f"] == 1100 and form["n_random"] == 1 and len(form["flip"]) == 1100
    assert 2 * 1100 > 2048
    assert all(l == [i, 1100] for i, l in enumerate(lists_of(form)))  # its own flip bit, and the one random symbol
    rows = c.compile_sampler(seed=2, method="affine", noise="host").sample(4096)
    assert rows.shape == (4096, 1100)
    first = rows[:, :1]
    assert 0.4 < first.mean() < 0.6 and 0.005 < (rows ^ first).mean() < 0.02  # a coin, re-read with 1 % flips


def test_rows_do_not_depend_on_batch_size():
    text = circuits.rotated_surface_code_memory(3, 3, after_clifford_depolarization=0.01, before_measure_flip_probability=0.01)
    c = CliffordCircuit(text)
    want = c.compile_sampler(seed=5, method="affine").sample(3000)
    for bs in (64, 1000, None):
        s = c.compile_sampler(seed=5, method="affine")
        assert np.array_equal(s.sample(3000, batch_size=bs), want), bs
        packed = c.compile_sampler(seed=5, method="affine").sample(3000, bs, True)
        assert np.array_equal(packed, np.packbits(want.view(np.uint8), axis=1, bitorder="little"))
    # one key per request: the second request of a sampler differs from its first, and is reproducible
    s, t = c.compile_sampler(seed=5, method="affine"), c.compile_sampler(seed=5, method="affine")
    a1, a2 = s.sample(640), s.sample(640)
    assert not np.array_equal(a1, a2)
    assert np.array_equal(t.sample(640, batch_size=64), a1) and np.array_equal(t.sample(640, batch_size=128), a2)
    assert s.sample(0).shape == (0, c.num_measurements) and s.sample(0, bit_packed=True).shape == (0, (c.num_measurements + 7) // 8)
