"""count(pair_columns="all") against the route without it (sample(bit_packed=True), then a numpy X^T X on the host), what
the pair counts add to a plain count(), and the pair kernels (tsim_pairs_*) on their own.

    python scripts/pairs_bench.py compare --distance 11 --shots 1000000 [--reps 3]
    python scripts/pairs_bench.py kernel --k 1321 [--rows 1000000] [--reps 5]

compare: a rotated_surface_code_memory(d, d) detector sampler with noise="device"; every call is timed to its
completion after one warm-up call of each kind, best of --reps.  The host route is the fastest numpy form of the
product: the packed rows are unpacked block by block and multiplied in float32 (sums of 0/1 products below 2^24 per
block are exact), the blocks added up in int64.  The two results are compared before anything is printed.

kernel: random rows of k columns (2 % of the bits set), resident in HBM, all k columns selected; one add + read per rep.
Run it under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times; the JSON line carries the operation counts
the rates are computed from (AND-popcount operations on 32-bit words: k (k + 1) / 2 pairs x rows / 32; the vector peak
is 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12 lane-operations/s, two per word operation).  One JSON line per case.

One case per process: run each under its own ``timeout`` and chain them with ``&&``, so that the first failure ends the
series (results: DESIGN.md 3.12, profiles/r07/pair_counts.txt).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tsim_amd import backend, circuits, synth  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def timed(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def host_product(packed: np.ndarray, n_cols: int, block: int = 1 << 15) -> np.ndarray:
    out = np.zeros((n_cols, n_cols), np.int64)
    for lo in range(0, len(packed), block):
        B = np.unpackbits(packed[lo:lo + block], axis=1, count=n_cols, bitorder="little").astype(np.float32)
        out += (B.T @ B).astype(np.int64)
    return out


def compare(args) -> None:
    d, shots = args.distance, args.shots
    c = CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=1e-3,
                                                             before_measure_flip_probability=1e-3))

    def mk(seed=1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return c.compile_detector_sampler(seed=seed, noise="device")

    s = mk()
    n_cols = int(s._program.num_outputs)

    def route(sampler):
        return host_product(sampler.sample(shots, bit_packed=True, append_observables=True), n_cols)

    # the two routes give the same matrix for the same seed
    got = mk(7).count(shots, pair_columns="all")
    if not np.array_equal(got.pair_counts, route(mk(7))):
        raise SystemExit("count(pair_columns='all') and the host product differ")
    warm = min(shots, 1 << 20)
    s.count(warm)
    s.count(warm, pair_columns="all")
    t_pairs = min(timed(lambda: s.count(shots, pair_columns="all")) for _ in range(args.reps))
    t_plain = min(timed(lambda: s.count(shots)) for _ in range(args.reps))
    t_sample = min(timed(lambda: s.sample(shots, bit_packed=True, append_observables=True)) for _ in range(args.reps))
    t_route = min(timed(lambda: route(s)) for _ in range(args.host_reps))
    print(json.dumps(dict(case=f"surface_d{d}", shots=shots, columns=n_cols, count_pairs_s=t_pairs, count_plain_s=t_plain,
                          pairs_add_s=t_pairs - t_plain, sample_bit_packed_s=t_sample, sample_and_host_product_s=t_route,
                          speedup_over_host_route=t_route / t_pairs, reps=args.reps, host_reps=args.host_reps)), flush=True)


def kernel(args) -> None:
    k, n = args.k, args.rows
    row_bytes = (k + 63) // 64 * 8
    hp = backend.HipProgram(synth.kat_h_m(), device=0)
    rng = np.random.default_rng(1)
    d_rows = hp.malloc(n * row_bytes)
    block = np.packbits(rng.random((1 << 14, row_bytes * 8)) < 0.02, axis=1, bitorder="little")
    for r0 in range(0, n, len(block)):
        hp.h2d(d_rows.ptr + r0 * row_bytes, block[: min(len(block), n - r0)])
    h = hp.pairs_create(k, np.arange(k))

    def run():
        hp.pairs_add_device(h, d_rows.ptr, n, row_bytes)
        hp.synchronize()

    run()
    ts = sorted(timed(run) for _ in range(args.reps))
    t = ts[len(ts) // 2]
    got = hp.pairs_read(h, k)
    reps_done = args.reps + 1
    whole, part = divmod(n, len(block))
    want = host_product(block, k) * whole + host_product(block[:part], k)
    if not np.array_equal(got, want * reps_done):
        raise SystemExit("the pair kernels and the host product differ")
    word_ops = k * (k + 1) // 2 * (n / 32)
    print(json.dumps(dict(case=f"pair_kernels_k{k}", rows=n, k=k, row_bytes=row_bytes, add_call_s=t, word_ops=word_ops,
                          word_ops_per_s_of_call=word_ops / t, valu_peak_word_ops_per_s=VALU_LANE_OPS_PER_S / 2,
                          fraction_of_valu_peak_of_call=2 * word_ops / t / VALU_LANE_OPS_PER_S, add_calls=reps_done)), flush=True)
    hp.pairs_destroy(h)
    d_rows.free()


def main() -> None:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    a = sub.add_parser("compare")
    a.add_argument("--distance", type=int, default=5)
    a.add_argument("--shots", type=int, default=1_000_000)
    a.add_argument("--reps", type=int, default=3)
    a.add_argument("--host-reps", type=int, default=3)
    b = sub.add_parser("kernel")
    b.add_argument("--k", type=int, default=121)
    b.add_argument("--rows", type=int, default=1_000_000)
    b.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    (compare if args.mode == "compare" else kernel)(args)


if __name__ == "__main__":
    main()
