"""The row table (tsim_rowtab_add_device) on resident rows against k_tally on the same buffers, and what
count(pattern_columns="all") adds to a plain count().

    python scripts/patterns_bench.py kernel --case d5_p1e-3|d5_p2e-2|random64|wide9241 [--reps 5]
    python scripts/patterns_bench.py count --distance 5 --shots 10000000 [--reps 3]

kernel: rows resident in HBM; one tsim_rowtab_add_device per rep into an EMPTY table (reset before each rep, outside the
clock: every pattern is claimed again, the worst case of an add) and one more into the filled table (the steady state of
a count() of many batches); tsim_tally_rows_device (kept rows and column counts, no histogram) on the same buffer.  Bytes
are n x row_bytes; the table's entries are compared with np.unique before anything is printed.
  d5_p1e-3 / d5_p2e-2  2^22 detector + observable rows of rotated_surface_code_memory(5, 5) (121 columns, 16 bytes) at that
                       noise: one pattern dominates / thousands of patterns
  random64             2^22 rows of 64 uniformly random columns drawn from 2^20 distinct values
  wide9241             2^16 rows of 9241 columns (the d = 21 width of DESIGN.md 3.10), 1 % of the bits set, 4096 distinct rows

count: a rotated_surface_code_memory(d, d) detector sampler at p = 1e-3 with noise="device"; count(shots,
pattern_columns="all") against count(shots), best of --reps after one warm-up call of each.

One case per process: run each under its own ``timeout`` and chain them with ``&&`` (results: DESIGN.md 3.13,
profiles/r07/pattern_counts.txt).  One JSON line per case.
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
from tsim_amd.counts import counters_length  # noqa: E402


def timed(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def median(ts):
    return sorted(ts)[len(ts) // 2]


def surface_sampler(d, p, seed=1):
    c = CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=p, before_measure_flip_probability=p))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return c.compile_detector_sampler(seed=seed, noise="device")


def case_rows(case: str):
    """(packed rows uint8[n, row_bytes], n_cols)"""
    rng = np.random.default_rng(1)
    if case.startswith("d5_p"):
        s = surface_sampler(5, float(case[4:]))
        return np.ascontiguousarray(s.sample(1 << 22, bit_packed=True, append_observables=True)), int(s._program.num_outputs)
    if case == "random64":
        values = rng.integers(0, 1 << 63, 1 << 20, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 1 << 20, dtype=np.uint64)
        return values[rng.integers(0, 1 << 20, 1 << 22)].view(np.uint8).reshape(1 << 22, 8), 64
    if case == "wide9241":
        n_cols = 9241
        pool = np.packbits(rng.random((4096, n_cols), dtype=np.float32) < 0.01, axis=1, bitorder="little")
        return np.ascontiguousarray(pool[rng.integers(0, 4096, 1 << 16)]), n_cols
    raise SystemExit(f"unknown case {case!r}")


def kernel(args) -> None:
    rows, n_cols = case_rows(args.case)
    n, row_bytes = rows.shape
    hp = backend.HipProgram(synth.kat_h_m(), device=0)
    d_rows = hp.malloc(rows.nbytes)
    hp.h2d(d_rows, rows)
    uniq, cnt = np.unique(rows.view(np.dtype((np.void, row_bytes))).reshape(n), return_counts=True)
    capacity = max(1 << 16, 4 * len(uniq))
    h = hp.rowtab_create(n_cols, np.arange(n_cols), capacity)
    d_counts = hp.malloc(8 * counters_length(n_cols, 0))
    hp.h2d(d_counts, np.zeros(counters_length(n_cols, 0), np.uint64))

    def add():
        hp.rowtab_add_device(h, d_rows.ptr, n, row_bytes)
        hp.synchronize()

    def tally():
        hp.tally_rows_device(d_rows.ptr, n, row_bytes, n_cols, d_counts.ptr)
        hp.synchronize()

    add()
    keys, counts, info = hp.rowtab_read(h, n_cols)
    got = {k.tobytes(): int(c) for k, c in zip(keys, counts)}
    kb = (n_cols + 7) // 8
    want = {}
    for u, c in zip(uniq, cnt):  # (pad bits of the last byte are not part of a pattern)
        key = bytearray(u.tobytes()[:kb])
        if n_cols % 8:
            key[-1] &= (1 << (n_cols % 8)) - 1
        want[bytes(key)] = want.get(bytes(key), 0) + int(c)
    if got != want or info[4] or info[5]:
        raise SystemExit(f"the row table and np.unique differ (info {info.tolist()})")
    t_filled = median([timed(add) for _ in range(args.reps)])
    t_empty = []
    for _ in range(args.reps):
        hp.rowtab_reset(h)
        hp.synchronize()
        t_empty.append(timed(add))
    t_empty = median(t_empty)
    tally()
    t_tally = median([timed(tally) for _ in range(args.reps)])
    nbytes = n * row_bytes
    print(json.dumps(dict(case=args.case, rows=n, columns=n_cols, row_bytes=row_bytes, distinct=len(want),
                          top_pattern_share=max(want.values()) / n, capacity=int(info[0]), launches_per_add=1 if n_cols <= 63 else 2,
                          add_into_empty_s=t_empty, add_into_filled_s=t_filled, tally_s=t_tally,
                          add_into_empty_bytes_per_s=nbytes / t_empty, add_into_filled_bytes_per_s=nbytes / t_filled,
                          tally_bytes_per_s=nbytes / t_tally, empty_over_tally=t_empty / t_tally, filled_over_tally=t_filled / t_tally,
                          reps=args.reps)), flush=True)
    hp.rowtab_destroy(h)
    d_rows.free()
    d_counts.free()


def count(args) -> None:
    s = surface_sampler(args.distance, 1e-3)
    warm = min(args.shots, 1 << 20)
    s.count(warm)
    s.count(warm, pattern_columns="all")
    t_pat = min(timed(lambda: s.count(args.shots, pattern_columns="all")) for _ in range(args.reps))
    t_plain = min(timed(lambda: s.count(args.shots)) for _ in range(args.reps))
    got = s.count(args.shots, pattern_columns="all")
    print(json.dumps(dict(case=f"count_surface_d{args.distance}", shots=args.shots, columns=int(s._program.num_outputs),
                          distinct=len(got.patterns), overflow=got.pattern_overflow, count_patterns_s=t_pat, count_plain_s=t_plain,
                          patterns_over_plain=t_pat / t_plain, shots_per_s_with_patterns=args.shots / t_pat, reps=args.reps)), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    a = sub.add_parser("kernel")
    a.add_argument("--case", required=True)
    a.add_argument("--reps", type=int, default=5)
    b = sub.add_parser("count")
    b.add_argument("--distance", type=int, default=5)
    b.add_argument("--shots", type=int, default=10_000_000)
    b.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    (kernel if args.mode == "kernel" else count)(args)


if __name__ == "__main__":
    main()
