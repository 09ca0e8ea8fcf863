"""Throughput of count() against sample(bit_packed=True), and of the tally kernel (tsim_tally_rows_device) on its own.

Samplers (noise="device"): synth.config_program("C2") and rotated_surface_code_memory(d, d) for d = 5 and 11; each
call is timed to its completion, after one warm-up call of each kind; shots/s of both and their ratio.  Kernel: random
rows of the d = 21 surface code's width (detectors + observables, padded to uint64 words as the samplers hold them, a
few percent of bits set), resident in HBM; bytes/s = rows x row bytes / time of one tally call to completion (median of
--reps).  One JSON line per case.

    python scripts/counts_bench.py [--shots 100000000] [--surface-shots 10000000] [--rows 2000000] [--reps 5]
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
from tsim_amd.channels import error_probs  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402
from tsim_amd.counts import counters_length  # noqa: E402
from tsim_amd.sampler import CompiledDetectorSampler  # noqa: E402


def timed(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def bench_sampler(name: str, s, shots: int, reps: int) -> None:
    s.count(min(shots, 1 << 22))
    s.sample(min(shots, 1 << 22), bit_packed=True)
    t_count = min(timed(lambda: s.count(shots)) for _ in range(reps))
    t_sample = min(timed(lambda: s.sample(shots, bit_packed=True)) for _ in range(reps))
    print(json.dumps(dict(case=name, shots=shots, outputs=int(s._program.num_outputs), count_shots_per_s=shots / t_count,
                          sample_bit_packed_shots_per_s=shots / t_sample, speedup=t_sample / t_count,
                          count_s=t_count, sample_s=t_sample)), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=100_000_000)
    ap.add_argument("--surface-shots", type=int, default=10_000_000)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-samplers", action="store_true")
    args = ap.parse_args()

    if not args.skip_samplers:
        prog, cfg = synth.config_program("C2")
        nf = cfg["num_f"]
        s = CompiledDetectorSampler(prog, channel_probs=[error_probs(0.03)] * nf, error_transform=np.eye(nf, dtype=np.uint8),
                                    seed=1, noise="device")
        bench_sampler("C2", s, args.shots, args.reps)
        for d in (5, 11):
            c = CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=1e-3,
                                                                     before_measure_flip_probability=1e-3))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                s = c.compile_detector_sampler(seed=1, noise="device")
            bench_sampler(f"surface_d{d}", s, args.surface_shots, args.reps)

    # the kernel alone on resident rows of the d = 21 width
    conv = CliffordCircuit(circuits.rotated_surface_code_memory(21, 21)).compile_m2d_converter()
    n_cols = conv.num_detectors + conv.num_observables
    nd = conv.num_detectors
    row_bytes = (n_cols + 63) // 64 * 8
    hp = backend.HipProgram(synth.kat_h_m(), device=0)
    B = args.rows
    rng = np.random.default_rng(1)
    d_rows = hp.malloc(B * row_bytes)
    d_c = hp.malloc(8 * counters_length(n_cols, 0))
    d_test = hp.malloc(row_bytes)
    block = np.packbits(rng.random((1 << 14, row_bytes * 8)) < 0.02, axis=1, bitorder="little")
    for r0 in range(0, B, len(block)):
        hp.h2d(d_rows.ptr + r0 * row_bytes, block[: min(len(block), B - r0)])
    test = np.zeros(row_bytes * 8, np.uint8)
    test[: nd // 2] = 1  # half the detectors post-selected
    hp.h2d(d_test, np.packbits(test, bitorder="little"))
    hp.h2d(d_c, np.zeros(counters_length(n_cols, 0), np.uint64))
    for label, dt in (("no_mask", 0), ("half_detectors_masked", d_test.ptr)):
        def run():
            hp.tally_rows_device(d_rows.ptr, B, row_bytes, n_cols, d_c.ptr, d_test=dt, observables=(nd, n_cols))
            hp.synchronize()

        run()
        ts = sorted(timed(run) for _ in range(args.reps))
        t = ts[len(ts) // 2]
        print(json.dumps(dict(case=f"tally_kernel_d21_{label}", rows=B, n_cols=n_cols, row_bytes=row_bytes, seconds=t,
                              rows_per_s=B / t, bytes_per_s=B * row_bytes / t)), flush=True)
    for buf in (d_rows, d_c, d_test):
        buf.free()


if __name__ == "__main__":
    main()
