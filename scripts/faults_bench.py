"""The fault-driven detector sampler next to the Pauli-frame and the default one: surface code memory,
rounds = d, one MI355X.

    python scripts/faults_bench.py                            # the table: the three methods per distance, JSON lines
    python scripts/faults_bench.py --profile --circuits d15   # a few requests of the faults method and nothing else, for
                                                              # rocprofv3 --kernel-trace --stats -- python scripts/faults_bench.py --profile ...

Per distance: the time to build each sampler from the circuit text (parse, compile, sampler object, first 2^14-shot request -
the device handle is created there), then ``count()`` of ``--shots`` shots per call in batches of 10^6: rows, tally and
counters never leave the device, the time is a host clock around a call that returns the counters (it ends in a device
synchronise).  The methods alternate, each is warmed up first; the median and the spread of ``--reps`` calls are reported.
The default method is skipped above ``--default-up-to`` (its build is quadratic in the circuit and worse).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tsim_amd import _lib, circuits  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402


def memory(d: int, p: float) -> str:
    return circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=p, before_measure_flip_probability=p)


def build(text: str, method: str):
    """``(sampler, seconds)``: from the circuit text to a sampler that has answered a first request."""
    t0 = time.perf_counter()
    c = CliffordCircuit(text)
    s = c.compile_detector_sampler(seed=1, noise="device", method=method)
    s.count(1 << 14)
    return s, time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10**7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--circuits", default="d3,d5,d7,d11,d15")
    ap.add_argument("--default-up-to", type=int, default=11)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("faults_bench: no HIP device - nothing is measured without one")
    for name in args.circuits.split(","):
        d = int(name[1:])
        text = memory(d, args.p)
        samplers, build_s = {}, {}
        samplers["faults"], build_s["faults"] = build(text, "faults")
        form = samplers["faults"]._form
        info = samplers["faults"]._frame_handle().info()
        shape = dict(case=name, p=args.p, outputs=form.n_out, num_e=form.num_e, noise_sites=form.n_sites, classes=form.n_classes,
                     flips=len(form.cols), gap_rows=len(form.gap_thr), row_words=info["row_words"], waves=info["waves"],
                     lds_bytes=info["lds_bytes"], tables_in_lds=info["tables_in_lds"], windows=info["n_windows"])
        if args.profile:
            for _ in range(3):
                samplers["faults"].count(args.shots, batch_size=10**6)
            print(json.dumps(dict(shape, profile="faults", shots=args.shots, requests=3)), flush=True)
            continue
        samplers["frame"], build_s["frame"] = build(text, "frame")
        if d <= args.default_up_to:
            samplers["autoregressive"], build_s["autoregressive"] = build(text, "autoregressive")
        times = {m: [] for m in samplers}
        for m, s in samplers.items():
            s.count(args.shots, batch_size=10**6)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, s in samplers.items():
                t0 = time.perf_counter()
                got = s.count(args.shots, batch_size=10**6)
                times[m].append(time.perf_counter() - t0)
                assert got.shots == args.shots
        rate = {m: args.shots / statistics.median(times[m]) for m in samplers}
        print(json.dumps(dict(
            shape, build_s=build_s, shots=args.shots, reps=args.reps, median_s={m: statistics.median(t) for m, t in times.items()},
            min_s={m: min(t) for m, t in times.items()}, max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate,
            faults_over_frame=rate["faults"] / rate["frame"],
            faults_over_default=(rate["faults"] / rate["autoregressive"]) if "autoregressive" in rate else None,
            detection_fraction={m: float(s.count(1 << 16).column_counts[:form.num_detectors].mean() / (1 << 16))
                                for m, s in samplers.items()})), flush=True)


if __name__ == "__main__":
    main()
