"""The Pauli-frame detector sampler next to the default one: surface code memory, rounds = d, one MI355X.

    python scripts/frame_bench.py                            # the table: both methods per distance, JSON lines
    python scripts/frame_bench.py --profile --circuits d11   # a few requests of the frame method and nothing else, for
                                                             # rocprofv3 --kernel-trace --stats -- python scripts/frame_bench.py --profile ...

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
        sys.exit("frame_bench: no HIP device - nothing is measured without one")
    for name in args.circuits.split(","):
        d = int(name[1:])
        text = memory(d, args.p)
        samplers, build_s = {}, {}
        samplers["frame"], build_s["frame"] = build(text, "frame")
        form = samplers["frame"]._form
        info = samplers["frame"]._frame_handle().info()
        shape = dict(case=name, p=args.p, qubits=form.n_qubits, records=form.n_records, outputs=form.n_out, num_e=form.num_e,
                     frame_operations=form.n_ops, batches=form.n_batches, noise_sites=len(form.site_chan), T=info["T"],
                     frame_lds_bytes=info["lds_bytes"], words_per_launch=info["max_words"], out_windows=info["n_windows"])
        if args.profile:
            for _ in range(3):
                samplers["frame"].count(args.shots, batch_size=10**6)
            print(json.dumps(dict(shape, profile="frame", shots=args.shots, requests=3)), flush=True)
            continue
        if d <= args.default_up_to:
            samplers["default"], build_s["default"] = build(text, "autoregressive")
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
            frame_over_default=(rate["frame"] / rate["default"]) if "default" in rate else None,
            detection_fraction={m: float(s.count(1 << 16).column_counts[:form.num_detectors].mean() / (1 << 16))
                                for m, s in samplers.items()})), flush=True)


if __name__ == "__main__":
    main()
