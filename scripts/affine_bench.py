"""Affine measurement sampler next to the autoregressive one: rows resident in HBM, one MI355X.

    python scripts/affine_bench.py                       # the table: both methods per circuit, JSON lines
    python scripts/affine_bench.py --profile affine      # a few requests of one method and nothing else, for
                                                         # rocprofv3 --kernel-trace --stats -- python scripts/affine_bench.py --profile affine

Both samplers run with ``noise="device"`` and hand their rows to a sink that does nothing: error bits, records and random
numbers never leave the device, and the time is a host clock around a call that ends in a stream synchronise.  The methods
alternate, each is warmed up first, the median and the spread of ``--reps`` calls are reported.  Where the autoregressive
method would take more than ``--budget`` seconds for the request (a warm-up at 2^14 shots says so) it is timed at fewer
shots, and the line says how many.  Bytes per shot are what the affine kernel must move (the packed f row in, the padded
packed record row out), computed from the shapes.
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

HBM_PEAK = 8.0e12       # bytes/s, specification
HBM_MEASURED = 6.3e12   # bytes/s, a float4 copy


def ghz(n: int, p: float) -> str:
    return "\n".join(["H 0"] + [f"CX {i} {i + 1}" for i in range(n - 1)] +
                     [f"X_ERROR({p}) " + " ".join(map(str, range(n))), "M " + " ".join(map(str, range(n)))])


def memory(d: int, p: float) -> str:
    return circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=p, before_round_data_depolarization=p,
                                                before_measure_flip_probability=p, after_reset_flip_probability=p)


def cases(p: float) -> dict:
    return {"d3": memory(3, p), "d5": memory(5, p), "d7": memory(7, p), "ghz300": ghz(300, p)}


def nothing(*_a) -> None:
    pass


def run(sampler, method: str, shots: int) -> float:
    t0 = time.perf_counter()
    if method == "affine":
        sampler._direct_device(shots, None, sink=nothing)
    elif sampler._program.components:
        sampler._device_noise_plain(shots, None, False, sink=nothing)
    else:
        sampler._direct_device(shots, None, sink=nothing)
    sampler._hip().synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10**6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--budget", type=float, default=4.0, help="seconds one autoregressive request may take")
    ap.add_argument("--circuits", default="d3,d5,d7,ghz300")
    ap.add_argument("--profile", choices=["affine", "autoregressive"], default=None)
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("affine_bench: no HIP device - nothing is measured without one")
    texts = cases(args.p)
    for name in args.circuits.split(","):
        c = CliffordCircuit(texts[name])
        t0 = time.perf_counter()
        form = c.compile_affine_measurements()
        compile_affine = time.perf_counter() - t0
        M, num_f = len(form["flip"]), form["num_f"]
        bytes_per_shot = 8 * max(1, (num_f + 63) // 64) + 8 * ((M + 63) // 64)
        samplers = {"affine": c.compile_sampler(seed=1, method="affine", noise="device")}
        if args.profile in (None, "autoregressive"):
            t0 = time.perf_counter()
            samplers["autoregressive"] = c.compile_sampler(seed=1, noise="device")
            compile_auto = time.perf_counter() - t0
        if args.profile:
            s = samplers[args.profile]
            run(s, args.profile, 1 << 14)
            for _ in range(3):
                run(s, args.profile, args.shots)
            print(json.dumps(dict(case=name, profile=args.profile, shots=args.shots, requests=3, records=M, num_f=num_f,
                                  n_random=form["n_random"], bytes_per_shot=bytes_per_shot)), flush=True)
            continue
        shots = {}
        for m, s in samplers.items():
            run(s, m, 1 << 14)
            t = min(run(s, m, 1 << 14) for _ in range(2))
            # (a request of 2^14 shots is mostly launch overhead: this only guards against minutes-long requests)
            shots[m] = args.shots if t * args.shots / (1 << 14) <= args.budget * 8 else max(1 << 14, int(args.budget / t * (1 << 14)) // 64 * 64)
            run(s, m, shots[m])
        times = {m: [] for m in samplers}
        for _ in range(args.reps):
            for m, s in samplers.items():
                times[m].append(run(s, m, shots[m]))
        rate = {m: shots[m] / statistics.median(times[m]) for m in samplers}
        info = samplers["affine"]._affine_handle().info()
        print(json.dumps(dict(
            case=name, p=args.p, records=M, num_f=num_f, n_random=form["n_random"], list_entries=int(len(form["cols"])),
            window=info["window"], n_windows=info["n_windows"], lds_bytes_per_wave=info["lds_bytes_per_wave"],
            compile_affine_s=compile_affine, compile_autoregressive_s=compile_auto,
            shots={m: shots[m] for m in samplers},
            median_s={m: statistics.median(times[m]) for m in samplers},
            min_s={m: min(times[m]) for m in samplers}, max_s={m: max(times[m]) for m in samplers},
            shots_per_s=rate, affine_over_autoregressive=rate["affine"] / rate["autoregressive"],
            bytes_per_shot=bytes_per_shot, affine_bytes_per_s=rate["affine"] * bytes_per_shot,
            affine_share_of_8_TBs=rate["affine"] * bytes_per_shot / HBM_PEAK,
            affine_share_of_6p3_TBs=rate["affine"] * bytes_per_shot / HBM_MEASURED, reps=args.reps)), flush=True)


if __name__ == "__main__":
    main()
