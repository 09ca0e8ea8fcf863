"""Fixed-weight fault sampling next to the unconditioned fault sampler, and the stratified logical error rate next to direct
sampling: surface code memory, rounds = d, one MI355X.

    python scripts/fixed_weight_bench.py            # writes profiles/fixed_weight_bench.txt (--out), JSON lines on stdout

Rates: per distance ``count()`` of ``--shots`` shots per call in batches of 10^6 at ``fault_weight`` 1, 4 and 16 and of the
unconditioned ``method="faults"`` sampler on the same circuit at ``--p``: rows, tally and counters never leave the device, the
time is a host clock around a call that returns the counters (it ends in a device synchronise).  The samplers alternate, each
is warmed up first; the median and the spread of ``--reps`` calls are reported.
Estimates: at ``--p-low`` the stratified rate of the unweighted union-find decoder (``--strata-shots`` per weight 0 ..
``--kmax``) next to ``count(decoder=...)`` of ``--direct-shots`` directly sampled shots, with the time each took.
"""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tsim_amd import _lib, circuits  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402
from tsim_amd.decode import UnionFindDecoder  # noqa: E402
from tsim_amd.fixed_weight import stratified_error_rate, weight_law  # noqa: E402

WEIGHTS = (1, 4, 16)


def memory(d: int, p: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=p, before_measure_flip_probability=p))


def rates(d: int, args) -> dict:
    c = memory(d, args.p)
    samplers = {"faults": c.compile_detector_sampler(seed=1, method="faults")}
    for k in WEIGHTS:
        samplers[f"k={k}"] = c.compile_detector_sampler(seed=1, method="faults", fault_weight=k)
    for s in samplers.values():
        s.count(args.shots, batch_size=10**6)  # warm-up at the timed size
    times = {m: [] for m in samplers}
    for _ in range(args.reps):
        for m, s in samplers.items():
            t0 = time.perf_counter()
            got = s.count(args.shots, batch_size=10**6)
            times[m].append(time.perf_counter() - t0)
            assert got.shots == args.shots
    form = c.compile_faults()
    info = samplers["k=16"]._frame_handle().weight_info()
    law, tail = weight_law(form, 32)
    return dict(kind="rate", d=d, p=args.p, outputs=form.n_out, noise_sites=form.n_sites, classes=form.n_classes,
                mean_weight=float(sum(k * v for k, v in enumerate(law))), weight_beyond_32=tail, waves=info["waves"],
                lds_bytes=info["lds_bytes"], row_words=info["row_words"], tables_in_lds=info["tables_in_lds"], shots=args.shots,
                reps=args.reps, median_s={m: statistics.median(t) for m, t in times.items()}, min_s={m: min(t) for m, t in times.items()},
                max_s={m: max(t) for m, t in times.items()}, shots_per_s={m: args.shots / statistics.median(t) for m, t in times.items()})


def estimates(d: int, args) -> dict:
    c = memory(d, args.p_low)
    uf = UnionFindDecoder.from_circuit(c)
    stratified_error_rate(c, uf, 1 << 14, kmax=args.kmax, seed=2)  # warm-up: handles, decoder tables
    c.compile_detector_sampler(seed=2, method="faults").count(1 << 14, decoder=uf)
    t0 = time.perf_counter()
    got = stratified_error_rate(c, uf, args.strata_shots, kmax=args.kmax, seed=3)
    t_strat = time.perf_counter() - t0
    t0 = time.perf_counter()
    direct = c.compile_detector_sampler(seed=4, method="faults").count(args.direct_shots, decoder=uf, batch_size=10**6)
    t_direct = time.perf_counter() - t0
    p = direct.decoded_errors / args.direct_shots
    return dict(kind="estimate", d=d, p=args.p_low, noise_sites=c.compile_faults().n_sites, kmax=args.kmax, strata_shots=args.strata_shots,
                law=got.law.tolist(), f=got.f.tolist(), decoded_errors=got.decoded_errors.tolist(), decoder_misses=got.decoder_misses.tolist(),
                estimate=got.estimate, std_error=got.std_error, tail=got.tail, stratified_s=t_strat, direct_shots=args.direct_shots,
                direct_errors=direct.decoded_errors, direct_rate=p, direct_std_error=math.sqrt(max(p * (1 - p), 0.0) / args.direct_shots),
                direct_s=t_direct)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10**7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--circuits", default="d5,d9,d15")
    ap.add_argument("--p-low", type=float, default=1e-4)
    ap.add_argument("--low-circuits", default="d5,d9")
    ap.add_argument("--kmax", type=int, default=8)
    ap.add_argument("--strata-shots", type=int, default=10**6)
    ap.add_argument("--direct-shots", type=int, default=10**7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fixed_weight_bench.txt"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("fixed_weight_bench: no HIP device - nothing is measured without one")
    rows = [rates(int(n[1:]), args) for n in args.circuits.split(",") if n]
    for r in rows:
        print(json.dumps(r), flush=True)
    ests = [estimates(int(n[1:]), args) for n in args.low_circuits.split(",") if n]
    for r in ests:
        print(json.dumps(r), flush=True)
    names = ["faults"] + [f"k={k}" for k in WEIGHTS]
    ms = lambda v: f"{1e3 * v:.2f}"  # noqa: E731
    lines = [
        "Fixed-weight fault sampling next to the unconditioned fault sampler (scripts/fixed_weight_bench.py; DESIGN.md 3.18)",
        "one MI355X, one session, the samplers alternating; rotated surface code memory, rounds = d,",
        f"after_clifford_depolarization = before_measure_flip_probability = {args.p:g}",
        f"rate: count() of {args.shots:.0e} shots in batches of 10^6 (host clock around the call, warm-up at that size, median of {args.reps})",
        "",
        "| d | outputs | sites | mean weight | P(K > 32) | S (words per row) | waves per block | LDS per block | count() faults | "
        + " | ".join(f"count() fault_weight={k}" for k in WEIGHTS) + " |",
        "|" + "---|" * (9 + len(WEIGHTS)),
    ]
    for r in rows:
        lines.append(f"| {r['d']} | {r['outputs']} | {r['noise_sites']} | {r['mean_weight']:.2f} | {r['weight_beyond_32']:.2e} | {r['row_words']} | "
                     f"{r['waves']} | {r['lds_bytes'] / 1024:.1f} KiB | " + " | ".join(f"{r['shots_per_s'][m]:.2e} /s" for m in names) + " |")
    lines += ["", f"spread of the {args.reps} calls (min .. max):"]
    for r in rows:
        lines.append(f"d = {r['d']}: " + ", ".join(f"{m} {ms(r['min_s'][m])} .. {ms(r['max_s'][m])} ms (median {ms(r['median_s'][m])})" for m in names))
    lines += ["", f"stratified estimate next to direct sampling, unweighted union-find decoder, p = {args.p_low:g}, weights 0 .. {args.kmax}, "
              f"{args.strata_shots:.0e} shots per weight, {args.direct_shots:.0e} direct shots (host clock, one call each, after a warm-up)", "",
              "| d | sites | stratified estimate | std error | tail P(K > kmax) | time | direct rate | std error | wrong shots | time |", "|" + "---|" * 10]
    for r in ests:
        lines.append(f"| {r['d']} | {r['noise_sites']} | {r['estimate']:.3e} | {r['std_error']:.1e} | {r['tail']:.1e} | {r['stratified_s']:.2f} s | "
                     f"{r['direct_rate']:.3e} | {r['direct_std_error']:.1e} | {r['direct_errors']} | {r['direct_s']:.2f} s |")
    lines += [""]
    for r in ests:
        lines.append(f"d = {r['d']}: P(K = k) = " + ", ".join(f"{v:.3e}" for v in r["law"]))
        lines.append(f"d = {r['d']}: f_k = " + ", ".join(f"{v:.3e}" for v in r["f"]) + f"; decoder misses {sum(r['decoder_misses'])}")
    lines += ["", "the script's output:"] + [json.dumps(r) for r in rows + ests]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
