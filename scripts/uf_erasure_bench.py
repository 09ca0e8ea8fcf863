"""Herald-blind against herald-aware union-find decoding inside ``count()``, one MI355X.

    python scripts/uf_erasure_bench.py                                  # d = 5, d = 9 and the largest d <= 15 that compiles
    python scripts/uf_erasure_bench.py --circuits d5 --shots 200000

The circuit is the rotated surface code memory, rounds = d, ``after_clifford_depolarization = before_measure_flip_probability
= --p`` and ``after_clifford_heralded_erasure = --pe``: a ``HERALDED_ERASE`` on the targets of every CX layer, each herald in a
detector of its own.  Per leg the ``method="faults"`` sampler counts ``--shots`` shots per call (a tenth of them beyond d = 9,
where a row is kilobytes) with ``decoder=UnionFindDecoder.from_circuit(circuit, heralds=False)`` and with ``heralds=True``,
alternating, each warmed up first, a fresh sampler of seed 1 per call so that both decoders count the same rows; the time is a
host clock around a call that ends in a device synchronise, median of ``--reps``.  Reported: shots/s of sampling and decoding
together, decoded errors, misses, and from ``tsim_uf_info`` of a handle of its own after ``--info-rows`` rows of a sampler of
seed 3 the most growth rounds and the rows decoded in LDS.  A decoder that cannot be built or whose handle is refused is
reported with the refusal and left out of the leg; the last leg starts at d = 15 and steps down by 2 until the circuit, its
sampler and the herald-aware decoder all compile, and says what stopped the larger ones.  The table and the JSON lines go to
``--out`` (default ``profiles/uf_erasure_bench.txt``) and to stdout.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tsim_amd import _lib, circuits  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402
from tsim_amd.decode import UnionFindDecoder  # noqa: E402

from uf_bench import device_info  # noqa: E402


def build(d: int, args):
    """``(circuit, {name: decoder}, {stage: refusal})`` of one distance; the circuit is ``None`` when it or its sampler does
    not compile."""
    refused, decoders = {}, {}
    t0 = time.perf_counter()
    try:
        c = CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=args.p,
                                                                 before_measure_flip_probability=args.p,
                                                                 after_clifford_heralded_erasure=args.pe))
        hp = c.compile_detector_sampler(seed=1, noise="device", method="faults")._hip()
    except Exception as e:  # noqa: BLE001 (whatever stops the sampler path is what the leg reports)
        return None, {}, {"sampler": f"{type(e).__name__}: {e}"}
    for name, heralds in (("blind", False), ("aware", True)):
        try:
            uf = UnionFindDecoder.from_circuit(c, heralds=heralds)
            hp.uf_destroy(hp.uf_create(uf.graph, uf.num_detectors + uf.num_observables))
            decoders[name] = uf
        except Exception as e:  # noqa: BLE001
            refused[name] = f"{type(e).__name__}: {e}"
    refused["compile_s"] = round(time.perf_counter() - t0, 1)
    return c, decoders, refused


def leg(name: str, c, decoders: dict, refused: dict, args) -> dict:
    d = int(name[1:])
    shots = args.shots if d <= 9 else max(1, args.shots // 10)
    batch = min(shots, 10**6 if d <= 9 else 10**5)

    def sampler():  # a fresh one per call: every call counts the same seeded rows
        return c.compile_detector_sampler(seed=1, noise="device", method="faults")

    times, last = {m: [] for m in decoders}, {}
    for m, uf in decoders.items():
        sampler().count(shots, batch_size=batch, decoder=uf)  # warm-up at the timed size
    for _ in range(args.reps):
        for m, uf in decoders.items():
            s = sampler()
            t0 = time.perf_counter()
            last[m] = s.count(shots, batch_size=batch, decoder=uf)
            times[m].append(time.perf_counter() - t0)
    if len({r.kept_with_observable_flip for r in last.values()}) != 1:
        sys.exit("uf_erasure_bench: the two decoders did not see the same rows")
    hp = s._hip()
    info = {m: device_info(hp, c.compile_detector_sampler(seed=3, noise="device", method="faults"), uf, args.info_rows)
            for m, uf in decoders.items()}
    rate = {m: shots / statistics.median(t) for m, t in times.items()}
    return dict(case=name, p=args.p, pe=args.pe, shots=shots, batch=batch, reps=args.reps, refused=refused,
                graph={m: uf.info() for m, uf in decoders.items()}, num_detectors=next(iter(decoders.values())).num_detectors,
                median_s={m: statistics.median(t) for m, t in times.items()}, min_s={m: min(t) for m, t in times.items()},
                max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate,
                aware_over_blind=rate["aware"] / rate["blind"] if len(rate) == 2 else None,
                raw_flips=next(iter(last.values())).kept_with_observable_flip, decoded_errors={m: last[m].decoded_errors for m in decoders},
                misses={m: last[m].decoder_misses for m in decoders}, info_rows=args.info_rows,
                max_rounds={m: info[m]["max_rounds"] for m in decoders}, rows_decoded={m: info[m]["rows_decoded"] for m in decoders},
                lds_bytes_per_shot={m: info[m]["lds_bytes_per_shot"] for m in decoders},
                shots_per_block={m: info[m]["shots_per_block"] for m in decoders})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=2 * 10**6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--pe", type=float, default=1e-2)
    ap.add_argument("--circuits", default="d5,d9,largest", help="dN, or `largest`: the largest d <= 15 that compiles")
    ap.add_argument("--info-rows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uf_erasure_bench.txt"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("uf_erasure_bench: no HIP device - nothing is measured without one")
    results, stopped = [], {}
    for name in args.circuits.split(","):
        tries = [15, 13, 11] if name == "largest" else [int(name[1:])]
        for d in tries:
            c, decoders, refused = build(d, args)
            if c is not None and "aware" in decoders:
                results.append(leg(f"d{d}", c, decoders, refused, args))
                print(json.dumps(results[-1]), flush=True)
                break
            stopped[f"d{d}"] = refused
            print(json.dumps({"case": f"d{d}", "stopped": refused}), flush=True)
    lines = [f"# scripts/uf_erasure_bench.py --shots {args.shots} --reps {args.reps} --p {args.p} --pe {args.pe} --circuits {args.circuits}"
             "   (one MI355X)",
             "# blind: UnionFindDecoder.from_circuit(c, heralds=False); aware: heralds=True; the same seeded rows, calls alternating,",
             "# median [min .. max] of the calls; most rounds / rows decoded: tsim_uf_info after --info-rows rows of another seed.",
             "#",
             "# d    decoder  nodes   edges   heralds  shots     seconds per call (median [min .. max])   shots/s     decoded errors  misses"
             "  most rounds  rows decoded in LDS  LDS B/shot"]
    for r in results:
        for m in r["graph"]:
            g = r["graph"][m]
            lines.append(f"  {r['case']:<4} {m:<8} {g['n_nodes']:<7} {g['n_edges']:<7} {g['n_heralds']:<8} {r['shots']:<9} "
                         f"{r['median_s'][m]:.4f} [{r['min_s'][m]:.4f} .. {r['max_s'][m]:.4f}]               {r['shots_per_s'][m]:.3e}   "
                         f"{r['decoded_errors'][m]:<15} {r['misses'][m]:<7} {r['max_rounds'][m]:<12} "
                         f"{r['rows_decoded'][m]} of {r['info_rows']:<10} {r['lds_bytes_per_shot'][m]}")
        for m, why in r["refused"].items():
            if m != "compile_s":
                lines.append(f"#      {r['case']} {m}: refused: {why}")
        lines.append(f"#      {r['case']}: {r['num_detectors']} detector columns, raw observable flips {r['raw_flips']}, aware / blind rate "
                     f"{r['aware_over_blind']}, host compile {r['refused']['compile_s']} s")
    for name, why in stopped.items():
        lines.append(f"#      {name} did not run: {why}")
    lines += ["#", "# The JSON lines:"] + [json.dumps(r) for r in results]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:len(lines) - len(results) - 2]))


if __name__ == "__main__":
    main()
