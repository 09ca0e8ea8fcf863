"""The union-find decoder inside ``count()``: surface code memory, rounds = d, one MI355X.

    python scripts/uf_bench.py                       # the table: per distance, JSON lines
    python scripts/uf_bench.py --circuits d15 --shots 1000000

Per distance the ``method="faults"`` sampler counts ``--shots`` shots per call in batches of 10^6, once without a decoder and
once with ``decoder=UnionFindDecoder.from_circuit(circuit)``, alternating, each warmed up first; the time is a host clock
around a call that returns the counters (it ends in a device synchronise); the median and the spread of ``--reps`` calls are
reported, with the decoded logical error rate, the misses and what ``tsim_uf_info`` says about the kernel (LDS per shot, shots
per block, the most growth rounds a row took).  At d = 3 a ``LookupDecoder`` trained on ``--train`` shots of another seed
runs beside it: the maximum-likelihood bound at that size.  All three noise options are set to ``--p``.
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
from tsim_amd.decode import LookupDecoder, UnionFindDecoder  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10**7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--circuits", default="d3,d5,d7,d11,d15")
    ap.add_argument("--train", type=int, default=10**8)
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("uf_bench: no HIP device - nothing is measured without one")
    for name in args.circuits.split(","):
        d = int(name[1:])
        c = CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=args.p,
                                                                 before_measure_flip_probability=args.p,
                                                                 after_reset_flip_probability=args.p))
        t0 = time.perf_counter()
        uf = UnionFindDecoder.from_circuit(c)
        graph_s = time.perf_counter() - t0
        s = c.compile_detector_sampler(seed=1, noise="device", method="faults")
        runs = {"plain": {}, "union_find": dict(decoder=uf)}
        if d == 3:
            train = c.compile_detector_sampler(seed=2, noise="device", method="faults").count(args.train, pattern_columns="all")
            runs["lookup"] = dict(decoder=LookupDecoder.from_counts(train))
        times, last = {m: [] for m in runs}, {}
        for m, kw in runs.items():
            s.count(args.shots, batch_size=10**6, **kw)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, kw in runs.items():
                t0 = time.perf_counter()
                last[m] = s.count(args.shots, batch_size=10**6, **kw)
                times[m].append(time.perf_counter() - t0)
        hp = s._hip()
        h = hp.uf_create(uf.graph, uf.num_detectors + uf.num_observables)
        info = hp.uf_info(h)
        hp.uf_destroy(h)
        rate = {m: args.shots / statistics.median(t) for m, t in times.items()}
        print(json.dumps(dict(
            case=name, p=args.p, shots=args.shots, reps=args.reps, graph=uf.info(), graph_s=graph_s,
            lds_bytes_per_shot=info["lds_bytes_per_shot"], shots_per_block=info["shots_per_block"], grid_blocks=info["grid_blocks"],
            median_s={m: statistics.median(t) for m, t in times.items()}, min_s={m: min(t) for m, t in times.items()},
            max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate, union_find_over_plain=rate["union_find"] / rate["plain"],
            raw_flip_rate=last["plain"].kept_with_observable_flip / args.shots,
            logical_error_rate={m: last[m].decoded_errors / args.shots for m in runs if m != "plain"},
            misses={m: last[m].decoder_misses for m in runs if m != "plain"},
            lookup_entries=len(runs["lookup"]["decoder"]) if "lookup" in runs else None)), flush=True)


if __name__ == "__main__":
    main()
