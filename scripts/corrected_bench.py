"""What corrected observables cost inside ``count()``: surface code memory, rounds = d, one MI355X.

    python scripts/corrected_bench.py                          # d = 5, 9, 15: the table, written to profiles/corrected_bench.txt
    python scripts/corrected_bench.py --plain-only > parent.jsonl   # in a checkout of the parent commit: its corrected=False leg
    python scripts/corrected_bench.py --parent parent.jsonl    # the table with the ratio against those lines

Per distance the ``method="faults"`` sampler (all three noise options at ``--p``) counts ``--shots`` shots per call in batches of
10^6 with ``decoder=UnionFindDecoder.from_circuit(circuit)``, once as it is (``plain``) and once with ``corrected=True``, a fresh
sampler of seed 1 per call (the same rows in every call), alternating, each warmed up first; the time is a host clock around a
call that returns the counters (it ends in a device synchronise); the median and the spread of ``--reps`` calls are reported.
The run stops when the two calls disagree on ``kept``, ``decoded_errors`` or ``decoder_misses``, or when the corrected call's
``kept_with_observable_flip`` is not its ``decoded_errors``.  ``--plain-only`` times the first call alone and uses nothing newer
than ``count(decoder=...)``, so it runs on the parent commit: one run of each gives the ratio of the ``corrected=False`` leg, which
is the same code path and should show run-to-run spread only.
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


def memory(d: int, p: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=p, before_measure_flip_probability=p,
                                                                after_reset_flip_probability=p))


def measure(name: str, args) -> dict:
    c = memory(int(name[1:]), args.p)
    uf = UnionFindDecoder.from_circuit(c)
    legs = {"plain": {}} if args.plain_only else {"plain": {}, "corrected": dict(corrected=True)}

    def sampler():  # a fresh one per call: every call counts the same seeded rows
        return c.compile_detector_sampler(seed=1, noise="device", method="faults")

    times, last = {m: [] for m in legs}, {}
    for kw in legs.values():
        sampler().count(args.shots, batch_size=10**6, decoder=uf, **kw)  # warm-up at the timed size
    for _ in range(args.reps):
        for m, kw in legs.items():
            s = sampler()
            t0 = time.perf_counter()
            last[m] = s.count(args.shots, batch_size=10**6, decoder=uf, **kw)
            times[m].append(time.perf_counter() - t0)
    a = last["plain"]
    out = dict(case=name, p=args.p, shots=args.shots, reps=args.reps, median_s={m: statistics.median(t) for m, t in times.items()},
               min_s={m: min(t) for m, t in times.items()}, max_s={m: max(t) for m, t in times.items()}, kept=a.kept,
               raw_flips=a.kept_with_observable_flip, decoded_errors={m: last[m].decoded_errors for m in legs},
               misses={m: last[m].decoder_misses for m in legs})
    if not args.plain_only:
        b = last["corrected"]
        if (a.kept, a.decoded_errors, a.decoder_misses) != (b.kept, b.decoded_errors, b.decoder_misses):
            sys.exit(f"corrected_bench: {name}: the corrected call did not count what the plain one counted")
        if b.kept_with_observable_flip != b.decoded_errors or int(b.observable_counts.sum()) < b.decoded_errors:
            sys.exit(f"corrected_bench: {name}: the corrected rows do not carry the decoded errors")
        out["observables_left"] = b.observable_counts.tolist()
        out["corrected_over_plain_time"] = out["median_s"]["corrected"] / out["median_s"]["plain"]
    return out


def table(results: list, parent: dict, args) -> str:
    def cell(r, m):
        return f"{r['median_s'][m]:.4f} [{r['min_s'][m]:.4f} .. {r['max_s'][m]:.4f}]"

    lines = [
        "# Corrected observables inside count() (DESIGN.md 3.25), one MI355X.  Surface code memory, rounds = d, all three noise options",
        f"# at p = {args.p:g}, method=\"faults\", count() of {args.shots:.0e} shots in batches of 10^6 with decoder=UnionFindDecoder.from_circuit(c),",
        "# a fresh sampler of seed 1 per call (the same rows in every call), `plain` and `corrected` (corrected=True) alternating, each",
        f"# warmed up first; time: a host clock around a call that ends in a device synchronise, median [min .. max] of {args.reps} calls.",
        "# Both calls agree on kept, decoded_errors and decoder_misses, and the corrected call has kept_with_observable_flip ==",
        "# decoded_errors (the script stops otherwise).",
        "#",
        "# d    leg        seconds per call (median [min .. max])   shots/s     corrected / plain time   decoded errors",
    ]
    for r in results:
        for m in ("plain", "corrected"):
            ratio = f"{r['corrected_over_plain_time']:.3f}" if m == "corrected" else ""
            lines.append(f"  {r['case']:<4} {m:<10} {cell(r, m):<40} {r['shots'] / r['median_s'][m]:.3e}   {ratio:<24} {r['decoded_errors'][m]}")
    if parent:
        lines += ["#", "# The corrected=False leg against the parent commit (scripts/corrected_bench.py --plain-only in a checkout of it, one run of",
                  "# each on the same machine; the same code path):", "#",
                  "# d    parent seconds per call                  this commit                              this / parent time   decoded errors"]
        for r in results:
            q = parent.get(r["case"])
            if q is not None:
                lines.append(f"  {r['case']:<4} {cell(q, 'plain'):<40} {cell(r, 'plain'):<40} {r['median_s']['plain'] / q['median_s']['plain']:.3f}"
                             f"                {q['decoded_errors']['plain']} / {r['decoded_errors']['plain']}")
    lines += ["#", "# The JSON lines:"] + [json.dumps(r) for r in results]
    if parent:
        lines += ["#", "# The parent's JSON lines:"] + [json.dumps(q) for q in parent.values()]
    return "\n".join(lines) + "\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=2 * 10**7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--circuits", default="d5,d9,d15")
    ap.add_argument("--plain-only", action="store_true", help="time count(decoder=uf) alone and print its JSON lines (runs on the parent commit)")
    ap.add_argument("--parent", default=None, metavar="FILE", help="the JSON lines of --plain-only on the parent commit, for the ratio")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corrected_bench.txt"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("corrected_bench: no HIP device - nothing is measured without one")
    parent = {}
    if args.parent:
        with open(args.parent) as f:
            parent = {q["case"]: q for q in (json.loads(line) for line in f if line.startswith("{"))}
    results = []
    for name in args.circuits.split(","):
        results.append(measure(name, args))
        print(json.dumps(results[-1]), flush=True)
    if not args.plain_only:
        with open(args.out, "w") as f:
            f.write(table(results, parent, args))


if __name__ == "__main__":
    main()
