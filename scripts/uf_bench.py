"""The union-find decoder inside ``count()``: surface code memory, rounds = d, one MI355X.

    python scripts/uf_bench.py                       # the table: per distance, JSON lines
    python scripts/uf_bench.py --circuits d15 --shots 1000000
    python scripts/uf_bench.py --resolution 4        # weighted against unweighted growth: d = 5, 9, 15
    python scripts/uf_bench.py --soft largest_cluster  # the price of a soft output: d = 5, 9
    python scripts/uf_bench.py --match 10 --resolution 4  # the price of cluster matching: d = 5, 9
    python scripts/uf_bench.py --gap --resolution 4  # the price of the complementary gap, and what it rejects: d = 5, 9
    python scripts/uf_bench.py --erasure-matching [--gap]  # cluster matching (and the gap) under heralded erasures: d = 5, 9

Per distance the ``method="faults"`` sampler counts ``--shots`` shots per call in batches of 10^6, once without a decoder and
once with ``decoder=UnionFindDecoder.from_circuit(circuit)``, alternating, each warmed up first; the time is a host clock
around a call that returns the counters (it ends in a device synchronise); the median and the spread of ``--reps`` calls are
reported, with the decoded logical error rate, the misses and what ``tsim_uf_info`` says about the kernel (LDS per shot, shots
per block, the most growth rounds a row took).  At d = 3 a ``LookupDecoder`` trained on ``--train`` shots of another seed
runs beside it: the maximum-likelihood bound at that size.  All three noise options are set to ``--p``.

``--resolution R`` is a leg of its own (``--circuits`` then defaults to d5,d9,d15): the same circuit, the same seeded rows and
the same ``count()`` call with ``UnionFindDecoder.from_circuit(circuit)`` and with ``from_circuit(circuit,
weights="probability", resolution=R)``, alternating; both rates with the spread of the calls, both decoded error counts and
misses, and per decoder the most growth rounds ``tsim_uf_info`` reports after decoding ``--info-rows`` sampled rows on a
handle of its own.

``--soft METRIC`` is a leg of its own too (``--circuits`` then defaults to d5,d9): the same ``count()`` call with
``UnionFindDecoder.from_circuit(circuit)`` and with its ``with_soft_output(METRIC, --bins)``, alternating over the same seeded
rows (with ``--resolution R`` both are the weighted decoder): both rates, their ratio, the two histograms and the rejection
curve.  The leg stops when the two calls disagree on a counter or the histograms do not add up to them.

``--match K`` is a leg of its own (``--circuits`` then defaults to d5,d9): the same ``count()`` call with the decoder
(weighted with ``--resolution R``) and with its ``with_cluster_matching(K)``, alternating over the same seeded rows: both rates,
their ratio, both decoded error counts, and what ``tsim_uf_info`` says after ``--info-rows`` rows (LDS per shot, shots per block,
clusters matched and peeled).  The leg stops when the two calls disagree on kept rows, raw flips or misses.

``--gap`` is a leg of its own (``--circuits`` then defaults to d5,d9): the same ``count()`` call with the
cluster-matching decoder (``--match K``, default 10; weighted with ``--resolution R``) and with its ``with_gap_output(0, --bins)``,
alternating over the same seeded rows: both rates and their ratio, the histograms, and the rejection table - the errors left among
the shots kept at 99, 95, 90 and 80 % by the gap, against ``largest_cluster`` of the decoder without matching over the same rows.
The leg stops when the two calls disagree on a counter or the histograms do not add up to them.

``--erasure-matching`` is a leg of its own (``--circuits`` then defaults to d5,d9): the memory circuit with
``after_clifford_heralded_erasure=--pe`` beside the depolarizing and measurement noise of ``--p``, decoded by the herald decoder
(weighted, ``--resolution R``, default 4) and by its ``with_erasure_matching(--match K, erased_weight=--erased-weight,
max_hubs=--max-hubs)``, with ``--gap`` also by that decoder's ``with_gap_output(0, --bins)``, alternating over the same seeded rows:
the rates and their ratios, the decoded errors, what ``tsim_uf_info`` and ``tsim_uf_erasure_info`` say after ``--info-rows`` rows and,
with ``--gap``, the rejection table against ``largest_cluster`` of the herald decoder.  The leg stops when the calls disagree on kept
rows, raw flips or misses, or the gap decoder on the decoded errors of the matching one.
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


def memory(d: int, p: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=p, before_measure_flip_probability=p,
                                                                after_reset_flip_probability=p))


def device_info(hp, sampler, uf, n: int) -> dict:
    """``tsim_uf_info`` of a handle that has decoded ``n`` rows of ``sampler`` (bit-packed on the host, then uploaded)."""
    import numpy as np

    rows = np.ascontiguousarray(np.packbits(sampler.sample(n, append_observables=True), axis=1, bitorder="little"))
    nd, n_cols = uf.num_detectors, uf.num_detectors + uf.num_observables
    h = hp.uf_create(uf.graph, n_cols, uf.edge_caps)
    d_rows, d_cnt = hp.malloc(rows.nbytes + 16), hp.malloc(64)
    try:
        hp.h2d(d_rows, rows)
        hp.h2d(d_cnt, np.zeros(3, np.uint64))
        hp.uf_decode_device(h, d_rows.ptr, len(rows), rows.shape[1], (nd, n_cols), d_cnt.ptr)
        return hp.uf_info(h)
    finally:
        hp.uf_destroy(h)
        d_rows.free()
        d_cnt.free()


def weighted_leg(args) -> None:
    for name in (args.circuits or "d5,d9,d15").split(","):
        d = int(name[1:])
        c = memory(d, args.p)
        decoders = {"unweighted": UnionFindDecoder.from_circuit(c),
                    "weighted": UnionFindDecoder.from_circuit(c, weights="probability", resolution=args.resolution)}
        def sampler():  # a fresh one per call: every call counts the same seeded rows
            return c.compile_detector_sampler(seed=1, noise="device", method="faults")

        times, last = {m: [] for m in decoders}, {}
        for m, uf in decoders.items():
            sampler().count(args.shots, batch_size=10**6, decoder=uf)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, uf in decoders.items():
                s = sampler()
                t0 = time.perf_counter()
                last[m] = s.count(args.shots, batch_size=10**6, decoder=uf)
                times[m].append(time.perf_counter() - t0)
        if last["weighted"].kept_with_observable_flip != last["unweighted"].kept_with_observable_flip:
            sys.exit("uf_bench: the two decoders did not see the same rows")
        hp = s._hip()
        info = {m: device_info(hp, c.compile_detector_sampler(seed=3, noise="device", method="faults"), uf, args.info_rows)
                for m, uf in decoders.items()}
        rate = {m: args.shots / statistics.median(t) for m, t in times.items()}
        caps = decoders["weighted"].edge_caps
        print(json.dumps(dict(
            case=name, leg="resolution", resolution=args.resolution, p=args.p, shots=args.shots, reps=args.reps,
            graph=decoders["unweighted"].info(), caps={int(k): int((caps == k).sum()) for k in sorted(set(caps.tolist()))},
            median_s={m: statistics.median(t) for m, t in times.items()}, min_s={m: min(t) for m, t in times.items()},
            max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate, weighted_over_unweighted=rate["weighted"] / rate["unweighted"],
            kept={m: last[m].kept for m in decoders}, raw_flips={m: last[m].kept_with_observable_flip for m in decoders},
            decoded_errors={m: last[m].decoded_errors for m in decoders}, misses={m: last[m].decoder_misses for m in decoders},
            info_rows=args.info_rows, max_rounds={m: info[m]["max_rounds"] for m in decoders},
            lds_bytes_per_shot={m: info[m]["lds_bytes_per_shot"] for m in decoders},
            shots_per_block={m: info[m]["shots_per_block"] for m in decoders}, grid_blocks={m: info[m]["grid_blocks"] for m in decoders})),
            flush=True)


def soft_leg(args) -> None:
    for name in (args.circuits or "d5,d9").split(","):
        d = int(name[1:])
        c = memory(d, args.p)
        plain = (UnionFindDecoder.from_circuit(c) if args.resolution is None
                 else UnionFindDecoder.from_circuit(c, weights="probability", resolution=args.resolution))
        decoders = {"plain": plain, "soft": plain.with_soft_output(args.soft, args.bins)}
        def sampler():  # a fresh one per call: every call counts the same seeded rows
            return c.compile_detector_sampler(seed=1, noise="device", method="faults")

        times, last = {m: [] for m in decoders}, {}
        for m, uf in decoders.items():
            sampler().count(args.shots, batch_size=10**6, decoder=uf)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, uf in decoders.items():
                s = sampler()
                t0 = time.perf_counter()
                last[m] = s.count(args.shots, batch_size=10**6, decoder=uf)
                times[m].append(time.perf_counter() - t0)
        a, b = last["plain"], last["soft"]
        if (a.kept, a.kept_with_observable_flip, a.decoded_errors, a.decoder_misses) != (b.kept, b.kept_with_observable_flip, b.decoded_errors,
                                                                                         b.decoder_misses):
            sys.exit("uf_bench: the soft decoder did not count what the plain one counted")
        if int(b.soft_kept.sum()) != b.kept or int(b.soft_errors.sum()) != b.decoded_errors:
            sys.exit("uf_bench: the histograms do not add up to the counters")
        rate = {m: args.shots / statistics.median(t) for m, t in times.items()}
        accepted, errors = b.rejection_curve()
        print(json.dumps(dict(
            case=name, leg="soft", metric=args.soft, bins=args.bins, resolution=args.resolution, p=args.p, shots=args.shots, reps=args.reps,
            graph=plain.info(), median_s={m: statistics.median(t) for m, t in times.items()}, min_s={m: min(t) for m, t in times.items()},
            max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate, soft_over_plain=rate["soft"] / rate["plain"], kept=b.kept,
            raw_flips=b.kept_with_observable_flip, decoded_errors=b.decoded_errors, misses=b.decoder_misses,
            soft_kept=b.soft_kept.tolist(), soft_errors=b.soft_errors.tolist(), accepted=accepted.tolist(), errors_accepted=errors.tolist())),
            flush=True)


def match_leg(args) -> None:
    for name in (args.circuits or "d5,d9").split(","):
        d = int(name[1:])
        c = memory(d, args.p)
        plain = (UnionFindDecoder.from_circuit(c) if args.resolution is None
                 else UnionFindDecoder.from_circuit(c, weights="probability", resolution=args.resolution))
        decoders = {"plain": plain, "matching": plain.with_cluster_matching(args.match)}
        def sampler():  # a fresh one per call: every call counts the same seeded rows
            return c.compile_detector_sampler(seed=1, noise="device", method="faults")

        times, last = {m: [] for m in decoders}, {}
        for m, uf in decoders.items():
            sampler().count(args.shots, batch_size=10**6, decoder=uf)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, uf in decoders.items():
                s = sampler()
                t0 = time.perf_counter()
                last[m] = s.count(args.shots, batch_size=10**6, decoder=uf)
                times[m].append(time.perf_counter() - t0)
        a, b = last["plain"], last["matching"]
        if (a.kept, a.kept_with_observable_flip, a.decoder_misses) != (b.kept, b.kept_with_observable_flip, b.decoder_misses):
            sys.exit("uf_bench: the matching decoder did not see the rows, or the misses, of the plain one")
        hp = s._hip()
        um = decoders["matching"]
        rows = c.compile_detector_sampler(seed=3, noise="device", method="faults").sample(args.info_rows, append_observables=True)
        import numpy as np

        packed = np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little"))
        nd, n_cols = um.num_detectors, um.num_detectors + um.num_observables
        h, decode, destroy = um._handle(hp, n_cols)
        d_rows, d_cnt = hp.malloc(packed.nbytes + 16), hp.malloc(64)
        try:
            hp.h2d(d_rows, packed)
            hp.h2d(d_cnt, np.zeros(3, np.uint64))
            decode(h, d_rows.ptr, len(packed), packed.shape[1], (nd, n_cols), d_cnt.ptr)
            info = hp.uf_info(h)
        finally:
            destroy(h)
            d_rows.free()
            d_cnt.free()
        rate = {m: args.shots / statistics.median(t) for m, t in times.items()}
        print(json.dumps(dict(
            case=name, leg="match", max_defects=args.match, resolution=args.resolution, p=args.p, shots=args.shots, reps=args.reps,
            graph=plain.info(), median_s={m: statistics.median(t) for m, t in times.items()}, min_s={m: min(t) for m, t in times.items()},
            max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate, matching_over_plain=rate["matching"] / rate["plain"], kept=b.kept,
            raw_flips=b.kept_with_observable_flip, decoded_errors={m: last[m].decoded_errors for m in decoders}, misses=b.decoder_misses,
            info_rows=args.info_rows, lds_bytes_per_shot=info["lds_bytes_per_shot"], shots_per_block=info["shots_per_block"],
            clusters_matched=info["clusters_matched"], clusters_peeled=info["clusters_peeled"], rows_decoded=info["rows_decoded"],
            device_bytes=info["device_bytes"])), flush=True)


def gap_leg(args) -> None:
    K = 10 if args.match is None else args.match
    for name in (args.circuits or "d5,d9").split(","):
        d = int(name[1:])
        c = memory(d, args.p)
        plain = (UnionFindDecoder.from_circuit(c) if args.resolution is None
                 else UnionFindDecoder.from_circuit(c, weights="probability", resolution=args.resolution))
        um = plain.with_cluster_matching(K)
        decoders = {"matching": um, "gap": um.with_gap_output(0, args.bins)}
        def sampler():  # a fresh one per call: every call counts the same seeded rows
            return c.compile_detector_sampler(seed=1, noise="device", method="faults")

        times, last = {m: [] for m in decoders}, {}
        for m, uf in decoders.items():
            sampler().count(args.shots, batch_size=10**6, decoder=uf)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, uf in decoders.items():
                s = sampler()
                t0 = time.perf_counter()
                last[m] = s.count(args.shots, batch_size=10**6, decoder=uf)
                times[m].append(time.perf_counter() - t0)
        a, b = last["matching"], last["gap"]
        if (a.kept, a.kept_with_observable_flip, a.decoded_errors, a.decoder_misses) != (b.kept, b.kept_with_observable_flip, b.decoded_errors,
                                                                                         b.decoder_misses):
            sys.exit("uf_bench: the gap decoder did not count what the matching one counted")
        if int(b.soft_kept.sum()) != b.kept or int(b.soft_errors.sum()) != b.decoded_errors:
            sys.exit("uf_bench: the histograms do not add up to the counters")
        # the rejection table: the errors left among the shots kept when each signal discards the least sure ones
        other = sampler().count(args.shots, batch_size=10**6, decoder=plain.with_soft_output("largest_cluster", args.bins))
        table = {}
        for signal, counts in (("gap", b), ("largest_cluster", other)):
            accepted, errors = counts.rejection_curve()
            for keep in (0.99, 0.95, 0.90, 0.80):
                t = int((accepted >= keep * counts.kept).argmax())  # the first bin that keeps at least that much
                table[f"{signal}@{keep:.2f}"] = dict(bin=t, kept=int(accepted[t]), errors=int(errors[t]), rate=float(errors[t] / accepted[t]))
        hp = s._hip()
        ug = decoders["gap"]
        h, _, destroy = ug._handle(hp, ug.num_detectors + ug.num_observables)
        try:
            info = hp.uf_info(h)
        finally:
            destroy(h)
        rate = {m: args.shots / statistics.median(t) for m, t in times.items()}
        print(json.dumps(dict(
            case=name, leg="gap", max_defects=K, bins=args.bins, gap_cap=ug.gap_cap, gap_step=ug.gap_step, resolution=args.resolution, p=args.p,
            shots=args.shots, reps=args.reps, graph=plain.info(), median_s={m: statistics.median(t) for m, t in times.items()},
            min_s={m: min(t) for m, t in times.items()}, max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate,
            gap_over_matching=rate["gap"] / rate["matching"], kept=b.kept, raw_flips=b.kept_with_observable_flip,
            decoded_errors=dict(matching=a.decoded_errors, gap=b.decoded_errors, plain=other.decoded_errors), misses=b.decoder_misses,
            lds_bytes_per_shot=info["lds_bytes_per_shot"], shots_per_block=info["shots_per_block"], device_bytes=info["device_bytes"],
            rejection=table, soft_kept=b.soft_kept.tolist(), soft_errors=b.soft_errors.tolist())), flush=True)


def erasure_leg(args) -> None:
    import numpy as np

    K = 10 if args.match is None else args.match
    R = 4 if args.resolution is None else args.resolution
    for name in (args.circuits or "d5,d9").split(","):
        d = int(name[1:])
        c = CliffordCircuit(circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=args.p, before_measure_flip_probability=args.p,
                                                                 after_clifford_heralded_erasure=args.pe))
        plain = UnionFindDecoder.from_circuit(c, weights="probability", resolution=R, heralds=True)
        ue = plain.with_erasure_matching(K, erased_weight=args.erased_weight, max_hubs=args.max_hubs)
        decoders = {"heralds": plain, "erasure_matching": ue}
        if args.gap:
            decoders["gap"] = ue.with_gap_output(0, args.bins)
        def sampler():  # a fresh one per call: every call counts the same seeded rows
            return c.compile_detector_sampler(seed=1, noise="device", method="faults")

        times, last = {m: [] for m in decoders}, {}
        for m, uf in decoders.items():
            sampler().count(args.shots, batch_size=10**6, decoder=uf)  # warm-up at the timed size
        for _ in range(args.reps):
            for m, uf in decoders.items():
                s = sampler()
                t0 = time.perf_counter()
                last[m] = s.count(args.shots, batch_size=10**6, decoder=uf)
                times[m].append(time.perf_counter() - t0)
        a = last["heralds"]
        for m in decoders:
            if (a.kept, a.kept_with_observable_flip, a.decoder_misses) != (last[m].kept, last[m].kept_with_observable_flip, last[m].decoder_misses):
                sys.exit(f"uf_bench: {m} did not see the rows, or the misses, of the herald decoder")
        table = None
        if args.gap:
            b = last["gap"]
            if b.decoded_errors != last["erasure_matching"].decoded_errors or int(b.soft_kept.sum()) != b.kept or int(b.soft_errors.sum()) != b.decoded_errors:
                sys.exit("uf_bench: the gap decoder did not count what the matching one counted")
            other = sampler().count(args.shots, batch_size=10**6, decoder=plain.with_soft_output("largest_cluster", args.bins))
            table = {}
            for signal, counts in (("gap", b), ("largest_cluster", other)):
                accepted, errors = counts.rejection_curve()
                for keep in (0.99, 0.95, 0.90, 0.80):
                    t = int((accepted >= keep * counts.kept).argmax())  # the first bin that keeps at least that much
                    table[f"{signal}@{keep:.2f}"] = dict(bin=t, kept=int(accepted[t]), errors=int(errors[t]), rate=float(errors[t] / accepted[t]))
        hp = s._hip()
        rows = c.compile_detector_sampler(seed=3, noise="device", method="faults").sample(args.info_rows, append_observables=True)
        packed = np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little"))
        nd, n_cols = ue.num_detectors, ue.num_detectors + ue.num_observables
        info = {}
        for m, uf in decoders.items():
            h, decode, destroy = uf._handle(hp, n_cols)
            d_rows, d_cnt = hp.malloc(packed.nbytes + 16), hp.malloc(64)
            try:
                hp.h2d(d_rows, packed)
                hp.h2d(d_cnt, np.zeros(3, np.uint64))
                decode(h, d_rows.ptr, len(packed), packed.shape[1], (nd, n_cols), d_cnt.ptr)
                info[m] = dict(hp.uf_info(h), **(hp.uf_erasure_info(h) if m != "heralds" else {}))
            finally:
                destroy(h)
                d_rows.free()
                d_cnt.free()
        rate = {m: args.shots / statistics.median(t) for m, t in times.items()}
        keys = ("lds_bytes_per_shot", "shots_per_block", "grid_blocks", "max_rounds", "rows_decoded", "clusters_matched", "clusters_peeled",
                "clusters_erased", "clusters_hub_overflow", "device_bytes")
        print(json.dumps(dict(
            case=name, leg="erasure_matching", max_defects=K, erased_weight=args.erased_weight, max_hubs=args.max_hubs, resolution=R, p=args.p,
            pe=args.pe, shots=args.shots, reps=args.reps, graph=plain.info(), median_s={m: statistics.median(t) for m, t in times.items()},
            min_s={m: min(t) for m, t in times.items()}, max_s={m: max(t) for m, t in times.items()}, shots_per_s=rate,
            over_heralds={m: rate[m] / rate["heralds"] for m in decoders if m != "heralds"}, kept=a.kept, raw_flips=a.kept_with_observable_flip,
            decoded_errors={m: last[m].decoded_errors for m in decoders}, misses=a.decoder_misses, info_rows=args.info_rows,
            info={m: {k: v[k] for k in keys if k in v} for m, v in info.items()}, rejection=table,
            **(dict(gap_cap=decoders["gap"].gap_cap, gap_step=decoders["gap"].gap_step, soft_kept=last["gap"].soft_kept.tolist(),
                    soft_errors=last["gap"].soft_errors.tolist()) if args.gap else {}))), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10**7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--circuits", default=None, help="default d3,d5,d7,d11,d15; d5,d9,d15 with --resolution")
    ap.add_argument("--train", type=int, default=10**8)
    ap.add_argument("--resolution", type=int, default=None, help="the leg that runs weighted against unweighted growth")
    ap.add_argument("--info-rows", type=int, default=20000)
    ap.add_argument("--soft", default=None, metavar="METRIC",
                    help="the leg that runs a decoder with this soft output against the same decoder without (weighted with --resolution)")
    ap.add_argument("--bins", type=int, default=64, help="the bins of --soft")
    ap.add_argument("--match", type=int, default=None, metavar="K",
                    help="the leg that runs a decoder with cluster matching of at most K defects against the same decoder without")
    ap.add_argument("--gap", action="store_true",
                    help="the leg that runs the cluster-matching decoder (--match K, default 10) with the complementary gap against the same without")
    ap.add_argument("--erasure-matching", action="store_true",
                    help="the leg that runs cluster matching under heralded erasures (with --gap: and its gap) against the herald decoder")
    ap.add_argument("--pe", type=float, default=1e-2, help="the heralded erasure probability of --erasure-matching")
    ap.add_argument("--erased-weight", type=int, default=1)
    ap.add_argument("--max-hubs", type=int, default=24)
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("uf_bench: no HIP device - nothing is measured without one")
    if args.erasure_matching:
        return erasure_leg(args)
    if args.gap:
        return gap_leg(args)
    if args.match is not None:
        return match_leg(args)
    if args.soft is not None:
        return soft_leg(args)
    if args.resolution is not None:
        return weighted_leg(args)
    for name in (args.circuits or "d3,d5,d7,d11,d15").split(","):
        d = int(name[1:])
        c = memory(d, args.p)
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
