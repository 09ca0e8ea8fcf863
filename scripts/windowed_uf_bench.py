"""Sliding-window union-find decoding next to the whole-graph decoder: surface code memory, one MI355X.

    python scripts/windowed_uf_bench.py                                  # the four legs below, JSON lines
    python scripts/windowed_uf_bench.py --legs rate --cases d9x27c9
    python scripts/windowed_uf_bench.py --legs quality --shots 1000000
    python scripts/windowed_uf_bench.py --match 10                       # cluster matching in windows: the ``match`` leg alone

A case ``d<D>x<R>c<C>`` is ``rotated_surface_code_memory(D, R)`` with all three noise options at ``--p``, decoded in windows
of ``commit = C`` rounds and ``window = 2 C`` rounds (a round is ``D * D - 1`` detector columns), unweighted.

``rate``: ``count(--shots, decoder=...)`` of the ``method="faults"`` sampler, in batches of ``--batch``, with the whole-graph
``UnionFindDecoder`` and with the ``WindowedUnionFindDecoder``, alternating, each warmed up first, on the same seeded rows; a
host clock around a call that returns the counters; the median and the spread of ``--reps`` calls.  A decoder that cannot be
built (the graph passes 65535 nodes or edges, or its state passes a block's LDS) is reported as such and left out, and so is
a sampler that does not build.  Then the decoders alone: ``--decode-rows`` rows of ``faults.fault_rows_host``, bit-packed and
uploaded, through ``tsim_uf_decode_device`` / ``tsim_ufw_decode_device`` on handles of their own (a host clock around the call
and a stream synchronise, median of ``--reps``), with what ``tsim_uf_info`` / ``tsim_ufw_info`` report.

``quality``: ``decoded_errors`` of the whole-graph decoder and of the windowed one for each ``--commits`` (rounds) on the same
``--quality-shots`` seeded shots of ``--quality-case`` at ``--quality-p``.

``erasure``: the ``--erasure-cases`` with ``after_clifford_depolarization = before_measure_flip_probability =
--p`` and ``after_clifford_heralded_erasure = --pe``; ``count(--erasure-shots, decoder=...)`` as in ``rate``, of the whole-graph
decoder with heralds (where it is built and fits), of the windowed decoder with heralds, and of the same windows over heralds
that list no edge (what ignoring the heralds costs in decoded errors), on the same seeded rows.

``soft`` (``profiles/windowed_soft_bench.txt``): ``--soft-case`` (d = 5, 400 rounds, commit = 120 and window = 240
columns), ``count(--soft-shots, decoder=...)`` as in ``rate`` of the windowed decoder and of the same decoder
``with_soft_output(--soft-metric, --soft-bins)``, alternating, and the errors ``rejection_curve()`` leaves at ``--soft-kept``.

``match`` (``--match K``; ``profiles/windowed_matching_bench.txt``): windowed peeling against
``with_cluster_matching(K)``.  Error counts: the ``--match-cases`` ``d<D>x<R>p<P>n<ROWS>``, ``weights="probability"``, commit = 2 and
window = 4 rounds, ``after_clifford_depolarization = before_measure_flip_probability = P``, rows of
``compile_detector_sampler(seed=3).sample()``; both decoders decode the uploaded rows on the device and by the numpy statement, which
must agree bit for bit.  Throughput: ``count(--soft-shots, decoder=...)`` of ``--soft-case`` as in ``soft``, the plain windowed
decoder and the matching one alternating, and the create call alone (it builds the match tables), ``--reps`` times each.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tsim_amd import _lib, circuits, faults, synth  # noqa: E402
from tsim_amd.backend import HipProgram  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402
from tsim_amd.decode import DecodingGraph, UnionFindDecoder, WindowedUnionFindDecoder  # noqa: E402


def memory(d: int, rounds: int, p: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, before_measure_flip_probability=p,
                                                                after_reset_flip_probability=p))


def parse(case: str):
    d, rest = case[1:].split("x")
    rounds, commit = rest.split("c")
    return int(d), int(rounds), int(commit)


def spread(times) -> dict:
    return dict(median_s=statistics.median(times), min_s=min(times), max_s=max(times))


def decoders_of(form, d: int, commit: int) -> tuple:
    """``({name: decoder}, {name: why it was not built})`` of the whole graph and of windows of ``commit`` + ``commit`` rounds."""
    n_obs = int(form.n_out) - int(form.num_detectors)
    built, refused = {}, {}
    try:
        built["whole"] = UnionFindDecoder(DecodingGraph.from_form(form), n_obs)
    except NotImplementedError as e:
        refused["whole"] = str(e)
    cols = commit * (d * d - 1)
    built["windowed"] = WindowedUnionFindDecoder(DecodingGraph.from_form(form, limit=None), cols, 2 * cols, n_obs)
    return built, refused


def decode_alone(hp, dec, rows: np.ndarray, reps: int) -> dict:
    """The decode call alone on uploaded rows: its times and the handle's info."""
    nd, n_cols = dec.num_detectors, dec.num_detectors + dec.num_observables
    windowed = isinstance(dec, WindowedUnionFindDecoder)
    h = hp.ufw_create(dec.graph, n_cols, dec.commit, dec.window, dec.edge_caps) if windowed else hp.uf_create(dec.graph, n_cols, dec.edge_caps)
    run, info, destroy = (hp.ufw_decode_device, hp.ufw_info, hp.ufw_destroy) if windowed else (hp.uf_decode_device, hp.uf_info, hp.uf_destroy)
    d_rows, d_cnt = hp.malloc(rows.nbytes + 16), hp.malloc(64)
    try:
        hp.h2d(d_rows, rows)
        times = []
        for i in range(reps + 1):  # (the first call warms up)
            hp.h2d(d_cnt, np.zeros(3, np.uint64))
            hp.stream_synchronize(0)
            t0 = time.perf_counter()
            run(h, d_rows.ptr, len(rows), rows.shape[1], (nd, n_cols), d_cnt.ptr)
            hp.stream_synchronize(0)
            times.append(time.perf_counter() - t0)
        cnt = np.zeros(3, np.uint64)
        hp.d2h(cnt, d_cnt)
        out = spread(times[1:])
        out.update(rows=len(rows), rows_per_s=len(rows) / out["median_s"], kept_wrong_missed=[int(x) for x in cnt], info=info(h))
        return out
    finally:
        destroy(h)
        d_rows.free()
        d_cnt.free()


def rate_leg(args, hp) -> None:
    for case in args.cases.split(","):
        d, rounds, commit = parse(case)
        c = memory(d, rounds, args.p)
        t0 = time.perf_counter()
        form = c.compile_faults()
        form_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        decoders, refused = decoders_of(form, d, commit)
        out = dict(leg="rate", case=case, p=args.p, commit_rounds=commit, window_rounds=2 * commit, form_s=form_s,
                   decoders_s=time.perf_counter() - t0, graph=decoders["windowed"].info(), not_built=refused)
        # count(): sampling and decoding together
        try:
            def sampler():  # a fresh one per call: every call counts the same seeded rows
                return c.compile_detector_sampler(seed=1, noise="device", method="faults")

            times, last = {m: [] for m in decoders}, {}
            for m, dec in decoders.items():
                sampler().count(args.shots, batch_size=args.batch, decoder=dec)  # warm-up at the timed size
            for _ in range(args.reps):
                for m, dec in decoders.items():
                    s = sampler()
                    t0 = time.perf_counter()
                    last[m] = s.count(args.shots, batch_size=args.batch, decoder=dec)
                    times[m].append(time.perf_counter() - t0)
            out["count"] = {m: dict(spread(t), shots=args.shots, shots_per_s=args.shots / statistics.median(t), kept=last[m].kept,
                                    raw_flips=last[m].kept_with_observable_flip, decoded_errors=last[m].decoded_errors,
                                    misses=last[m].decoder_misses) for m, t in times.items()}
        except (NotImplementedError, ValueError, MemoryError, _lib.HipBackendError) as e:
            if "failed:" in str(e):  # (a HIP call failed: that is no refusal, and nothing more is started on the device)
                raise
            out["count"] = dict(not_run=f"{type(e).__name__}: {e}")
        # the decoders alone, on the same uploaded rows
        bits = faults.fault_rows_host(form, 0, args.decode_rows, (3, 4))
        rows = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little"))
        rows = np.ascontiguousarray(np.pad(rows, ((0, 0), (0, -rows.shape[1] % 8))))
        out["mean_defects_per_row"] = float(bits[:, :int(form.num_detectors)].sum(axis=1).mean())
        out["decode_alone"] = {}
        for m, dec in decoders.items():
            try:
                out["decode_alone"][m] = decode_alone(hp, dec, rows, args.reps)
            except _lib.HipBackendError as e:
                if "failed:" in str(e):
                    raise
                out["decode_alone"][m] = dict(not_run=str(e))
        print(json.dumps(out), flush=True)


def quality_leg(args) -> None:
    d, rounds, _ = parse(args.quality_case + "c1")
    c = memory(d, rounds, args.quality_p)
    form = c.compile_faults()
    n_obs = int(form.n_out) - int(form.num_detectors)
    g = DecodingGraph.from_form(form)
    decoders = {"whole": UnionFindDecoder(g, n_obs)}
    for k in (int(x) for x in args.commits.split(",")):
        decoders[f"commit{k}"] = WindowedUnionFindDecoder(g, k * (d * d - 1), 2 * k * (d * d - 1), n_obs)
    res = {}
    for m, dec in decoders.items():
        t0 = time.perf_counter()
        r = c.compile_detector_sampler(seed=5, noise="device", method="faults").count(args.quality_shots, batch_size=args.batch, decoder=dec)
        res[m] = dict(kept=r.kept, raw_flips=r.kept_with_observable_flip, decoded_errors=r.decoded_errors, misses=r.decoder_misses,
                      seconds=time.perf_counter() - t0, windows=dec.info().get("n_windows", 1))
    if len({(r["kept"], r["raw_flips"]) for r in res.values()}) != 1:
        sys.exit("windowed_uf_bench: the decoders did not see the same rows")
    print(json.dumps(dict(leg="quality", case=args.quality_case, p=args.quality_p, shots=args.quality_shots, graph=g.info(), results=res)), flush=True)


def erasure_memory(d: int, rounds: int, p: float, pe: float) -> CliffordCircuit:
    return CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, before_measure_flip_probability=p,
                                                                after_clifford_heralded_erasure=pe))


def erasure_leg(args) -> None:
    """``count(--erasure-shots, decoder=...)`` on the same seeded rows of the heralded memory: the whole graph with heralds (where
    it is built and fits), windows with heralds, and the same windows with the heralds ignored (their decoded errors only)."""
    for case in args.erasure_cases.split(","):
        d, rounds, commit = parse(case)
        c = erasure_memory(d, rounds, args.p, args.pe)
        t0 = time.perf_counter()
        form = c.compile_faults()
        form_s = time.perf_counter() - t0
        n_obs = int(form.n_out) - int(form.num_detectors)
        cols = commit * (d * d - 1)
        t0 = time.perf_counter()
        g = DecodingGraph.from_form(form, heralds=True, limit=None)
        decoders, refused = {}, {}
        try:
            decoders["whole"] = UnionFindDecoder(DecodingGraph.from_form(form, heralds=True), n_obs)
        except NotImplementedError as e:
            refused["whole"] = str(e)
        decoders["windowed"] = WindowedUnionFindDecoder(g, cols, 2 * cols, n_obs, heralds=True)
        blind = DecodingGraph(g.n_nodes, g.edge_u, g.edge_v, g.edge_obs, g.edge_p, node_det=g.node_det, herald_det=g.herald_det,
                              herald_ptr=np.zeros(g.n_heralds + 1, np.int64), herald_edges=[], limit=None)   # the heralds list nothing
        decoders["windowed_heralds_ignored"] = WindowedUnionFindDecoder(blind, cols, 2 * cols, n_obs, heralds=True)
        out = dict(leg="erasure", case=case, p=args.p, pe=args.pe, commit_rounds=commit, window_rounds=2 * commit, form_s=form_s,
                   decoders_s=time.perf_counter() - t0, graph=decoders["windowed"].info(), n_cols=int(form.n_out), not_built=refused,
                   heralds_per_window=[len(w.heralds) for w in decoders["windowed"].windows()][:8])

        def sampler():  # a fresh one per call: every call counts the same seeded rows
            return c.compile_detector_sampler(seed=1, noise="device", method="faults")

        times, last = {}, {}
        for m, dec in list(decoders.items()):
            try:
                last[m] = sampler().count(args.erasure_shots, batch_size=args.batch, decoder=dec)  # warm-up at the timed size
                times[m] = []
            except (NotImplementedError, ValueError, MemoryError, _lib.HipBackendError) as e:
                if "failed:" in str(e):  # (a HIP call failed: that is no refusal, and nothing more is started on the device)
                    raise
                refused[m] = f"{type(e).__name__}: {e}"
        for _ in range(args.reps):
            for m in times:
                s = sampler()
                t0 = time.perf_counter()
                last[m] = s.count(args.erasure_shots, batch_size=args.batch, decoder=decoders[m])
                times[m].append(time.perf_counter() - t0)
        out["count"] = {m: dict(spread(t), shots=args.erasure_shots, shots_per_s=args.erasure_shots / statistics.median(t), kept=last[m].kept,
                                raw_flips=last[m].kept_with_observable_flip, decoded_errors=last[m].decoded_errors,
                                misses=last[m].decoder_misses) for m, t in times.items()}
        print(json.dumps(out), flush=True)


def soft_leg(args) -> None:
    """``count(--soft-shots, decoder=...)`` of the windowed decoder of ``--soft-case`` with and without
    ``with_soft_output(--soft-metric, --soft-bins)``, alternating on the same seeded rows, and what ``rejection_curve()`` leaves
    at each of ``--soft-kept``: the lowest bin threshold that accepts at least that share of the kept shots."""
    d, rounds, commit = parse(args.soft_case)
    c = memory(d, rounds, args.p)
    t0 = time.perf_counter()
    form = c.compile_faults()
    form_s = time.perf_counter() - t0
    cols = commit * (d * d - 1)
    t0 = time.perf_counter()
    plain = WindowedUnionFindDecoder(DecodingGraph.from_form(form, limit=None), cols, 2 * cols, int(form.n_out) - int(form.num_detectors))
    decoders = {"plain": plain, "soft": plain.with_soft_output(args.soft_metric, args.soft_bins)}
    out = dict(leg="soft", case=args.soft_case, p=args.p, commit_columns=cols, window_columns=2 * cols, metric=args.soft_metric,
               bins=args.soft_bins, form_s=form_s, decoders_s=time.perf_counter() - t0, graph=plain.info())

    def sampler():  # a fresh one per call: every call counts the same seeded rows
        return c.compile_detector_sampler(seed=1, noise="device", method="faults")

    times, last = {m: [] for m in decoders}, {}
    for m, dec in decoders.items():
        sampler().count(args.soft_shots, batch_size=args.batch, decoder=dec)  # warm-up at the timed size
    for _ in range(args.reps):
        for m, dec in decoders.items():
            s = sampler()
            t0 = time.perf_counter()
            last[m] = s.count(args.soft_shots, batch_size=args.batch, decoder=dec)
            times[m].append(time.perf_counter() - t0)
    out["count"] = {m: dict(spread(t), shots=args.soft_shots, shots_per_s=args.soft_shots / statistics.median(t), kept=last[m].kept,
                            raw_flips=last[m].kept_with_observable_flip, decoded_errors=last[m].decoded_errors,
                            misses=last[m].decoder_misses) for m, t in times.items()}
    if (last["plain"].kept, last["plain"].decoded_errors) != (last["soft"].kept, last["soft"].decoded_errors):
        sys.exit("windowed_uf_bench: the soft call does not count what the plain call counts")
    res = last["soft"]
    accepted, errors = res.rejection_curve()
    out["soft_kept"], out["soft_errors"] = res.soft_kept.tolist(), res.soft_errors.tolist()
    out["rejection"] = []
    for share in (float(x) for x in args.soft_kept.split(",")):
        t = int(np.searchsorted(accepted, share * res.kept))  # (the last entry is `kept`: always found)
        out["rejection"].append(dict(kept_share_asked=share, threshold_bin=t, accepted=int(accepted[t]), errors=int(errors[t]),
                                     accepted_share=int(accepted[t]) / res.kept, error_rate=int(errors[t]) / int(accepted[t])))
    print(json.dumps(out), flush=True)


def match_leg(args, hp) -> None:
    """Windowed peeling against windowed cluster matching with ``K = --match``: decoded errors on the ``--match-cases``, device
    and numpy statement bit for bit, then the shots per second of both on ``--soft-case`` and the time of the create call."""
    K = args.match
    for case in args.match_cases.split(","):
        d, rest = case[1:].split("x")
        rounds, rest = rest.split("p")
        p, n = rest.split("n")
        d, rounds, p, n = int(d), int(rounds), float(p), int(n)
        c = CliffordCircuit(circuits.rotated_surface_code_memory(d, rounds, after_clifford_depolarization=p, before_measure_flip_probability=p))
        cols = 2 * (d * d - 1)
        peel = WindowedUnionFindDecoder.from_circuit(c, cols, 2 * cols, weights="probability")
        decoders = {"peeling": peel, "matching": peel.with_cluster_matching(K)}
        bits = np.asarray(c.compile_detector_sampler(seed=3).sample(n, append_observables=True), dtype=np.bool_)
        nd, n_obs = peel.num_detectors, peel.num_observables
        obs = (bits[:, nd:nd + n_obs].astype(np.uint64) << np.arange(n_obs, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        rows = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little"))
        rows = np.ascontiguousarray(np.pad(rows, ((0, 0), (0, -rows.shape[1] % 8))))
        out = dict(leg="match", part="errors", case=case, K=K, rows=n, commit_columns=cols, window_columns=2 * cols, windows=peel.info()["n_windows"],
                   raw_flips=int((obs != 0).sum()))
        d_rows = hp.malloc(rows.nbytes + 16)
        try:
            hp.h2d(d_rows, rows)
            for m, dec in decoders.items():
                t0 = time.perf_counter()
                want = dec.predictions(bits[:, :nd])
                host_s = time.perf_counter() - t0
                pred, (kept, wrong, missed) = dec.decode_device(hp, d_rows.ptr, n, rows.shape[1])
                if not np.array_equal(pred, want) or wrong != int((want != obs).sum()) or missed != int(dec.missed(bits[:, :nd]).sum()):
                    sys.exit(f"windowed_uf_bench: {case}: the device and the numpy statement of windowed {m} differ "
                             f"({int((pred != want).sum())} rows)")
                out[m] = dict(decoded_errors=wrong, misses=missed, numpy_statement_s=host_s)
            counts = decoders["matching"].match_counts(bits[:, :nd]).sum(0)
            out["clusters_matched"], out["clusters_peeled"] = int(counts[0]), int(counts[1])
            out["rows_with_a_path_committed_in_part"] = int((decoders["matching"].mixed_pairs(bits[:, :nd]) > 0).sum())
        finally:
            d_rows.free()
        print(json.dumps(out), flush=True)
    # throughput on the long run
    d, rounds, commit = parse(args.soft_case)
    c = memory(d, rounds, args.p)
    form = c.compile_faults()
    cols = commit * (d * d - 1)
    plain = WindowedUnionFindDecoder(DecodingGraph.from_form(form, limit=None), cols, 2 * cols, int(form.n_out) - int(form.num_detectors))
    decoders = {"plain": plain, "matching": plain.with_cluster_matching(K)}
    out = dict(leg="match", part="throughput", case=args.soft_case, p=args.p, K=K, commit_columns=cols, window_columns=2 * cols, graph=plain.info())
    n_cols = int(form.n_out)
    creates = []
    for _ in range(args.reps + 1):  # (the first call warms up)
        t0 = time.perf_counter()
        h = hp.ufw_create_matching(plain.graph, n_cols, decoders["matching"].match_weights, K, plain.commit, plain.window)
        creates.append(time.perf_counter() - t0)
        out["handle"], out["match_info"] = hp.ufw_info(h), hp.ufw_match_info(h)
        hp.ufw_destroy(h)
    out["create_matching"] = spread(creates[1:])
    creates = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        h = hp.ufw_create(plain.graph, n_cols, plain.commit, plain.window)
        creates.append(time.perf_counter() - t0)
        hp.ufw_destroy(h)
    out["create_plain"] = spread(creates[1:])

    def sampler():  # a fresh one per call: every call counts the same seeded rows
        return c.compile_detector_sampler(seed=1, noise="device", method="faults")

    times, last = {m: [] for m in decoders}, {}
    for m, dec in decoders.items():
        sampler().count(args.soft_shots, batch_size=args.batch, decoder=dec)  # warm-up at the timed size
    for _ in range(args.reps):
        for m, dec in decoders.items():
            s = sampler()
            t0 = time.perf_counter()
            last[m] = s.count(args.soft_shots, batch_size=args.batch, decoder=dec)
            times[m].append(time.perf_counter() - t0)
    out["count"] = {m: dict(spread(t), shots=args.soft_shots, shots_per_s=args.soft_shots / statistics.median(t), kept=last[m].kept,
                            raw_flips=last[m].kept_with_observable_flip, decoded_errors=last[m].decoded_errors,
                            misses=last[m].decoder_misses) for m, t in times.items()}
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=None, help="rate,quality,erasure,soft (all four unless --match is given), match")
    ap.add_argument("--match", type=int, default=0, help="K of with_cluster_matching for the match leg")
    ap.add_argument("--match-cases", default="d3x12p3e-3n40000,d3x12p5e-3n40000,d5x20p3e-3n6000")
    ap.add_argument("--soft-case", default="d5x400c5")
    ap.add_argument("--soft-shots", type=int, default=100000)
    ap.add_argument("--soft-metric", default="largest_cluster")
    ap.add_argument("--soft-bins", type=int, default=64)
    ap.add_argument("--soft-kept", default="0.99,0.95,0.90")
    ap.add_argument("--erasure-cases", default="d5x20c5,d9x27c9")
    ap.add_argument("--erasure-shots", type=int, default=200000)
    ap.add_argument("--pe", type=float, default=1e-2)
    ap.add_argument("--cases", default="d9x27c9,d11x500c11")
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--shots", type=int, default=10**6)
    ap.add_argument("--batch", type=int, default=10**5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decode-rows", type=int, default=4096)
    ap.add_argument("--quality-case", default="d5x20")
    ap.add_argument("--quality-p", type=float, default=2e-3)
    ap.add_argument("--quality-shots", type=int, default=10**6)
    ap.add_argument("--commits", default="2,5")
    args = ap.parse_args()
    if args.legs is None:
        args.legs = "match" if args.match else "rate,quality,erasure,soft"
    if "match" in args.legs.split(",") and not 1 <= args.match <= 12:
        sys.exit("windowed_uf_bench: the match leg needs --match K, 1 .. 12")
    _lib.load()
    if _lib.device_count() < 1:
        sys.exit("windowed_uf_bench: no HIP device - nothing is measured without one")
    if "quality" in args.legs.split(","):
        quality_leg(args)
    if "rate" in args.legs.split(","):
        rate_leg(args, HipProgram(synth.kat_h_m()))
    if "erasure" in args.legs.split(","):
        erasure_leg(args)
    if "soft" in args.legs.split(","):
        soft_leg(args)
    if "match" in args.legs.split(","):
        match_leg(args, HipProgram(synth.kat_h_m()))


if __name__ == "__main__":
    main()
