"""The union-find numpy statement, recorded: what a fixed list of decoders decodes fixed rows to.

``tsim_amd/decode.py`` is the oracle of every union-find kernel, so a refactor of it must not move a bit.  This script
builds decoders of every kind the statement has, from the graphs the CPU tests build (no GPU, no library load), decodes per
decoder 256 rows of fixed seeds, the all-zero row and one row per single set detector, and records per decoder a sha256 of
the output of every public reader it supports and, in plain numbers, the totals that show what the rows exercised.

    python scripts/host_checks/uf_statement_trace.py                 # the totals, one line per decoder
    python scripts/host_checks/uf_statement_trace.py --only NAME     # one decoder, with its hashes
    python scripts/host_checks/uf_statement_trace.py --write-golden  # tests/golden/unionfind_statement.json

``tests/test_unionfind_statement_trace.py`` holds the tree to the committed file.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "tests")):   # (the tests import one another by module name)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_unionfind_large import dense_graph  # noqa: E402  (what test_unionfind_matching imports)
from test_unionfind_matching_large import heralded_memory  # noqa: E402
from test_unionfind_windowed import fire, long_memory, time_ladder  # noqa: E402
from test_unionfind_windowed_erasure import herald_ladder  # noqa: E402

from tsim_amd import faults  # noqa: E402
from tsim_amd.decode import UnionFindDecoder, WindowedUnionFindDecoder  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "unionfind_statement.json")
N_ROWS = 256
READERS = ("predictions", "missed", "growth_rounds", "flipped_edges", "soft_outputs", "soft_bin_counts", "match_counts", "gap_outputs",
           "erasure_counts", "mixed_pairs")
TOTALS = ("rows", "decoded", "misses", "matched", "peeled", "with_erased", "overflowed", "mixed", "deficits_between", "gap_bins")


def with_singles(rows: np.ndarray) -> np.ndarray:
    """``rows``, then the all-zero row and one row per single set detector column."""
    return np.concatenate([rows, np.zeros((1, rows.shape[1]), np.bool_), np.eye(rows.shape[1], dtype=np.bool_)])


def fired_rows(graph, seed: int, p=None) -> np.ndarray:
    return with_singles(fire(graph, np.random.default_rng(seed), N_ROWS, p))


def circuit_rows(circuit, seed: int, nd: int) -> np.ndarray:
    """Seeded rows of the circuit's fault sampler on the host: the detector columns, heralds among them."""
    return with_singles(faults.fault_rows_host(circuit.compile_faults(), 0, N_ROWS, (seed, 2)).view(np.bool_)[:, :nd])


def ladder_rows(graph, seed: int, p: float, p_herald: float) -> np.ndarray:
    """Rows of a graph with heralds that no circuit samples: the nodes' columns fire by edge, every herald column is set with
    ``p_herald``."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((N_ROWS, graph.num_detectors), np.bool_)
    rows[:, graph.node_det] = fire(graph, rng, N_ROWS, p)
    rows[:, graph.herald_det] = rng.random((N_ROWS, graph.n_heralds)) < p_herald
    return with_singles(rows)


def decoders() -> dict:
    """name -> ``(decoder, rows)``, in the order of the golden file."""
    out = {}
    # the d = 3 memory of 4 rounds, whole: plain, weighted, cluster matching and the gap
    c = long_memory(3, 4, 2e-2)
    plain, weighted = UnionFindDecoder.from_circuit(c), UnionFindDecoder.from_circuit(c, weights="probability")
    rows = fired_rows(plain.graph, 11)
    out["uf/plain"] = plain, rows
    out["uf/plain/soft"] = plain.with_soft_output("full_edges", 16), rows
    out["uf/weighted"] = weighted, rows
    out["uf/weighted/soft"] = weighted.with_soft_output("correction_weight", 8), rows
    for K in (1, 4, 10):
        out[f"uf/matching/K{K}"] = weighted.with_cluster_matching(K), rows
    out["uf/matching/K4/gap"] = out["uf/matching/K4"][0].with_gap_output(0, bins=16), rows
    # a small random graph with components that have no boundary edge: misses
    g = dense_graph(31, 40, 44)
    sparse = UnionFindDecoder(g, 2)
    rows = fired_rows(g, 12, 0.08)
    out["uf/islands"] = sparse, rows
    out["uf/islands/soft"] = sparse.with_soft_output("largest_cluster", 8), rows
    out["uf/islands/matching/K2/gap"] = sparse.with_cluster_matching(2).with_gap_output(1, bins=8, cap=3000), rows
    # the heralded d = 3 memory of 3 rounds: heralds, erasure matching, with and without a gap, and hubs that overflow
    c = heralded_memory(3, 3, 3e-3, 5e-2)
    heralds = UnionFindDecoder.from_circuit(c, weights="probability", heralds=True)
    rows = circuit_rows(c, 13, heralds.num_detectors)
    out["uf/heralds"] = heralds, rows
    out["uf/heralds/soft"] = heralds.with_soft_output("rounds", 4), rows
    out["uf/erasure/K4"] = heralds.with_erasure_matching(4), rows
    out["uf/erasure/K4/gap"] = out["uf/erasure/K4"][0].with_gap_output(0, bins=16), rows
    out["uf/erasure/K2/H2/gap"] = heralds.with_erasure_matching(2, max_hubs=2).with_gap_output(0, bins=16), rows
    # windows: the d = 3 memory of 12 rounds, a ladder with caps, the ladder with heralds, one window
    c = long_memory(3, 12, 2e-2)
    w_plain = WindowedUnionFindDecoder.from_circuit(c, 16, 32)
    w_weighted = WindowedUnionFindDecoder.from_circuit(c, 16, 32, weights="probability")
    rows = fired_rows(w_plain.graph, 14)
    out["ufw/plain"] = w_plain, rows
    out["ufw/plain/soft"] = w_plain.with_soft_output("full_edges", 32), rows
    out["ufw/weighted"] = w_weighted, rows
    for K in (2, 10):
        out[f"ufw/matching/K{K}"] = w_weighted.with_cluster_matching(K), rows
    g, caps = time_ladder(3, 10, skip=True)
    out["ufw/ladder"] = WindowedUnionFindDecoder(g, 6, 15, edge_caps=caps), fired_rows(g, 15, 0.04)
    g, caps = herald_ladder()
    out["ufw/heralds"] = WindowedUnionFindDecoder(g, 4, 8, edge_caps=caps, heralds=True), ladder_rows(g, 16, 0.06, 0.15)
    g = dense_graph(31, 40, 44)
    rows = fired_rows(g, 12, 0.08)
    out["ufw/one_window"] = WindowedUnionFindDecoder(g, 8, 1000, 2), rows
    out["ufw/one_window/matching/K2"] = out["ufw/one_window"][0].with_cluster_matching(2), rows
    return out


def _digest(x) -> str:
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, (list, tuple)):
            h.update(f"[{len(v)}]".encode())
            for y in v:
                feed(y)
        else:
            a = np.ascontiguousarray(v)
            h.update(f"{a.dtype.str}{list(a.shape)}".encode())
            h.update(a.tobytes())

    feed(x)
    return h.hexdigest()


def outputs(dec, rows: np.ndarray) -> dict:
    """reader -> its output, for the readers ``dec`` supports."""
    matching, windowed = dec.match_defects is not None, isinstance(dec, WindowedUnionFindDecoder)
    gap = getattr(dec, "gap_observable", None) is not None
    out = dict(predictions=dec.predictions(rows), missed=dec.missed(rows), growth_rounds=dec.growth_rounds(rows))
    if not matching:
        out.update(flipped_edges=dec.flipped_edges(rows), soft_outputs=dec.soft_outputs(rows))
    if dec.soft_output is not None:
        out["soft_bin_counts"] = dec.soft_bin_counts(rows, np.arange(len(rows)) % 3 == 0)
    if matching:
        out["match_counts"] = dec.match_counts(rows)
    if gap:
        out["gap_outputs"] = dec.gap_outputs(rows)
    if getattr(dec, "erased_weight", None) is not None:
        out["erasure_counts"] = dec.erasure_counts(rows)
    if matching and windowed:
        out["mixed_pairs"] = dec.mixed_pairs(rows)
    return out


def trace(dec, rows: np.ndarray) -> dict:
    """What the golden file holds of one decoder: a hash per supported reader, and the totals."""
    out = outputs(dec, rows)
    missed = out["missed"]
    decoded = rows[:, dec.graph.node_det].any(axis=1)
    counts = np.asarray(out["match_counts"], np.int64).reshape(-1, 2).sum(axis=0) if "match_counts" in out else (0, 0)
    erasure = out.get("erasure_counts", (0, 0))
    deficits = out.get("gap_outputs")
    totals = dict(rows=len(rows), decoded=int(decoded.sum()), misses=int(missed.sum()), matched=int(counts[0]), peeled=int(counts[1]),
                  with_erased=int(erasure[0]), overflowed=int(erasure[1]), mixed=int(out["mixed_pairs"].sum()) if "mixed_pairs" in out else 0,
                  deficits_between=0 if deficits is None else int(((deficits > 0) & (deficits < dec.gap_cap)).sum()),
                  gap_bins=[] if deficits is None else [int(x) for x in out["soft_bin_counts"][0]])
    assert tuple(totals) == TOTALS
    return dict(sha256={k: _digest(v) for k, v in out.items()}, totals=totals)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", help="the one decoder of this name, with its hashes")
    ap.add_argument("--write-golden", action="store_true", help=f"write {os.path.relpath(GOLDEN, ROOT)}")
    args = ap.parse_args()
    golden = {}
    for name, (dec, rows) in decoders().items():
        if args.only and name != args.only:
            continue
        golden[name] = trace(dec, rows)
        print(f"{name:28s} " + " ".join(f"{k}={v}" for k, v in golden[name]["totals"].items()))
        if args.only:
            for k, v in golden[name]["sha256"].items():
                print(f"   {k:16s} {v}")
    if args.write_golden:
        if args.only:
            ap.error("--write-golden writes every decoder: not with --only")
        with open(GOLDEN, "w") as fh:  # one decoder per line
            fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(golden.items())) + "\n}\n")


if __name__ == "__main__":
    main()
