"""The union-find numpy statement decodes the recorded rows to what it decoded when ``tests/golden/unionfind_statement.json`` was
written (CPU): per decoder a sha256 of the output of every public reader it supports, and in plain numbers the totals (rows,
misses, matched and peeled clusters, clusters with an erased edge, overflowed ones, mixed pairs, the gap bins).  The decoders
and their rows live in ``scripts/host_checks/uf_statement_trace.py``; run that script to read the totals, and with
``--write-golden`` only when what a decoder computes is meant to change."""

import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("uf_statement_trace", os.path.join(ROOT, "scripts", "host_checks", "uf_statement_trace.py"))
uf_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(uf_trace)

with open(uf_trace.GOLDEN) as _fh:
    GOLDEN = json.load(_fh)
_DECODERS: dict = {}


def decoders() -> dict:
    if not _DECODERS:
        _DECODERS.update(uf_trace.decoders())
    return _DECODERS


def test_the_golden_file_covers_the_decoders():
    assert sorted(GOLDEN) == sorted(decoders())


def test_the_recorded_rows_exercise_every_branch():
    """Each of these is non-zero in at least one decoder of its kind: a miss (whole and windowed), a peeled cluster beside matched
    ones, a cluster with an erased edge, an overflowed cluster, a mixed pair, a deficit strictly between 0 and the cap."""
    totals = {name: entry["totals"] for name, entry in GOLDEN.items()}
    assert any(t["misses"] for name, t in totals.items() if name.startswith("uf/"))
    assert any(t["misses"] for name, t in totals.items() if name.startswith("ufw/"))
    for kind in ("uf/matching", "uf/erasure", "ufw/matching"):
        assert any(t["matched"] and t["peeled"] for name, t in totals.items() if name.startswith(kind)), kind
    for key in ("with_erased", "overflowed", "mixed", "deficits_between"):
        assert any(t[key] for t in totals.values()), key
    assert all(sum(t["gap_bins"]) == t["rows"] for t in totals.values() if t["gap_bins"])


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_statement_decodes_what_was_recorded(name):
    got, want = uf_trace.trace(*decoders()[name]), GOLDEN[name]
    assert got["totals"] == want["totals"]
    assert sorted(got["sha256"]) == sorted(want["sha256"])
    for reader in want["sha256"]:
        assert got["sha256"][reader] == want["sha256"][reader], f"{reader}() of {name} moved: python scripts/host_checks/uf_statement_trace.py --only {name}"
