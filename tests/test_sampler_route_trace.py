"""The sampler's device route makes the device calls it made when ``tests/golden/sampler_route_traces.json`` was
written (CPU): per case the number of calls, their names in order, a hash over every argument, and where the sampler's
two key chains stand afterwards.  The recording stand-in and the cases live in ``scripts/host_checks/route_trace.py``;
run that script to read a trace line by line, and with ``--write-golden`` when the route is meant to change."""

import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("route_trace", os.path.join(ROOT, "scripts", "host_checks", "route_trace.py"))
route_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(route_trace)

with open(route_trace.GOLDEN) as _fh:
    GOLDEN = json.load(_fh)
CASES = route_trace.cases()


def test_the_golden_file_covers_the_cases():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_makes_the_recorded_calls(name):
    log, keys = route_trace.trace(CASES[name])
    got, want = route_trace.summary(log, keys), GOLDEN[name]
    assert got["names"] == want["names"]
    assert got["calls"] == want["calls"]
    assert (got["key"], got["noise_key"]) == (want["key"], want["noise_key"])
    assert got["sha1"] == want["sha1"], f"same calls, other arguments: python scripts/host_checks/route_trace.py --only {name}"
