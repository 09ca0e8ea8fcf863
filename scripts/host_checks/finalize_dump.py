#!/usr/bin/env python3
"""Writes the program dump that ``finalize_replay.cpp`` replays: the arguments of ``tsim_program_create``, ``_add_component`` and
``_add_level`` of a set of programs, as plain binary.  The dump goes to a scratch directory and is never committed.

    python scripts/host_checks/finalize_dump.py OUT/programs.bin [names to leave out ...]

Format (little endian): int32 n_programs; per program: blob name, int32 num_outputs, num_detectors, blobs direct_f (int32),
direct_flips (uint8), output_order (int32), int32 n_components; per component: int32 n_levels, blobs output_indices, f_selection
(int32); per level: int32 G, P, ta, tb, tc, td, has_approx, then the 18 arrays of ``tsim_level_desc`` in the struct's order, a blob
each.  A blob is int64 n_bytes + the bytes; an empty blob is a NULL pointer.
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tsim_amd import backend, synth  # noqa: E402
from tsim_amd.program import from_tsim  # noqa: E402
import test_gpu_fuzz as F  # noqa: E402


def programs():
    for n in ("C2", "C4", "C5"):
        yield n, synth.config_program(n)[0]
    for n in ("20narrow", "w12", "F70", "n24", "2wide", "3narrow", "n9", "F60"):
        yield n, synth.shape_class_program(n)[0]
    yield "kat_h_m", synth.kat_h_m()
    for seed in range(12):
        yield "fuzz%d" % seed, F.random_program(np.random.default_rng(seed))[0]
        r = F.random_physical_program(np.random.default_rng(seed))
        yield "fuzzp%d" % seed, r[0] if isinstance(r, tuple) else r


def blob(f, arr):
    b = np.ascontiguousarray(arr).tobytes()
    f.write(struct.pack("<q", len(b)))
    f.write(b)


def main(out, skip=()):
    progs = [(n, p) for n, p in programs() if n not in skip]
    with open(out, "wb") as f:
        f.write(struct.pack("<i", len(progs)))
        for name, prog in progs:
            prog = from_tsim(prog)
            blob(f, np.frombuffer(name.encode(), np.uint8))
            f.write(struct.pack("<ii", int(prog.num_outputs), int(prog.num_detectors)))
            blob(f, backend._c(prog.direct_f_indices, np.int32))
            blob(f, backend._c(np.asarray(prog.direct_flips).astype(np.uint8), np.uint8))
            blob(f, backend._c(prog.output_order, np.int32))
            f.write(struct.pack("<i", len(prog.components)))
            for comp in prog.components:
                f.write(struct.pack("<i", len(comp.compiled_scalar_graphs)))
                blob(f, backend._c(comp.output_indices, np.int32))
                blob(f, backend._c(comp.f_selection, np.int32))
                for lv in comp.compiled_scalar_graphs:
                    keep = []
                    d = backend._level_desc(lv, keep)  # (keep: the 18 arrays in the struct's order)
                    f.write(struct.pack("<7i", d.num_graphs, d.n_params, d.ta, d.tb, d.tc, d.td, d.has_approx))
                    assert len(keep) == 18
                    for arr in keep:
                        blob(f, arr)
    print(f"{len(progs)} programs -> {out}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
