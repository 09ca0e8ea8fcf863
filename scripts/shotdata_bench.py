"""Throughput of the shot-data codec (tsim_shotdata_encode / _decode) and of sample_write against sample(bit_packed=True)
plus ndarray.tofile.

Codec: random rows of the d = 11 surface code's detector width (+ observables) at densities 1e-3 and 0.5, resident in
HBM; kernel-only GB/s = (packed row bytes + format bytes) / time of one call to completion (median of --reps; encode of
r8 / hits / dets includes its 8-byte size read).  End to end (noise="device"): synth.config_program("C2") and
rotated_surface_code_memory(d, d) for d = 5 and 11 at p = 1e-3; sample_write in b8, r8 and dets and sample(bit_packed=True)
+ tofile, alternated in the same call into the same directory (the order rotates per rep), median of --reps (and the
fastest and slowest rep); shots/s, file bytes per shot and bytes per shot that crossed PCIe (the packed rows for sample(), the encoded bytes for sample_write).  One JSON line per case.

    python scripts/shotdata_bench.py [--rows 1000000] [--shots 4000000] [--surface-shots 2000000] [--reps 5] [--dir DIR]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tsim_amd import circuits, shotdata, synth  # noqa: E402
from tsim_amd.channels import error_probs  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402
from tsim_amd.sampler import CompiledDetectorSampler  # noqa: E402


def timed(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def bench_codec(rows: int, reps: int) -> None:
    c = shotdata.codec(0)
    conv = CliffordCircuit(circuits.rotated_surface_code_memory(11, 11)).compile_m2d_converter()
    nd, no = conv.num_detectors, conv.num_observables
    n = nd + no
    used = (n + 7) // 8
    slots = [c.take_slot() for _ in range(3)]
    try:
        for p in (1e-3, 0.5):
            rng = np.random.default_rng(1)
            packed = np.packbits((rng.random((rows, n)) < p).view(np.uint8), axis=1, bitorder="little")
            d_rows = c.staging(slots[0], packed.nbytes, pinned=False)
            c.copy(d_rows, packed.ctypes.data, packed.nbytes)
            c.sync()
            for fmt in shotdata.FORMATS:
                sec = dict(num_detectors=nd, num_observables=no) if fmt == "dets" else {}
                cap = shotdata.encode_rows_device(d_rows, rows, row_bytes=used, n_bits=n, format=fmt, d_out=0, out_capacity=0, **sec)
                d_out = c.staging(slots[1], cap, pinned=False)
                d_dec = c.staging(slots[2], packed.nbytes, pinned=False)

                def enc():
                    shotdata.encode_rows_device(d_rows, rows, row_bytes=used, n_bits=n, format=fmt, d_out=d_out, out_capacity=cap, **sec)
                    c.sync()

                def dec():
                    r = shotdata.decode_bytes_device(d_out, cap, final=True, n_bits=n, format=fmt, d_rows=d_dec, row_bytes=used,
                                                     max_rows=rows, **sec)
                    assert r[0] == rows and r[2] == -1, r

                enc()
                te = statistics.median(timed(enc) for _ in range(reps))
                td = None
                if cap < (1 << 31):  # (one decode call takes a chunk of less than 2 GiB)
                    dec()
                    td = statistics.median(timed(dec) for _ in range(reps))
                moved = packed.nbytes + cap
                print(json.dumps(dict(case="codec", format=fmt, density=p, rows=rows, columns=n, format_bytes_per_row=cap / rows,
                                      encode_gb_per_s=moved / te / 1e9, decode_gb_per_s=moved / td / 1e9 if td else None,
                                      encode_s=te, decode_s=td)), flush=True)
    finally:
        for s in slots:
            c.give_slot(s)


def bench_sampler(name: str, s, shots: int, reps: int, directory: str) -> None:
    path = os.path.join(directory, "shots")
    n_cols = s._num_detectors

    def baseline():
        s.sample(shots, bit_packed=True).tofile(path)

    cases = {"sample_bit_packed_tofile": baseline}
    for fmt in ("b8", "r8", "dets"):
        cases[f"sample_write_{fmt}"] = (lambda f: (lambda: s.sample_write(shots, filepath=path, format=f)))(fmt)
    sizes = {}
    for k, fn in cases.items():  # warm-up, and the file size of each
        fn()
        sizes[k] = os.path.getsize(path)
    times = {k: [] for k in cases}
    keys = list(cases)
    for r in range(reps):  # the order rotates from rep to rep: no case always runs first or after the same neighbour
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            times[k].append(timed(cases[k]))
    base = statistics.median(times["sample_bit_packed_tofile"])
    for k in cases:
        t = statistics.median(times[k])
        pcie = (n_cols + 7) // 8 if k.endswith("tofile") else sizes[k] / shots
        print(json.dumps(dict(case=name, method=k, shots=shots, detectors=n_cols, shots_per_s=shots / t, seconds=t,
                              seconds_min=min(times[k]), seconds_max=max(times[k]),
                              file_bytes_per_shot=sizes[k] / shots, pcie_bytes_per_shot=pcie, vs_baseline=base / t)), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--shots", type=int, default=4_000_000)
    ap.add_argument("--surface-shots", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--skip-codec", action="store_true")
    ap.add_argument("--skip-samplers", action="store_true")
    args = ap.parse_args()
    if not args.skip_codec:
        bench_codec(args.rows, args.reps)
    if args.skip_samplers:
        return
    directory = args.dir or tempfile.mkdtemp(prefix="shotdata_bench_")
    os.makedirs(directory, exist_ok=True)
    prog, cfg = synth.config_program("C2")
    nf = cfg["num_f"]
    s = CompiledDetectorSampler(prog, channel_probs=[error_probs(1e-3)] * nf, error_transform=np.eye(nf, dtype=np.uint8), seed=1,
                                noise="device")
    bench_sampler("C2", s, args.shots, args.reps, directory)
    for d in (5, 11):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            text = circuits.rotated_surface_code_memory(d, d, after_clifford_depolarization=1e-3, before_measure_flip_probability=1e-3)
            s = CliffordCircuit(text).compile_detector_sampler(seed=1, noise="device")
        bench_sampler(f"surface_d{d}", s, args.surface_shots, args.reps, directory)


if __name__ == "__main__":
    main()
