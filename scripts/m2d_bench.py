"""Throughput of the measurements -> detection events kernel (tsim_m2d_convert_device) on resident device buffers.

For rotated_surface_code_memory(d, d), d = 5 and 11, B shots of random measurement rows (dense rows: ceil(M/8) bytes
bit-packed or M bytes unpacked) convert to dense detector + observable rows (packed or unpacked, same as the input).
Reports the wall time of a call up to its completion (median of --reps; kernel times: run under
`rocprofv3 --kernel-trace --stats`), shots/s and the bytes/s the shapes imply: bytes per
shot = input row + output row (d = 5 bit-packed: 19 + 16 B; d = 11: 181 + 166 B).  One JSON line per case.

    python scripts/m2d_bench.py [--shots 10000000] [--reps 5]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tsim_amd import backend, circuits, synth  # noqa: E402
from tsim_amd.clifford import CliffordCircuit  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distances", type=int, nargs="*", default=[5, 11])
    args = ap.parse_args()
    hp = backend.HipProgram(synth.kat_h_m(), device=0)  # device buffers and the stream the conversions run on
    stream = hp.stream_ptr()
    B = args.shots
    rng = np.random.default_rng(1)
    for d in args.distances:
        conv = CliffordCircuit(circuits.rotated_surface_code_memory(d, d)).compile_m2d_converter()
        M, n_out = conv.num_measurements, conv.num_detectors + conv.num_observables
        for packed in (True, False):
            in_rb = (M + 7) // 8 if packed else M
            out_rb = (n_out + 7) // 8 if packed else n_out
            d_in, d_out = hp.malloc(B * in_rb), hp.malloc(B * out_rb)
            block = rng.integers(0, 256 if packed else 2, (1 << 16, in_rb)).astype(np.uint8)
            for r0 in range(0, B, len(block)):
                hp.h2d(d_in.ptr + r0 * in_rb, block[: min(len(block), B - r0)])

            def run():
                conv.convert_device(d_in.ptr, B, d_out.ptr, in_row_bytes=in_rb, in_packed=packed, out_row_bytes=out_rb,
                                    out_packed=packed, stream=stream)

            run()
            hp.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run()
                hp.synchronize()
                times.append(time.perf_counter() - t0)
            t = sorted(times)[len(times) // 2]
            per_shot = in_rb + out_rb
            print(json.dumps(dict(distance=d, packed=packed, shots=B, num_measurements=M, outputs=n_out,
                                  bytes_per_shot=per_shot, call_ms=round(t * 1e3, 3), shots_per_s=float(f"{B / t:.4g}"),
                                  bytes_per_s=float(f"{B * per_shot / t:.4g}"), hbm_fraction_of_6p3TBs=round(B * per_shot / t / 6.3e12, 3))),
                  flush=True)
            d_in.free()
            d_out.free()
        conv.close()
    hp.close()


if __name__ == "__main__":
    main()
