"""The sampler's device route without a GPU: every call it makes, recorded.

``tsim_amd/sampler.py`` reaches the device through ``HipProgram`` methods and a handful of names it imports from the
backend.  ``RecordingHip`` stands in for the handle and logs every call with its arguments (arrays as shape, dtype and a
short hash; device buffers as their address - ``malloc`` hands out ``k << 40``), ``patched()`` swaps the imported names
(and the writer and the sink of ``sample_write()``, which would open a codec on the device).
The route then runs on the CPU and its log says which kernels, copies and waits a request costs, in which order, on
which addresses - what a refactor of the route must not change.

    python scripts/host_checks/route_trace.py                 # one block of lines per case
    python scripts/host_checks/route_trace.py --only NAME     # one case
    python scripts/host_checks/route_trace.py --write-golden  # tests/golden/sampler_route_traces.json

``tests/test_sampler_route_trace.py`` holds the tree to the committed file.
"""

from __future__ import annotations

import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tsim_amd.sampler as S  # noqa: E402
from tsim_amd import shotdata  # noqa: E402
from tsim_amd.backend import HipProgram  # noqa: E402
from tsim_amd.channels import error_probs  # noqa: E402
from tsim_amd.program import CompiledComponent, make_program, scalar_graphs_from_terms  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_route_traces.json")
_WRITES = {"d2h": 0, "d2h_async": 0}  # methods whose array argument is a destination: its contents say nothing


class _Buf:
    def __init__(self, hp, ptr: int, nbytes: int):
        self._hp, self.ptr, self.nbytes = hp, ptr, nbytes

    def free(self) -> None:
        self._hp.log.append(f"free(buf@{self.ptr:#x})")


def _show(x, contents: bool = True) -> str:
    if isinstance(x, _Buf):
        return f"buf@{x.ptr:#x}"
    if isinstance(x, np.ndarray):
        digest = hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:10] if contents else "-"
        return f"nd{list(x.shape)}:{x.dtype}:{digest}"
    if isinstance(x, ctypes.Array):
        return _show([int(v) for v in x])
    if isinstance(x, (list, tuple)):
        return "[" + ", ".join(_show(v, contents) for v in x) + "]"
    if isinstance(x, (bool, np.bool_)):
        return str(bool(x))
    if isinstance(x, (int, np.integer)):
        return hex(int(x)) if int(x) >= (1 << 32) else str(int(x))
    if x is None or isinstance(x, (float, str)):
        return repr(x)
    return type(x).__name__


class RecordingHip:
    """A ``HipProgram`` that computes nothing.  Downloads deliver zeros, except the 4-byte read of the survivor queue's
    tail, which delivers the rows appended so far (every row survives a filter that never ran), so that survivor batches
    are dispatched as they would be."""

    PIPELINE_SLOTS = HipProgram.PIPELINE_SLOTS

    def __init__(self):
        self.log: list[str] = []
        self._allocs = self._slot = self._tail = 0

    def _record(self, name: str, args, kw) -> None:
        parts = [_show(a, contents=not (name in _WRITES and i == _WRITES[name])) for i, a in enumerate(args)]
        parts += [f"{k}={_show(v)}" for k, v in sorted(kw.items())]
        self.log.append(f"{name}({', '.join(parts)})")

    def __getattr__(self, name: str):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            self._record(name, args, kw)

        return call

    def malloc(self, nbytes: int) -> _Buf:
        self._allocs += 1
        self._record("malloc", (nbytes,), {})
        return _Buf(self, self._allocs << 40, int(nbytes))

    def mem_info(self):
        self._record("mem_info", (), {})
        return 64 << 30, 128 << 30

    def aux_stream(self, index: int) -> int:
        self._record("aux_stream", (index,), {})
        return 0x5000 + index

    def pipeline_next_slot(self) -> int:
        self._record("pipeline_next_slot", (), {})
        return self._slot

    def sample_steps_noise_device(self, noise, d_f, B, num_f, key_state, noise_key_state, d_out, **kw) -> None:
        self._record("sample_steps_noise_device", (noise, d_f, B, num_f, key_state, noise_key_state, d_out), kw)
        self._slot = (self._slot + len(d_f)) % self.PIPELINE_SLOTS
        for state in (key_state, noise_key_state):  # (the library leaves the chains len(d_f) splits further on)
            state[0] = (state[0] + len(d_f)) & 0xFFFFFFFF

    def survivors_append_device(self, d_gone, n, *rest) -> None:
        self._record("survivors_append_device", (d_gone, n) + rest, {})
        self._tail += n

    def d2h(self, dst, src) -> None:
        self._record("d2h", (dst, src), {})
        dst[...] = self._tail if (dst.nbytes == 4 and dst.dtype == np.uint32) else 0


class _Pool:
    def take(self, shape, dtype=np.uint8):
        return np.zeros(shape, dtype=dtype)


class _Noise:
    def __init__(self, hp, channel_sampler):
        self._prog = hp


class _Writer:
    """``shotdata.ShotWriter`` without a codec: ``sample_write()``'s route is traced up to the sink it builds."""

    def __init__(self, path, fmt, n_cols, sections, device=0):
        self.n_bits = n_cols

    def abort(self) -> None:
        pass


class _FileSink:
    def __init__(self, hp, words, files, lo, hi):
        self._hp = hp
        hp._record("FileSink", (words, [cols for _w, cols in files], lo, hi), {})

    def __call__(self, *args) -> None:
        self._hp._record("sink", args, {})

    def release(self) -> None:
        self._hp._record("FileSink.release", (), {})


@contextlib.contextmanager
def patched(hp: RecordingHip):
    """The sampler module's doors to the device, swapped for the stand-ins.  ``sample_program`` and the name the module
    compares it with get the same stub, so the samplers keep to the device route."""

    def seam(program, f_params, key, **kw):
        f = np.asarray(f_params)
        hp.log.append(f"sample_program({_show(f)}, {_show(key)})")
        n_out = int(program.num_outputs)
        return np.broadcast_to(np.arange(n_out) % 2 == 0, (len(f), n_out)).copy()

    new = dict(sample_program=seam, _backend_sample_program=seam, result_pool=lambda: _Pool(), DeviceNoiseSampler=_Noise,
               alloc_pinned_numpy=lambda nbytes, dtype, shape: np.zeros(shape, dtype=dtype),
               get_hip_program=lambda *a, **kw: hp)
    swaps = [(S, k, v) for k, v in new.items()]
    swaps += [(shotdata, "ShotWriter", _Writer), (shotdata, "FileSink", _FileSink), (shotdata, "close_all", lambda writers: None)]
    old = [(mod, k, getattr(mod, k)) for mod, k, _v in swaps]
    for mod, k, v in swaps:
        setattr(mod, k, v)
    try:
        yield
    finally:
        for mod, k, v in old:
            setattr(mod, k, v)


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------


def _random_bit(output_index: int, f_index: int | None = None) -> CompiledComponent:
    F = 0 if f_index is None else 1
    fsel = np.zeros(0, np.int32) if f_index is None else np.asarray([f_index], np.int32)
    return CompiledComponent((output_index,), fsel, (scalar_graphs_from_terms(F, [dict()]),
                                                     scalar_graphs_from_terms(F + 1, [dict(power2=-1)])))


_NOISE = dict(channel_probs=[error_probs(0.3)], error_transform=np.array([[1]], np.uint8))


def mixed(noise: str):
    """Detector 0 reads the one noisy f bit; detector 1 and the observable are one-output components."""
    prog = make_program([_random_bit(1, f_index=0), _random_bit(2)], [(0, 0, False)], 3, 2)
    return S.CompiledDetectorSampler(prog, seed=7, noise=noise, **_NOISE)


def direct_only():
    """No components: two detectors read the f bit (one flipped), the rows come from ``_direct_device``."""
    prog = make_program([], [(0, 0, False), (1, 0, True)], 2, 2)
    return S.CompiledDetectorSampler(prog, seed=7, noise="host", **_NOISE)


DET, OBS = "use_detector_reference_sample", "use_observable_reference_sample"
MASK = np.array([True, False])
ARRANGEMENTS = {
    "bools": {},
    "packed": dict(bit_packed=True),
    "packed_append": dict(bit_packed=True, append_observables=True),
    "prepend": dict(prepend_observables=True),
    "separate_packed": dict(separate_observables=True, bit_packed=True),
    "det_ref": {DET: True},
    "obs_ref_append": {OBS: True, "append_observables": True},
    "both_refs_packed_append": {DET: True, OBS: True, "bit_packed": True, "append_observables": True},
    "mask": dict(postselection_mask=MASK),
    "mask_det_ref": {"postselection_mask": MASK, DET: True},
    "mask_packed_append": dict(postselection_mask=MASK, bit_packed=True, append_observables=True),
    "mask_packed_both_refs": {"postselection_mask": MASK, "bit_packed": True, DET: True, OBS: True},
}
SHAPES = {  # noise, shots, batch_size
    "host_7x100_exact": ("host", 700, 100),
    "host_650_partial": ("host", 650, 100),
    "host_12_batches": ("host", 1200, 100),
    "device_6x2^20": ("device", 6 << 20, 1 << 20),
    "device_one_batch": ("device", 650, None),
}


def _sink(hp: RecordingHip):
    def sink(*args):
        hp._record("sink", args, {})

    return sink


def cases() -> dict:
    """name -> callable(hp) that builds a sampler, makes one request and returns the sampler."""
    out = {}
    n = (1 << 20) + 5  # rows of a component-free program: two chunks

    def add(name, make, request):
        def run(hp):
            s = make()
            request(s, hp)
            return s

        out[name] = run

    for shape, (noise, shots, bs) in SHAPES.items():
        for arr, kw in ARRANGEMENTS.items():
            add(f"sample/{shape}/{arr}", lambda noise=noise: mixed(noise),
                lambda s, hp, shots=shots, bs=bs, kw=kw: s.sample(shots, batch_size=bs, **kw))
        for ride in (False, True):
            add(f"sink/{shape}/{'ride' if ride else 'plain'}", lambda noise=noise: mixed(noise),
                lambda s, hp, shots=shots, bs=bs, ride=ride: s._device_plain(shots, bs, ride, sink=_sink(hp)))
        add(f"plain_ref/{shape}", lambda noise=noise: mixed(noise),
            lambda s, hp, shots=shots, bs=bs: s._sample_batches(shots, bs, compute_reference=True))
        add(f"plain_ref_packed/{shape}", lambda noise=noise: mixed(noise),
            lambda s, hp, shots=shots, bs=bs: s._device_plain(shots, bs, True, packed_columns=2))
        add(f"plain_ref_full_packed/{shape}", lambda noise=noise: mixed(noise),
            lambda s, hp, shots=shots, bs=bs: s._device_plain(shots, bs, True, packed_columns=3))
    refs = {"plain": {}, "det_ref": {DET: True}, "both_refs": {DET: True, OBS: True}}
    for shape in ("host_7x100_exact", "host_650_partial", "device_one_batch"):
        noise, shots, bs = SHAPES[shape]
        for ref, kw in refs.items():
            add(f"count/{shape}/{ref}", lambda noise=noise: mixed(noise),
                lambda s, hp, shots=shots, bs=bs, kw=kw: s.count(shots, batch_size=bs, **kw))
            add(f"write/{shape}/{ref}", lambda noise=noise: mixed(noise),
                lambda s, hp, shots=shots, bs=bs, kw=kw: s.sample_write(shots, batch_size=bs, filepath="unused.01", append_observables=True, **kw))
        add(f"count/{shape}/mask_det_ref", lambda noise=noise: mixed(noise),
            lambda s, hp, shots=shots, bs=bs: s.count(shots, batch_size=bs, postselection_mask=MASK, **refs["det_ref"]))
    add("count/direct/det_ref", direct_only, lambda s, hp: s.count(n, **refs["det_ref"]))
    add("write/direct/det_ref", direct_only, lambda s, hp: s.sample_write(n, filepath="unused.01", **refs["det_ref"]))
    add("two_requests/host", lambda: mixed("host"),
        lambda s, hp: (s.sample(300, batch_size=100), s.sample(700, batch_size=200, bit_packed=True), s.release()))
    add("two_requests/device", lambda: mixed("device"),
        lambda s, hp: (s.sample(300), s.sample((2 << 20) + 5, batch_size=1 << 20, bit_packed=True), s.release()))
    add("direct/bools", direct_only, lambda s, hp: s._direct_device(n, None))
    add("direct/packed_all", direct_only, lambda s, hp: s._direct_device(n, None, packed_columns=2))
    add("direct/packed_prefix", direct_only, lambda s, hp: s._direct_device(n, None, packed_columns=1))
    add("direct/sink", direct_only, lambda s, hp: s._direct_device(n, None, sink=_sink(hp)))
    return out


def trace(run) -> tuple[list[str], dict]:
    hp = RecordingHip()
    with patched(hp):
        s = run(hp)
    keys = {"key": [int(v) for v in s._key], "noise_key": [int(v) for v in s._noise_key]}
    return hp.log, keys


def summary(log: list[str], keys: dict) -> dict:
    return {"calls": len(log), "names": [line.split("(", 1)[0] for line in log],
            "sha1": hashlib.sha1("\n".join(log).encode()).hexdigest(), **keys}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", help="run the one case of this name")
    ap.add_argument("--write-golden", action="store_true", help=f"write {os.path.relpath(GOLDEN, ROOT)}")
    args = ap.parse_args()
    golden = {}
    for name, run in cases().items():
        if args.only and name != args.only:
            continue
        log, keys = trace(run)
        golden[name] = summary(log, keys)
        print(f"== {name}  calls={len(log)} key={keys['key']} noise_key={keys['noise_key']}")
        for line in log:
            print("   " + line)
    if args.write_golden:
        if args.only:
            ap.error("--write-golden writes every case: not with --only")
        with open(GOLDEN, "w") as fh:  # one case per line
            fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(golden.items())) + "\n}\n")


if __name__ == "__main__":
    main()
