#!/usr/bin/env python
"""Times disassembly() (codecad_amd/disassembly.py) pass by pass, against the voxel volume alone and against the time of
reading the same bytes, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05, and `plates_256` of tools/time_thin_walls.py: a block of
256^3 samples with slots cut into it.  Over LAUNCHES calls after WARMUP:
  call               disassembly(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the memset of the key table, the three passes, the read-backs), `wall_ms` the host clock around it
  passes_ms          per axis (x, y, z), device events around that launch of hu_blocking_lines alone, in calls of their own
                     (STAGE_LAUNCHES after one), median (min-max), and the sum of the medians
  voxels             assembly_voxels() alone, in the same run: what the user already pays
  floor              one volume of nx * ny * pz bytes copied by the library: a pass must read one byte per sample, the copy
                     reads one and writes one
Writes profiles/disassembly_<scene>.json (or under --out) and prints the same.

usage: python tools/time_disassembly.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy  # noqa: E402

STAGE_LAUNCHES = 5
STAGE = "hu_blocking_lines"
AXES = ("x", "y", "z")
COPY_RATE = 6.29e12             # bytes a second, the measured float4 copy


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=10)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--scenes", default="gear_train,plates_256")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd import hip_util
    from codecad_amd.hip_util import manager as m, check
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import time_thin_walls
    module = sys.modules["codecad_amd.disassembly"]
    voxel_module = sys.modules["codecad_amd.assembly_voxels"]

    def timed(call):
        spans, walls, result = [], [], None
        for k in range(args.warmup + args.launches):
            t0 = time.perf_counter()
            ev = Event(m, m.queue)
            result = call()
            span = ev._done().elapsed_ms()
            if k >= args.warmup:
                spans.append(span)
                walls.append((time.perf_counter() - t0) * 1e3)
        return {"span_ms": summary(spans), "wall_ms": summary(walls)}, result

    class StagedLib:
        """The library with device events around every launch of the new entry point."""

        def __init__(self):
            self.events = []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name != STAGE:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append(ev._done())
                return rc
            return staged

    def pass_times(call):
        per_axis = [[] for _ in AXES]
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib()
            module.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                module.hip_manager = m
            assert len(lib.events) == len(AXES)
            if k:
                for ms, ev in zip(per_axis, lib.events):
                    ms.append(ev.elapsed_ms())
        return per_axis

    def floor(dims):
        """One volume copied by the library: 1 byte read and 1 written per sample."""
        shape = voxel_module.volume_shape(dims, 2 ** 40)
        a, b = (hip_util.Buffer(numpy.uint8, shape, queue=m.queue) for _ in range(2))
        ms = []
        for k in range(args.warmup + args.launches):
            ev = Event(m, m.queue)
            check(m.lib.hu_memcpy_d2d(b.device_ptr, a.device_ptr, a.size, m.queue.handle), "hu_memcpy_d2d")
            span = ev._done().elapsed_ms()
            if k >= args.warmup:
                ms.append(span)
        for buffer in (a, b):
            buffer.release()
        volume = int(numpy.prod(shape))
        return dict(summary(ms), bytes=2 * volume, pass_bytes=volume, pass_at_copy_rate_ms=volume / COPY_RATE * 1e3)

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": time_thin_walls.plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "kernel": STAGE}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        result["floor"] = floor(voxels.dims)
        call = lambda: cc.disassembly(asm, resolution)   # noqa: E731
        result["call"], report = timed(call)
        passes = pass_times(call)
        result["passes_ms"] = {axis: summary(ms) for axis, ms in zip(AXES, passes)}
        result["passes_sum_ms"] = sum(statistics.median(ms) for ms in passes)
        result["pass_over_copy_rate"] = {axis: statistics.median(ms) / result["floor"]["pass_at_copy_rate_ms"] for axis, ms in zip(AXES, passes)}
        result["span_over_voxels"] = result["call"]["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
        sequence, stuck = report.order()
        result.update({"finite_entries": [int((report.distance[a] != module.NEVER).sum()) for a in range(3)],
                       "contacts": [len(report.contacts(a)) for a in range(3)], "order": [list(s) for s in sequence], "stuck": stuck,
                       "same_part_ids": bool(numpy.array_equal(report.part_ids, voxels.part_ids))})
        with open(os.path.join(args.out, "disassembly_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
