#!/usr/bin/env python
"""Times overhangs() (codecad_amd/overhangs.py) kernel by kernel, against the voxel volume alone and against the time of
moving the same bytes, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05, and `plates_256` of tools/time_thin_walls.py: a block of
256^3 samples with slots cut into it.  For the directions +z and +x and reach_sq = 1 and 8, over LAUNCHES calls after WARMUP,
of=SOLID:
  call               overhangs(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the three kernels, all read-backs, the labelling of the support ids and the host's gaps between
                     them), `wall_ms` the host clock around the call
  kernels_ms         per entry point (first_layer, mark, columns), device events around its launch alone, in calls of their own
                     (STAGE_LAUNCHES after one), median (min-max), and the sum of the medians
  voxels             assembly_voxels() alone: what the user already pays
  floor              the same bytes moved by the library's own copy and memset: a volume of nx * ny * pz bytes copied once (1
                     byte read and 1 written per sample) and two such volumes set (2 written), which is what the ids in and
                     the three id volumes out come to; the mark and the column pass read further bytes (the taps; the ids
                     and the overhang ids a second time) that the floor does not count
Writes profiles/overhangs_<scene>.json (or under --out) and prints the same.

usage: python tools/time_overhangs.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256]
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
STAGES = ("hu_overhang_first_layer", "hu_overhang_mark", "hu_overhang_columns")
DIRECTIONS = (("+z", 2, True), ("+x", 0, True))
REACHES = (1, 8)


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
    over = sys.modules["codecad_amd.overhangs"]
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
        """The library with device events around every new entry point."""

        def __init__(self):
            self.events = []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name not in STAGES:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append(ev._done())
                return rc
            return staged

    def kernel_times(call):
        per_stage = [[] for _ in STAGES]
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib()
            over.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                over.hip_manager = m
            assert len(lib.events) == len(STAGES)
            if k:
                for ms, ev in zip(per_stage, lib.events):
                    ms.append(ev.elapsed_ms())
        return per_stage

    def floor(dims):
        """One volume copied and two set, by the library: 1 byte read and 3 written per sample."""
        shape = voxel_module.volume_shape(dims, 2 ** 40)
        a, b, c, d = (hip_util.Buffer(numpy.uint8, shape, queue=m.queue) for _ in range(4))
        ms = []
        for k in range(args.warmup + args.launches):
            ev = Event(m, m.queue)
            check(m.lib.hu_memcpy_d2d(b.device_ptr, a.device_ptr, a.size, m.queue.handle), "hu_memcpy_d2d")
            check(m.lib.hu_memset(c.device_ptr, 255, c.size, m.queue.handle), "hu_memset")
            check(m.lib.hu_memset(d.device_ptr, 255, d.size, m.queue.handle), "hu_memset")
            span = ev._done().elapsed_ms()
            if k >= args.warmup:
                ms.append(span)
        for buffer in (a, b, c, d):
            buffer.release()
        return dict(summary(ms), bytes=4 * int(numpy.prod(shape)))

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": time_thin_walls.plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "of": over.SOLID, "kernels": list(STAGES), "runs": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        result["floor"] = floor(voxels.dims)
        for label, axis, up in DIRECTIONS:
            for reach_sq in REACHES:
                call = lambda: cc.overhangs(asm, resolution, axis=axis, up=up, reach_sq=reach_sq)   # noqa: E731
                entry, report = timed(call)
                stages = kernel_times(call)
                entry["kernels_ms"] = {s: summary(ms) for s, ms in zip(STAGES, stages)}
                entry["kernels_sum_ms"] = sum(statistics.median(ms) for ms in stages)
                entry["kernels_over_floor"] = entry["kernels_sum_ms"] / result["floor"]["median_ms"]
                entry["span_over_voxels"] = entry["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
                entry.update({"first_layer": report.first_layer, "overhang_samples": sum(report.overhang_counts),
                              "support_samples": sum(report.support_counts), "landing_samples": sum(report.landing_counts),
                              "plate_landings": report.plate_landings, "supports": len(report.supports),
                              "invariant_holds": sum(report.overhang_counts) == sum(report.landing_counts) + report.plate_landings,
                              "same_part_ids": bool(numpy.array_equal(report.part_ids, voxels.part_ids))})
                result["runs"]["%s reach_sq=%d" % (label, reach_sq)] = entry
        with open(os.path.join(args.out, "overhangs_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
