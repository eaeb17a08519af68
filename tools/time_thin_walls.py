#!/usr/bin/env python
"""Times thin_walls() (codecad_amd/thin_walls.py) pass by pass, with its taps staged in LDS and read from global memory, and
against the voxel volume alone, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05, and `plates_256`: a block of 256^3 samples with slots cut
into it that leave plates of 2 to 40 samples.  For K1 = 2, 8 and 32 (radius_sq = K1^2, cover_sq = 3 K1^2), over LAUNCHES calls
after WARMUP, of=SOLID:
  lds / global       thin_walls() with lds True / False: `span_ms` is the device-event time from before its first enqueue to
                     after its last (the voxel stage, the six passes, the labelling of the thin ids, all read-backs and the
                     host's gaps between them), `wall_ms` the host clock around the call
  passes_ms          per pass (z, y, x of transform 1, then of transform 2), device events around its launch alone, in calls
                     of their own (STAGE_LAUNCHES after one), medians, and their sum
  roof_fraction      per pass, the bytes it must move (every sample of the lattice read and written once: 3, 4, 5, 4, 4, 4
                     bytes) over its median time, as a fraction of ROOF_TBPS, the copy rate measured on this device
  voxels             assembly_voxels() alone: what the user already pays
Writes profiles/thin_walls_<scene>.json (or under --out) and prints the same.

usage: python tools/time_thin_walls.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256] [--radii 2,8,32]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy  # noqa: E402

STAGE_LAUNCHES = 5
STAGES = ("hu_thickness_pass_z", "hu_thickness_pass_axis")
PASSES = ("z1", "y1", "x1", "z2", "y2", "x2")
PASS_BYTES = (3, 4, 5, 4, 4, 4)        # per sample: the ids or a uint16 volume in, a uint16 volume or the thin ids out, the ids of a finish
ROOF_TBPS = 6.29                       # a float4 copy on one MI355X; the specification says 8.0


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def plates_256():
    import codecad_amd as cc
    from codecad_amd import shapes
    step = 4 / 256
    slots, at = [], 8
    for wall in (2, 3, 4, 6, 9, 12, 16, 17, 24, 33, 40):         # samples of solid between two slots of 8
        lo = (at - 128) * step
        slots.append(shapes.box(8 * step, 3.5, 3.5).translated(lo + 4 * step, 0, 0.25))
        at += 8 + wall
    return cc.assembly("plates", [(shapes.box(4) - shapes.union(slots)).make_part("block")]), step


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=10)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--scenes", default="gear_train,plates_256")
    ap_.add_argument("--radii", default="2,8,32")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    thin = sys.modules["codecad_amd.thin_walls"]

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
        """The library with device events around every pass."""

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

    def pass_times(call):
        per_pass = [[] for _ in PASSES]
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib()
            thin.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                thin.hip_manager = m
            assert len(lib.events) == len(PASSES)
            if k:
                for ms, ev in zip(per_pass, lib.events):
                    ms.append(ev.elapsed_ms())
        return [statistics.median(ms) for ms in per_pass]

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "of": thin.SOLID, "roof_TBps": ROOF_TBPS,
                  "passes": list(PASSES), "pass_bytes_per_sample": list(PASS_BYTES), "radii": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        samples = int(numpy.prod([int(d) for d in voxels.dims]))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        for k1 in (int(v) for v in args.radii.split(",")):
            radii = {"radius_sq": k1 * k1, "cover_sq": 3 * k1 * k1}
            entry, reports = dict(radii, tiles={"K1": thin.axis_tile(k1, True), "K2": thin.axis_tile(thin.math.isqrt(3 * k1 * k1), True)}), {}
            for key, lds in (("lds", True), ("global", False)):
                entry[key], reports[key] = timed(lambda: cc.thin_walls(asm, resolution, lds=lds, **radii))
                passes = pass_times(lambda: cc.thin_walls(asm, resolution, lds=lds, **radii))
                entry[key]["passes_ms"] = dict(zip(PASSES, passes))
                entry[key]["passes_sum_ms"] = sum(passes)
                entry[key]["roof_fraction"] = {p: b * samples / (ms * 1e-3) / (ROOF_TBPS * 1e12) for p, b, ms in zip(PASSES, PASS_BYTES, passes)}
                entry[key]["span_over_voxels"] = entry[key]["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
            first, second = reports["lds"], reports["global"]
            entry.update({"thin_samples": sum(first.thin_counts), "core_samples": sum(first.core_counts), "regions": len(first.regions),
                          "lds_vs_global_passes": entry["lds"]["passes_sum_ms"] / entry["global"]["passes_sum_ms"],
                          "lds_vs_global_per_pass": {p: entry["lds"]["passes_ms"][p] / entry["global"]["passes_ms"][p] for p in PASSES},
                          "same_result": bool(numpy.array_equal(first.depth_sq, second.depth_sq)
                                              and numpy.array_equal(first.thin_ids, second.thin_ids)
                                              and first.core_counts == second.core_counts and first.thin_counts == second.thin_counts
                                              and [r[:6] for r in first.regions] == [r[:6] for r in second.regions]
                                              and numpy.array_equal(first.part_ids, voxels.part_ids))})
            result["radii"]["K1=%d" % k1] = entry
        with open(os.path.join(args.out, "thin_walls_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
