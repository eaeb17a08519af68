#!/usr/bin/env python
"""Times the connected components of an assembly's part-id volume (codecad_amd/assembly_components.py) with and without the
LDS stage, and against the voxel volume alone, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05, the grid of 64 solids of tests/test_gpu_assembly_picture.py
at 1/256 of its longest side, and `bubbles_256`: a block of 256^3 samples with 4 x 4 x 4 spherical voids sealed inside it.
Over LAUNCHES calls after WARMUP, of=EMPTY_SPACE:
  local / global     assembly_components() with local True / False: `span_ms` is the device-event time from before its first
                     enqueue to after its last (the voxel stage, every labelling kernel, all read-backs and the host's gaps
                     between them), `wall_ms` the host clock around the call
  voxels             assembly_voxels() alone: what the labelling adds is the difference
  stages_ms          per entry point of csrc/instance_components.hip, device events around its launches alone, in calls of
                     their own (STAGE_LAUNCHES after one), medians
Writes profiles/assembly_components_<scene>.json (or under --out) and prints the same.

usage: python tools/time_assembly_components.py [--out DIR] [--launches 20] [--warmup 3] [--scenes gear_train,grid_64,bubbles_256]
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
STAGES = ("hu_components_local", "hu_components_merge", "hu_components_flatten", "hu_components_stats", "hu_components_finish")


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def bubbles_256():
    import codecad_amd as cc
    from codecad_amd import shapes
    voids = [shapes.sphere(r=0.3).translated(x - 1.5, y - 1.5, z - 1.5) for x in range(4) for y in range(4) for z in range(4)]
    return cc.assembly("bubbles", [(shapes.box(4) - shapes.union(voids)).make_part("block")]), 4 / 256


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--warmup", type=int, default=3)
    ap_.add_argument("--scenes", default="gear_train,grid_64,bubbles_256")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import test_gpu_assembly_picture
    components = sys.modules["codecad_amd.assembly_components"]

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
        """The library with device events around every components entry point."""

        def __init__(self):
            self.events = []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name not in STAGES:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append((name, ev._done()))
                return rc
            return staged

    def stage_times(call):
        per_stage = {name: [] for name in STAGES}
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib()
            components.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                components.hip_manager = m
            if k:
                for name in STAGES:
                    per_stage[name].append(sum(ev.elapsed_ms() for n, ev in lib.events if n == name))
        return {name: statistics.median(ms) for name, ms in per_stage.items()}

    grid = test_gpu_assembly_picture._grid(64)
    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05),
              "grid_64": lambda: (grid, max(grid.shape().bounding_box().size()) / 256),
              "bubbles_256": bubbles_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "of": components.EMPTY_SPACE,
                  "tile": list(components.TILE)}
        reports = {}
        for key, local in (("local", True), ("global", False)):
            result[key], reports[key] = timed(lambda: cc.assembly_components(asm, resolution, local=local))
            result[key]["stages_ms"] = stage_times(lambda: cc.assembly_components(asm, resolution, local=local))
            result[key]["component_capacity_runs"] = reports[key].component_capacity_runs
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        first = reports["local"]
        result.update({"dims": [int(d) for d in first.dims], "instances": len(first.instances),
                       "components": len(first.components),
                       "cavities": sum(1 for c in first.components if not c.touches_border),
                       "samples_in_set": int(sum(c.count for c in first.components)),
                       "same_result": bool(numpy.array_equal(first.labels, reports["global"].labels)
                                           and [c[:6] for c in first.components] == [c[:6] for c in reports["global"].components]
                                           and numpy.array_equal(first.part_ids, voxels.part_ids))})
        for key in ("local", "global"):
            result[key]["labelling_ms"] = sum(result[key]["stages_ms"].values())
            result[key]["span_over_voxels"] = result[key]["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
        result["local_vs_global_span"] = result["local"]["span_ms"]["median_ms"] / result["global"]["span_ms"]["median_ms"]
        result["local_vs_global_labelling"] = result["local"]["labelling_ms"] / result["global"]["labelling_ms"]
        with open(os.path.join(args.out, "assembly_components_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
