#!/usr/bin/env python
"""Times tool_access() (codecad_amd/tool_access.py) entry point by entry point, against overhangs() in the same direction and
against the voxel volume alone, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05, and `plates_256` of tools/time_thin_walls.py: a block of
256^3 samples with slots cut into it.  For the directions +z and +x and the tools flat_tool(1), flat_tool(64), ball_tool(8) and
ball_tool(32), over LAUNCHES calls after WARMUP, of=SOLID:
  call               tool_access(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the upload of the profile, the four launches, the read-back, the labelling of the rest ids and the
                     host's gaps between them), `wall_ms` the host clock around the call
  kernels_ms         per entry point (tops, dilate, erode, rest), device events around its launch alone, in calls of their own
                     (STAGE_LAUNCHES after one), median (min-max), and the sum of the medians
  overhangs          in the same run and direction, overhangs(reach_sq=1): the whole call and its three entry points the same
                     way: the yardstick
  voxels             assembly_voxels() alone: what the user already pays
Writes profiles/tool_access_<scene>.json (or under --out) and prints the same.

usage: python tools/time_tool_access.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256]
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
STAGES = ("hu_tool_tops", "hu_tool_dilate", "hu_tool_erode", "hu_tool_rest")
YARDSTICK = ("hu_overhang_first_layer", "hu_overhang_mark", "hu_overhang_columns")
DIRECTIONS = (("+z", 2, True), ("+x", 0, True))


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
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import time_thin_walls
    tool_module = sys.modules["codecad_amd.tool_access"]
    over_module = sys.modules["codecad_amd.overhangs"]
    tools = (("flat_tool(1)", cc.flat_tool(1)), ("flat_tool(64)", cc.flat_tool(64)), ("ball_tool(8)", cc.ball_tool(8)),
             ("ball_tool(32)", cc.ball_tool(32)))

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
        """The library with device events around the entry points of `stages`."""

        def __init__(self, stages):
            self.stages, self.events = stages, []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name not in self.stages:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append(ev._done())
                return rc
            return staged

    def kernel_times(module, stages, call):
        per_stage = [[] for _ in stages]
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib(stages)
            module.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                module.hip_manager = m
            assert len(lib.events) == len(stages)
            if k:
                for ms, ev in zip(per_stage, lib.events):
                    ms.append(ev.elapsed_ms())
        return {"kernels_ms": {s: summary(ms) for s, ms in zip(stages, per_stage)},
                "kernels_sum_ms": sum(statistics.median(ms) for ms in per_stage)}

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": time_thin_walls.plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "of": tool_module.SOLID, "kernels": list(STAGES),
                  "runs": {}, "overhangs": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        for label, axis, up in DIRECTIONS:
            yard = lambda: cc.overhangs(asm, resolution, axis=axis, up=up, reach_sq=1)   # noqa: E731
            entry, _ = timed(yard)
            entry.update(kernel_times(over_module, YARDSTICK, yard))
            result["overhangs"][label] = entry
            for tool_label, tool in tools:
                call = lambda: cc.tool_access(asm, resolution, axis=axis, up=up, tool=tool)   # noqa: E731
                entry, report = timed(call)
                entry.update(kernel_times(tool_module, STAGES, call))
                nu, nv = report.tops.shape
                taps = len([1 for du in range(-tool.reach, tool.reach + 1) for dv in range(-tool.reach, tool.reach + 1)
                            if du * du + dv * dv <= tool.radius_sq])
                entry.update({"columns": nu * nv, "taps": taps, "undercut_samples": sum(report.undercut_counts),
                              "tight_samples": sum(report.tight_counts), "pockets": len(report.pockets),
                              "highest_cut": int(report.cut.max()), "cut_not_below_tops": bool((report.cut >= report.tops).all()),
                              "span_over_overhangs": entry["span_ms"]["median_ms"] / result["overhangs"][label]["span_ms"]["median_ms"],
                              "kernels_over_overhangs": entry["kernels_sum_ms"] / result["overhangs"][label]["kernels_sum_ms"],
                              "same_part_ids": bool(numpy.array_equal(report.part_ids, voxels.part_ids))})
                result["runs"]["%s %s" % (label, tool_label)] = entry
        with open(os.path.join(args.out, "tool_access_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
