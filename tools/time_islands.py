#!/usr/bin/env python
"""Times islands() (codecad_amd/islands.py) entry point by entry point, and in the same run the stages of drainage(), which
work on the complementary set with the same machinery: the yardstick.  Nothing here is a gate.

Scenes: those of tools/time_drainage.py -- the gear train of tests/test_gpu_interference.py at 0.05, and `plates_256` of
tools/time_thin_walls.py.  For the directions +z, -z and +x, over LAUNCHES calls after WARMUP:
  call               islands(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the stages below, the word read back per pass, all read-backs, the labelling of the islands and the
                     host's gaps between them), `wall_ms` the host clock around the call
  kernels_ms         per entry point (hu_overhang_first_layer, hu_ground_layers, the hu_components_flatten after it,
                     hu_ground_seed, hu_drain_rise summed over the passes of a call, hu_ground_mark), device events around
                     its launch alone, in calls of their own (STAGE_LAUNCHES after one), median (min-max); `rise_pass_ms` is
                     the same per single pass
  layers_not_local   hu_ground_layers with local=False, the comparison arm of stage 1, measured the same way
  drainage_ms        the stages of drainage() in the same direction, measured the same way, and `over_drainage`: layers over
                     hu_drain_layers, seed over hu_drain_seed, rise over rise, hu_ground_mark over hu_drain_floor
  passes             what the report says
Writes profiles/islands_<scene>.json (or under --out) and prints the same.

usage: python tools/time_islands.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256]
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
STAGES = ("hu_overhang_first_layer", "hu_ground_layers", "hu_components_flatten", "hu_ground_seed", "hu_drain_rise", "hu_ground_mark")
DRAIN_STAGES = ("hu_drain_layers", "hu_components_flatten", "hu_drain_seed", "hu_drain_rise", "hu_drain_floor")
COUNTERPARTS = (("hu_ground_layers", "hu_drain_layers"), ("hu_ground_seed", "hu_drain_seed"), ("hu_drain_rise", "hu_drain_rise"),
                ("hu_ground_mark", "hu_drain_floor"))
DIRECTIONS = (("+z", 2, True), ("-z", 2, False), ("+x", 0, True))


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
    ground = sys.modules["codecad_amd.islands"]
    drain = sys.modules["codecad_amd.drainage"]

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
        """The library with device events around the entry points of `names`, up to the labelling that follows the stages."""

        def __init__(self, names, last):
            self.names, self.last, self.events, self.done = names, last, [], False

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name not in self.names or self.done:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append((name, ev._done()))
                self.done = name == self.last                # (the flatten of the labelling afterwards is not a stage)
                return rc
            return staged

    def stage_times(module, names, call):
        """{entry point: [ms summed over a call's launches of it]} and [ms of every single hu_drain_rise], over calls of their own."""
        per_stage, passes = {s: [] for s in names}, []
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib(names, names[-1])
            module.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                module.hip_manager = m
            if k:
                for s in names:
                    per_stage[s].append(sum(ev.elapsed_ms() for name, ev in lib.events if name == s))
                passes += [ev.elapsed_ms() for name, ev in lib.events if name == "hu_drain_rise"]
        return per_stage, passes

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": time_thin_walls.plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "kernels": list(STAGES), "runs": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        for label, axis, up in DIRECTIONS:
            call = lambda local=True: cc.islands(asm, resolution, axis=axis, up=up, local=local)   # noqa: E731
            entry, report = timed(call)
            stages, passes = stage_times(ground, STAGES, call)
            other, _ = stage_times(ground, STAGES, lambda: call(False))
            drained, drain_passes = stage_times(drain, DRAIN_STAGES, lambda: cc.drainage(asm, resolution, axis=axis, up=up))
            entry["kernels_ms"] = {s: summary(ms) for s, ms in stages.items()}
            entry["kernels_sum_ms"] = sum(statistics.median(ms) for ms in stages.values())
            entry["rise_pass_ms"] = summary(passes)
            entry["layers_not_local"] = summary(other["hu_ground_layers"])
            entry["drainage_ms"] = {s: summary(ms) for s, ms in drained.items()}
            entry["drainage_sum_ms"] = sum(statistics.median(ms) for ms in drained.values())
            entry["drainage_rise_pass_ms"] = summary(drain_passes)
            entry["over_drainage"] = {mine: statistics.median(stages[mine]) / statistics.median(drained[theirs]) for mine, theirs in COUNTERPARTS}
            entry["span_over_voxels"] = entry["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
            not_local = cc.islands(asm, resolution, axis=axis, up=up, local=False)
            entry.update({"passes": report.passes, "drainage_passes": len(drain_passes) // STAGE_LAUNCHES, "first_layer": report.first_layer,
                          "floating_samples": sum(report.floating_counts), "start_samples": sum(report.start_counts),
                          "join_samples": sum(report.join_counts), "islands": len(report.islands),
                          "loose": sum(1 for i in report.islands if i.loose),
                          "same_part_ids": bool(numpy.array_equal(report.part_ids, voxels.part_ids)),
                          "same_bytes_not_local": bool(all(numpy.array_equal(getattr(report, f), getattr(not_local, f))
                                                           for f in ("floating_ids", "start_ids", "join_ids", "labels")))})
            result["runs"][label] = entry
        with open(os.path.join(args.out, "islands_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
