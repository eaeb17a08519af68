#!/usr/bin/env python
"""Times drainage() (codecad_amd/drainage.py) entry point by entry point, against the labelling of empty space it is a cut-down
of and against the time of copying one volume, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05, and `plates_256` of tools/time_thin_walls.py: a block of
256^3 samples with slots cut into it.  For the directions +z, -z and +x, over LAUNCHES calls after WARMUP:
  call               drainage(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the stages below, the word read back per pass, all read-backs, the labelling of the pools and the
                     host's gaps between them), `wall_ms` the host clock around the call
  kernels_ms         per entry point (hu_drain_layers, the hu_components_flatten after it, hu_drain_seed, hu_drain_rise summed
                     over the passes of a call, hu_drain_floor), device events around its launch alone, in calls of their own
                     (STAGE_LAUNCHES after one), median (min-max); `rise_pass_ms` is the same per single pass
  layers_not_local   hu_drain_layers with local=False, the comparison arm of stage 1, measured the same way
  passes             what the report says
  voxels             assembly_voxels() alone: what the user already pays
  labelling          the three labelling launches of assembly_components(of=EMPTY_SPACE), hu_components_local, _merge and
                     _flatten, events around each in calls of their own: stage 1 is a cut-down of them
  copy               one volume of nx * ny * pz bytes copied by the library: 1 byte read and 1 written per sample
Writes profiles/drainage_<scene>.json (or under --out) and prints the same.

usage: python tools/time_drainage.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256]
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
STAGES = ("hu_drain_layers", "hu_components_flatten", "hu_drain_seed", "hu_drain_rise", "hu_drain_floor")
LABELLING = ("hu_components_local", "hu_components_merge", "hu_components_flatten")
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
    from codecad_amd import hip_util
    from codecad_amd.hip_util import manager as m, check
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import time_thin_walls
    drain = sys.modules["codecad_amd.drainage"]
    comp = sys.modules["codecad_amd.assembly_components"]
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
        """The library with device events around the entry points of `names`."""

        def __init__(self, names):
            self.names, self.events = names, []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name not in self.names:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append((name, ev._done()))
                return rc
            return staged

    def stage_times(module, names, call):
        """{entry point: [ms summed over a call's launches of it]} and [ms of every single hu_drain_rise], over calls of their own."""
        per_stage, passes = {s: [] for s in names}, []
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib(names)
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

    def copy(dims):
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
        return dict(summary(ms), bytes=2 * int(numpy.prod(shape)))

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": time_thin_walls.plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "kernels": list(STAGES), "runs": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        result["copy"] = copy(voxels.dims)
        labelling, _ = stage_times(comp, LABELLING, lambda: cc.assembly_components(asm, resolution, of=comp.EMPTY_SPACE))
        result["labelling"] = {s: summary(ms) for s, ms in labelling.items()}
        result["labelling_sum_ms"] = sum(statistics.median(ms) for ms in labelling.values())
        for label, axis, up in DIRECTIONS:
            call = lambda local=True: cc.drainage(asm, resolution, axis=axis, up=up, local=local)   # noqa: E731
            entry, report = timed(call)
            stages, passes = stage_times(drain, STAGES, call)
            other, _ = stage_times(drain, STAGES, lambda: call(False))
            entry["kernels_ms"] = {s: summary(ms) for s, ms in stages.items()}
            entry["kernels_sum_ms"] = sum(statistics.median(ms) for ms in stages.values())
            entry["rise_pass_ms"] = summary(passes)
            entry["layers_not_local"] = summary(other["hu_drain_layers"])
            entry["local_over_not_local"] = statistics.median(stages["hu_drain_layers"]) / statistics.median(other["hu_drain_layers"])
            entry["layers_over_labelling"] = (statistics.median(stages["hu_drain_layers"]) + statistics.median(stages["hu_components_flatten"])) \
                / result["labelling_sum_ms"]
            entry["kernels_over_copy"] = entry["kernels_sum_ms"] / result["copy"]["median_ms"]
            entry["span_over_voxels"] = entry["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
            not_local = cc.drainage(asm, resolution, axis=axis, up=up, local=False)
            entry.update({"passes": report.passes, "trapped_samples": sum(report.trapped_counts), "pools": len(report.pools),
                          "same_part_ids": bool(numpy.array_equal(report.part_ids, voxels.part_ids)),
                          "same_bytes_not_local": bool(numpy.array_equal(report.trapped_ids, not_local.trapped_ids)
                                                       and numpy.array_equal(report.labels, not_local.labels))})
            result["runs"][label] = entry
        with open(os.path.join(args.out, "drainage_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
