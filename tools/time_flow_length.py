#!/usr/bin/env python
"""Times flow_length() (codecad_amd/flow_length.py) as a whole and kernel by kernel, and against the voxel volume alone, on the
device.

Scenes, both of about 256^3 = 16.8 million samples: `gear_train`, the planetary gear train of tests/test_gpu_interference.py
(eight parts; it is flat, 32 x 32 x 8 units) at 0.08, a lattice of about 396 x 405 x 100, and `bracket_256`, a sheet-like part:
three plates of 3 samples that meet in a corner, 256 samples a side.  For every case of a scene (a source and a set), over
LAUNCHES calls after WARMUP:
  whole              flow_length(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the seed, every round with the host's read of its word, the statistics and the read-backs),
                     `wall_ms` the host clock around the call
  kernels_ms         per kernel (the seed, a sweep along z, along y, along x, the statistics), device events around its launch
                     alone, in calls of their own (STAGE_LAUNCHES after one): the median over every launch of that kind, and
                     `round_ms`, the sum of the three sweeps' medians
  map                from the result: the rounds, the seeds, the samples of S, those reached, the greatest d
  voxels             assembly_voxels() alone: what the user already pays
Writes profiles/flow_length_<scene>.json (or under --out) and prints the same.

usage: python tools/time_flow_length.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,bracket_256]
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
STAGES = ("hu_geodesic_seed", "hu_geodesic_sweep", "hu_geodesic_stats")
KERNELS = ("seed", "sweep_z", "sweep_y", "sweep_x", "stats")


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def gear_train():
    import codecad_amd as cc
    import test_gpu_interference
    return test_gpu_interference._gear_train(), 0.08, [("plate_solid", cc.Plate(), cc.SOLID), ("border_empty", cc.BORDER, cc.EMPTY_SPACE)]


def bracket_256():
    import codecad_amd as cc
    from codecad_amd import shapes
    step = 4 / 256
    t = 3 * step
    plates = [shapes.box(4, 4, t).translated(0, 0, (t - 4) / 2), shapes.box(4, t, 4).translated(0, (t - 4) / 2, 0),
              shapes.box(t, 4, 4).translated((t - 4) / 2, 0, 0)]
    far = 2 - 1.5 * step                                                   # in the corner of the bottom plate away from the other two
    asm = cc.assembly("bracket", [shapes.union(plates).make_part("bracket")])
    return asm, step, [("gate_solid", cc.Gates([(far, far, -far)]), cc.SOLID), ("plate_x_solid", cc.Plate(0, False), cc.SOLID)]


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=10)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--scenes", default="gear_train,bracket_256")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    flow = sys.modules["codecad_amd.flow_length"]

    def timed(call, launches=args.launches):
        spans, walls, result = [], [], None
        for k in range(args.warmup + launches):
            t0 = time.perf_counter()
            ev = Event(m, m.queue)
            result = call()
            span = ev._done().elapsed_ms()
            if k >= args.warmup:
                spans.append(span)
                walls.append((time.perf_counter() - t0) * 1e3)
        return {"span_ms": summary(spans), "wall_ms": summary(walls)}, result

    class StagedLib:
        """The library with device events around every kernel."""

        def __init__(self):
            self.events = []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name not in STAGES:
                return real

            def staged(*a):
                kind = {"hu_geodesic_seed": "seed", "hu_geodesic_stats": "stats"}.get(name) or "sweep_" + "xyz"[a[5]]
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append((kind, ev._done()))
                return rc
            return staged

    def kernel_times(call):
        per_kernel = {k: [] for k in KERNELS}
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib()
            flow.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                flow.hip_manager = m
            if k:
                for kind, ev in lib.events:
                    per_kernel[kind].append(ev.elapsed_ms())
        return {k: summary(ms) for k, ms in per_kernel.items()}

    scenes = {"gear_train": gear_train, "bracket_256": bracket_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution, cases = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "kernels": list(KERNELS), "cases": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        for case, source, of in cases:
            entry, report = timed(lambda: cc.flow_length(asm, resolution, source, of=of))
            again = cc.flow_length(asm, resolution, source, of=of)
            kernels = kernel_times(lambda: cc.flow_length(asm, resolution, source, of=of))
            entry["kernels_ms"] = kernels
            entry["round_ms"] = sum(kernels[k]["median_ms"] for k in ("sweep_z", "sweep_y", "sweep_x"))
            entry["span_over_voxels"] = entry["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
            reached = report.steps != flow.NONE
            entry["map"] = {"of": str(of), "rounds": report.rounds, "seeds": report.seed_count, "samples_in_set": int(report.in_set().sum()),
                            "reached": int(reached.sum()), "greatest_d": int(report.steps[reached].max()) if reached.any() else None}
            entry["same_result"] = bool(report.steps.tobytes() == again.steps.tobytes() and report.rounds == again.rounds
                                        and numpy.array_equal(report.part_ids, voxels.part_ids))
            result["cases"][case] = entry
            print("done", name, case, json.dumps({"rounds": report.rounds, "span_ms": entry["span_ms"]["median_ms"], "round_ms": entry["round_ms"]}),
                  flush=True)
        with open(os.path.join(args.out, "flow_length_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
