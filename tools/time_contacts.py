#!/usr/bin/env python
"""Times the face kernel of contacts() (codecad_amd/contacts.py) against the three blocking passes of disassembly() and against
the voxel volume alone, in one run on the device.

Scenes: those of tools/time_disassembly.py, the gear train of tests/test_gpu_interference.py at 0.05 and `plates_256` of
tools/time_thin_walls.py.  Over LAUNCHES calls after WARMUP:
  call               contacts(): `span_ms` is the device-event time from before its first enqueue to after its last (the voxel
                     stage, the two memsets, the face kernel, the read-backs, the labelling of the patches), `wall_ms` the host
                     clock around it; `call_no_patches` the same with patches=False
  faces_ms           device events around the launch of hu_contact_faces alone, in calls of their own (STAGE_LAUNCHES after
                     one), median (min-max)
  blocking_ms        the YARDSTICK: per axis (x, y, z), device events around that launch of hu_blocking_lines alone, the same way,
                     and the sum of the medians: the three passes read the same bytes three times, the face kernel reads them
                     once plus its neighbours
  voxels             assembly_voxels() alone: what the user already pays
Writes profiles/contacts_<scene>.json (or under --out) and prints the same.

usage: python tools/time_contacts.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,plates_256]
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
AXES = ("x", "y", "z")


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
    contacts_module, blocking_module = sys.modules["codecad_amd.contacts"], sys.modules["codecad_amd.disassembly"]

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
        """The library with device events around every launch of one entry point."""

        def __init__(self, stage):
            self.stage, self.events = stage, []

        def __getattr__(self, name):
            real = getattr(m.lib, name)
            if name != self.stage:
                return real

            def staged(*a):
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append(ev._done())
                return rc
            return staged

    def stage_times(module, stage, launches, call):
        """[[ms per call] per launch of `stage` in one call of `call`]"""
        per_launch = [[] for _ in range(launches)]
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib(stage)
            module.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                module.hip_manager = m
            assert len(lib.events) == launches
            if k:
                for ms, ev in zip(per_launch, lib.events):
                    ms.append(ev.elapsed_ms())
        return per_launch

    scenes = {"gear_train": lambda: (test_gpu_interference._gear_train(), 0.05), "plates_256": time_thin_walls.plates_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "kernel": "hu_contact_faces",
                  "yardstick": "hu_blocking_lines"}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        result["call"], report = timed(lambda: cc.contacts(asm, resolution))
        result["call_no_patches"], bare = timed(lambda: cc.contacts(asm, resolution, patches=False))
        (faces,) = stage_times(contacts_module, "hu_contact_faces", 1, lambda: cc.contacts(asm, resolution, patches=False))
        passes = stage_times(blocking_module, "hu_blocking_lines", 3, lambda: cc.disassembly(asm, resolution))
        result["faces_ms"] = summary(faces)
        result["blocking_ms"] = {axis: summary(ms) for axis, ms in zip(AXES, passes)}
        result["blocking_sum_ms"] = sum(statistics.median(ms) for ms in passes)
        result["faces_over_blocking_sum"] = statistics.median(faces) / result["blocking_sum_ms"]
        result["span_over_voxels"] = result["call"]["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
        blocking = cc.disassembly(asm, resolution)
        result.update({"pairs": [list(p) for p in report.pairs()], "faces": [int(report.faces[a].astype(object).sum()) for a in range(3)],
                       "patches": len(report.patches), "interface_samples": sum(report.contact_counts),
                       "loose": report.loose(), "same_part_ids": bool(numpy.array_equal(report.part_ids, voxels.part_ids)),
                       "same_tables_without_patches": bool(report.faces.tobytes() == bare.faces.tobytes()
                                                           and report.witness.tobytes() == bare.witness.tobytes()),
                       "faces_iff_distance_one": bool(numpy.array_equal(report.faces > 0, blocking.distance == 1))})
        with open(os.path.join(args.out, "contacts_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
