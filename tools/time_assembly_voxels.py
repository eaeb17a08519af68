#!/usr/bin/env python
"""Times the part-id volume of an assembly (codecad_amd/assembly_voxels.py) with and without retirement, and against a host
loop of section() over every lattice plane, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05 and the grid of 64 solids of tests/test_gpu_assembly_picture.py
at 1/256 of its longest side.  Over LAUNCHES calls after WARMUP:
  retire / descend   assembly_voxels() with retire True / False: `span_ms` is the device-event time from before its first
                     enqueue to after its last (the prefill, uploads, every level, both read-backs, and the host's gaps between
                     them), `wall_ms` the host clock around the call; `samples_evaluated`, the rows every level listed and
                     the bytes the retired children filled
  sections           the only way before assembly_voxels(): section() on Plane.xy through every lattice plane, the part_ids
                     stacked into the same volume (-1 -> 255): one upload, one set of lists and one synchronisation per plane
Writes profiles/assembly_voxels_<scene>.json (or under --out) and prints the same.

usage: python tools/time_assembly_voxels.py [--out DIR] [--launches 20] [--warmup 3] [--scenes gear_train,grid_64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy  # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--warmup", type=int, default=3)
    ap_.add_argument("--scenes", default="gear_train,grid_64")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd import _instance_cells as cells
    from codecad_amd.section import Plane
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import test_gpu_assembly_picture

    listed = []
    run = cells._run

    def recording_run(*a, **k):
        counts, evaluations, acc = run(*a, **k)
        listed.append((counts, acc))
        return counts, evaluations, acc

    cells._run = recording_run

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

    grid = test_gpu_assembly_picture._grid(64)
    scenes = {"gear_train": (test_gpu_interference._gear_train(), 0.05),
              "grid_64": (grid, max(grid.shape().bounding_box().size()) / 256)}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]
        instances = cells.visible(asm, resolution)
        corner, step, dims = cells.checked_lattice(instances, resolution)
        n, samples = len(instances), int(numpy.prod(dims))
        result = {"scene": name, "dims": [int(d) for d in dims], "resolution": resolution, "instances": n, "device": m.device_name}
        volumes = {}
        for key, retire in (("retire", True), ("descend", False)):
            result[key], voxels = timed(lambda: cc.assembly_voxels(asm, resolution, retire=retire))
            counts, acc = listed[-1]
            volumes[key] = voxels
            result[key].update({"samples_evaluated": voxels.samples_evaluated, "traversals": voxels.traversals,
                                "rows_listed_per_level": counts, "bytes_filled_by_retirement": int(acc[n]),
                                "volume_bytes": int(dims[0]) * int(dims[1]) * (-(-int(dims[2]) // 16) * 16),
                                "evaluated_share": voxels.samples_evaluated / (samples * n)})

        def stacked():
            out = numpy.empty(tuple(int(d) for d in dims), dtype=numpy.uint8)
            for z in range(int(dims[2])):
                ids = cc.section(asm, Plane.xy(float(corner[2] + step * numpy.float32(z))), resolution).part_ids
                out[:, :, z] = numpy.where(ids < 0, 255, ids).T
            return out

        result["sections"], stack = timed(stacked)
        result["sections"]["planes"] = int(dims[2])
        result["same_volume"] = bool(numpy.array_equal(volumes["retire"].part_ids, volumes["descend"].part_ids)
                                     and numpy.array_equal(volumes["retire"].part_ids, stack)
                                     and volumes["retire"].counts == volumes["descend"].counts)
        result["owned_samples"] = int(sum(volumes["retire"].counts))
        result["retire_vs_descend"] = result["retire"]["span_ms"]["median_ms"] / result["descend"]["span_ms"]["median_ms"]
        result["retire_vs_sections"] = result["retire"]["span_ms"]["median_ms"] / result["sections"]["span_ms"]["median_ms"]
        with open(os.path.join(args.out, "assembly_voxels_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
