#!/usr/bin/env python
"""Times wall_thickness() (codecad_amd/wall_thickness.py) kernel by kernel, with its taps staged in LDS and read from global
memory, and against the voxel volume alone, on the device.

Scenes, both of about 256^3 = 16.8 million samples: `gear_train`, the planetary gear train of tests/test_gpu_interference.py
(eight parts; it is flat, 32 x 32 x 8 units) at 0.08, a lattice of about 396 x 405 x 100, and `bracket_256`, a sheet-like part:
three plates of 3 samples that meet in a corner, 256 samples a side.  For every R2 of --radii
(16 and 256 by default), over LAUNCHES calls after WARMUP, of=SOLID:
  lds / global       wall_thickness() with lds True / False: `span_ms` is the device-event time from before its first enqueue to
                     after its last (the voxel stage, the three passes, the gather, the read-backs and the host's gaps between
                     them), `wall_ms` the host clock around the call
  kernels_ms         per kernel (z, y, x of transform 1, then hu_thickness_local), device events around its launch alone, in
                     calls of their own (STAGE_LAUNCHES after one), medians; `passes_ms` is the sum of the first three
  map                from the result, by replaying on the host what decides a wavefront's exit: the samples of S, those at the
                     cap in depth_sq and in thickness_sq, the tiles of 8 x 8 x 16 with nothing in reach, and the WAVEFRONTS (4 y x
                     16 z of one x of a tile) by how they end: `never_search` (no lane holds a value below top = min(M, cap): the
                     first ballot ends it), `leave_early` (every lane that searches ends at top: a ballot ends it before the
                     ball is walked; where in the walk is not replayed) and `walk_the_ball` (some lane ends below top, so no
                     ballot can end it: it reads every offset of the tile's shrunken ball).  `reads_per_sample`: the reads
                     (LDS or global) of the gather over the samples of S, a lower bound (the wavefronts that walk the ball
                     alone) and an upper bound (those that leave early counted as if they walked it)
  voxels             assembly_voxels() alone: what the user already pays
Writes profiles/wall_thickness_<scene>.json (or under --out) and prints the same.

usage: python tools/time_wall_thickness.py [--out DIR] [--launches 10] [--warmup 2] [--scenes gear_train,bracket_256] [--radii 16,256]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy  # noqa: E402

STAGE_LAUNCHES = 5
STAGES = ("hu_thickness_pass_z", "hu_thickness_pass_axis", "hu_thickness_local")
KERNELS = ("z1", "y1", "x1", "local")
TILE = (8, 8, 16)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def gear_train():
    import test_gpu_interference
    return test_gpu_interference._gear_train(), 0.08


def bracket_256():
    import codecad_amd as cc
    from codecad_amd import shapes
    step = 4 / 256
    t = 3 * step
    plates = [shapes.box(4, 4, t).translated(0, 0, (t - 4) / 2), shapes.box(4, t, 4).translated(0, (t - 4) / 2, 0),
              shapes.box(t, 4, 4).translated((t - 4) / 2, 0, 0)]
    return cc.assembly("bracket", [shapes.union(plates).make_part("bracket")]), step


def ball_offsets(r2):
    k = math.isqrt(r2)
    a = numpy.arange(-k, k + 1)
    return int(((a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2) <= r2).sum())


def map_statistics(report):
    """What the result says about where the gather's time goes (the module's docstring)."""
    depth, L, r2, cap = report.depth_sq, report.thickness_sq, report.radius_sq, report.cap
    K = math.isqrt(r2)
    shape = depth.shape
    tiles = [-(-n // t) for n, t in zip(shape, TILE)]
    padded = numpy.zeros([n * t + 2 * K for n, t in zip(tiles, TILE)], dtype=numpy.uint16)
    padded[K:K + shape[0], K:K + shape[1], K:K + shape[2]] = depth
    # the greatest value in reach of every tile: a running maximum along each axis over the tile and its halo
    reach = padded
    for axis in range(3):
        windows = [numpy.take(reach, range(i * TILE[axis], i * TILE[axis] + TILE[axis] + 2 * K), axis=axis).max(axis=axis) for i in range(tiles[axis])]
        reach = numpy.stack(windows, axis=axis)
    def wavefronts(volume):
        """[tx][ty][tz][x in tile][y half][lanes]: a wavefront's 64 samples of `volume`, zeros beyond the lattice."""
        whole = numpy.zeros([n * t for n, t in zip(tiles, TILE)], dtype=numpy.int64)
        whole[:shape[0], :shape[1], :shape[2]] = volume
        split = whole.reshape(tiles[0], TILE[0], tiles[1], 2, TILE[1] // 2, tiles[2], TILE[2])
        return split.transpose(0, 2, 5, 1, 3, 4, 6).reshape(tiles[0], tiles[1], tiles[2], TILE[0], 2, -1)

    top = numpy.minimum(reach, cap).astype(numpy.int64)[:, :, :, None, None, None]
    own, last = wavefronts(depth), wavefronts(L)
    searches = (own > 0) & (own < top)                         # the lanes that are open at the first ballot
    never = ~searches.any(axis=-1)
    walks = (searches & (last < top)).any(axis=-1)             # a lane that ends below top is never finished
    early = ~never & ~walks
    live = (reach > 0)[:, :, :, None, None]                    # (a tile with nothing in reach leaves before any wavefront starts)
    offsets = numpy.array([ball_offsets(v) for v in range(r2 + 1)])
    ball = offsets[numpy.minimum(numpy.maximum(reach.astype(numpy.int64), 1) - 1, r2)][:, :, :, None, None]
    in_set = int((depth > 0).sum())
    started = int((live & numpy.ones_like(never)).sum())
    return {"samples_in_set": in_set, "depth_at_cap": int((depth == cap).sum()), "thickness_at_cap": int((L == cap).sum()),
            "greatest_value": int(depth.max()), "tiles": int(numpy.prod(tiles)), "tiles_with_nothing_in_reach": int((reach == 0).sum()),
            "greatest_value_in_reach_median": float(numpy.median(reach[reach > 0])) if (reach > 0).any() else 0.0,
            "samples_that_search": int(searches.sum()),
            "wavefronts": {"started": started, "never_search": int((never & live).sum()), "leave_early": int(early.sum()),
                           "walk_the_ball": int(walks.sum())},
            "reads_per_sample": {"lower_bound": 64.0 * float((walks * ball).sum()) / max(in_set, 1),
                                 "upper_bound": 64.0 * float(((walks | early) * ball).sum()) / max(in_set, 1)}}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=10)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--scenes", default="gear_train,bracket_256")
    ap_.add_argument("--radii", default="16,256")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    wall = sys.modules["codecad_amd.wall_thickness"]

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
                ev = Event(m, m.queue)
                rc = real(*a)
                self.events.append(ev._done())
                return rc
            return staged

    def kernel_times(call):
        per_kernel = [[] for _ in KERNELS]
        for k in range(1 + STAGE_LAUNCHES):
            lib = StagedLib()
            wall.hip_manager = types.SimpleNamespace(lib=lib, queue=m.queue)
            try:
                call()
            finally:
                wall.hip_manager = m
            assert len(lib.events) == len(KERNELS)
            if k:
                for ms, ev in zip(per_kernel, lib.events):
                    ms.append(ev.elapsed_ms())
        return [summary(ms) for ms in per_kernel]

    scenes = {"gear_train": gear_train, "bracket_256": bracket_256}
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        asm, resolution = scenes[name]()
        result = {"scene": name, "resolution": resolution, "device": m.device_name, "of": wall.SOLID, "kernels": list(KERNELS), "radii": {}}
        result["voxels"], voxels = timed(lambda: cc.assembly_voxels(asm, resolution))
        result.update({"dims": [int(d) for d in voxels.dims], "instances": len(voxels.instances)})
        for r2 in (int(v) for v in args.radii.split(",")):
            entry, reports = {"radius_sq": r2, "K": math.isqrt(r2)}, {}
            for key, lds in (("lds", True), ("global", False)):
                entry[key], reports[key] = timed(lambda: cc.wall_thickness(asm, resolution, radius_sq=r2, lds=lds))
                kernels = kernel_times(lambda: cc.wall_thickness(asm, resolution, radius_sq=r2, lds=lds))
                entry[key]["kernels_ms"] = dict(zip(KERNELS, kernels))
                entry[key]["passes_ms"] = sum(k["median_ms"] for k in kernels[:3])
                entry[key]["span_over_voxels"] = entry[key]["span_ms"]["median_ms"] / result["voxels"]["span_ms"]["median_ms"]
            first, second = reports["lds"], reports["global"]
            entry.update({"map": map_statistics(first), "min_sq": first.min_sq, "thinnest": first.thinnest,
                          "lds_vs_global_local": entry["lds"]["kernels_ms"]["local"]["median_ms"] / entry["global"]["kernels_ms"]["local"]["median_ms"],
                          "same_result": bool(first.thickness_sq.tobytes() == second.thickness_sq.tobytes()
                                              and first.depth_sq.tobytes() == second.depth_sq.tobytes()
                                              and first[9:14] == second[9:14] and numpy.array_equal(first.part_ids, voxels.part_ids))})
            result["radii"]["R2=%d" % r2] = entry
            print("done", name, r2, json.dumps({k: entry[k]["kernels_ms"]["local"]["median_ms"] for k in ("lds", "global")}), flush=True)
        with open(os.path.join(args.out, "wall_thickness_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
