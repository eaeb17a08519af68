#!/usr/bin/env python
"""Times the section of an assembly (codecad_amd/section.py) against evaluating its union on the same samples, on the device.

Scenes: the gear train of tests/test_gpu_interference.py on its xy mid-plane, and the grid of 64 solids of
tests/test_gpu_assembly_picture.py on its xy mid-plane (which meets one row of eight solids) and on the xz plane through all
64, each at the resolution that gives 2048 samples along the longer side.  Over LAUNCHES calls after WARMUP:
  union_interpreter     grid_eval of asm.shape() over the same (w, h, 1) samples through the interpreter: what looking at that
                        plane costs without section(); the kernel's device-event time
  union_per_tape_code   the same with the tape's hipRTC code (for information)
  section_*             section() with cull False / True, without and with distance: `span_ms` is the device-event time from
                        before its first enqueue to after its last (uploads, every level, the read-back, and the host's gaps
                        between them), `wall_ms` the host clock around the call; and the share of instance evaluations culled
Writes profiles/section_<scene>.json (or under --out) and prints the same.

usage: python tools/time_section.py [--out DIR] [--launches 20] [--warmup 3] [--samples 2048] [--no-per-tape]
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
    ap_.add_argument("--samples", type=int, default=2048)
    ap_.add_argument("--no-per-tape", action="store_true")
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd import hip_util, nodes
    from codecad_amd.section import Plane, lattice
    from codecad_amd import _instance_cells as cells
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import test_gpu_assembly_picture

    def mid(asm, axis):
        box = asm.shape().bounding_box()
        return (box.a[axis] + box.b[axis]) / 2

    gears, grid = test_gpu_interference._gear_train(), test_gpu_assembly_picture._grid(64)
    scenes = {"gear_train": (gears, Plane.xy(mid(gears, 2)), (0, 1)), "grid_64_xy": (grid, Plane.xy(mid(grid, 2)), (0, 1)),
              "grid_64_xz": (grid, Plane.xz(mid(grid, 1)), (0, 2))}
    os.makedirs(args.out, exist_ok=True)
    for name, (asm, plane, axes) in scenes.items():
        box = asm.shape().bounding_box()
        resolution = max(box.size()[k] for k in axes) / args.samples
        instances = cells.visible(asm, resolution)
        corner, step, dims, _, _ = lattice(instances, plane, resolution)
        n, samples = len(instances), int(dims[0]) * int(dims[1])
        program = nodes.make_program(asm.shape())
        result = {"scene": name, "dims": [int(d) for d in dims], "resolution": resolution, "instances": n,
                  "union_tape_instructions": int(len(program)), "device": m.device_name}
        grid_dims = [1, 1, 1]
        grid_dims[axes[0]], grid_dims[axes[1]] = int(dims[0]), int(dims[1])
        out = hip_util.Buffer(numpy.float32, (samples, 4))

        def timed(launch):
            for _ in range(args.warmup):
                launch().wait()
            return summary([launch().elapsed_ms() for _ in range(args.launches)])

        tape = hip_util.Tape(program)
        result["union_interpreter"] = timed(lambda: m.k.grid_eval(tuple(grid_dims), None, tape, corner, step, out))
        union = out.read().copy()
        if not args.no_per_tape:
            spec = hip_util.Tape(program).specialize()
            result["union_per_tape_code"] = timed(lambda: m.k.grid_eval(tuple(grid_dims), None, spec, corner, step, out))
            result["union_per_tape_code"]["same_values_as_interpreter"] = bool(numpy.array_equal(out.read(), union))
        out.release()
        cuts = {}
        for key, kwargs in (("section_no_cull", {"cull": False}), ("section_cull", {}),
                            ("section_no_cull_distance", {"cull": False, "distance": True}), ("section_cull_distance", {"distance": True})):
            spans, walls = [], []
            for k in range(args.warmup + args.launches):
                t0 = time.perf_counter()
                ev = Event(m, m.queue)
                cut = cc.section(asm, plane, resolution, **kwargs)
                span = ev._done().elapsed_ms()
                if k >= args.warmup:
                    spans.append(span)
                    walls.append((time.perf_counter() - t0) * 1e3)
            cuts[key] = cut
            result[key] = {"span_ms": summary(spans), "wall_ms": summary(walls), "evaluations": cut.evaluations, "runs": cut.runs,
                           "culled_share": 1.0 - cut.evaluations / (samples * n)}
        # the arms computed the same thing, and the union's distance is the section's
        result["same_maps"] = bool(all(numpy.array_equal(cuts["section_cull"].part_ids, c.part_ids) and
                                       numpy.array_equal(cuts["section_cull"].inside_count, c.inside_count) for c in cuts.values()) and
                                   numpy.array_equal(cuts["section_cull_distance"].distance, cuts["section_no_cull_distance"].distance) and
                                   numpy.array_equal(cuts["section_cull_distance"].nearest, cuts["section_no_cull_distance"].nearest))
        w = union[:, 3].reshape(grid_dims[axes[0]], grid_dims[axes[1]]).T
        result["distance_equals_union"] = float((cuts["section_cull_distance"].distance == w).mean())
        base = result["union_interpreter"]
        result["cull_vs_union_interpreter"] = result["section_cull"]["span_ms"]["median_ms"] / base["median_ms"]
        result["cull_distance_vs_union_interpreter"] = result["section_cull_distance"]["span_ms"]["median_ms"] / base["median_ms"]
        result["union_interpreter_spread"] = (base["max_ms"] - base["min_ms"]) / base["median_ms"]
        with open(os.path.join(args.out, "section_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
