#!/usr/bin/env python
"""Times the picture of an assembly (rendering/assembly_picture.py) against the picture of its union, on the device.

For each scene -- the gear train and the grid of 64 solids of tests/test_gpu_assembly_picture.py -- at 1024 x 768,
device-event times over LAUNCHES launches after WARMUP:
  union_interpreter   ray_caster.render(asm.shape()) through the interpreter: the like-for-like baseline
  union_per_tape_code the same with the tape's hipRTC code (for information)
  instances_no_skip   the instance table, every instance at every sample
  instances_skip      ... with skipping, and the share of instance programs it left out
Writes profiles/assembly_picture_<scene>.json (or under --out) and prints the same.

usage: python tools/time_assembly_picture.py [--out DIR] [--launches 20] [--warmup 3] [--no-per-tape]
"""
import argparse
import json
import os
import statistics
import sys

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
    ap_.add_argument("--no-per-tape", action="store_true")
    args = ap_.parse_args()

    from codecad_amd import hip_util, nodes, _instance_cells as cells
    from codecad_amd.hip_util import manager as m
    from codecad_amd.rendering import assembly_picture as ap, ray_caster
    import test_gpu_assembly_picture as scenes

    size = (1024, 768)
    os.makedirs(args.out, exist_ok=True)
    for name in ("gear_train", "grid_64"):
        asm = scenes.SCENES[name]()
        instances, hues, camera, a = ap.scene(asm, size, colors="parts")
        n = len(instances)
        scalars = [numpy.float32(a[k]) for k in ("pixel_tolerance", "box_radius", "min_distance", "max_distance", "floor_z")]
        frame = [a[k].as_float4() for k in ("origin", "forward", "up", "right")]
        out = hip_util.Buffer(numpy.uint8, size + (3,))
        ids = hip_util.Buffer(numpy.int32, size)
        depth = hip_util.Buffer(numpy.float32, size)
        counters = hip_util.Buffer(numpy.uint64, (2,))
        hues4 = numpy.zeros((n, 4), dtype=numpy.float32)
        hues4[:, :3] = hues
        colors = hip_util.Buffer(numpy.float32, hues4.shape)
        colors.enqueue_write(hues4)
        table, distance_only, lane_bytes = cells.device_table(instances, m.queue, full_programs=True)
        program = nodes.make_program(asm.shape())
        result = {"scene": name, "size": list(size), "instances": n, "lane_bytes": lane_bytes, "union_tape_instructions": int(len(program)),
                  "device": m.device_name}

        def timed(launch):
            for _ in range(args.warmup):
                launch().wait()
            return summary([launch().elapsed_ms() for _ in range(args.launches)])

        tape = hip_util.Tape(program)
        result["union_interpreter"] = timed(lambda: m.k.ray_caster(size, None, tape, *frame, *scalars, 0, out))
        union_pixels = out.read().copy()
        for key, flags in (("instances_no_skip", 1), ("instances_skip", 0)):
            result[key] = timed(lambda: m.k.ray_caster_instances(size, None, table, n, distance_only, lane_bytes, *frame, *scalars, 0,
                                                                 colors, out, ids, depth, flags=flags))
            counters.enqueue_fill(0)
            m.k.ray_caster_instances(size, None, table, n, distance_only, lane_bytes, *frame, *scalars, 0, colors, out, ids, depth,
                                     flags=flags, counters=counters).wait()
            run, asked = (int(v) for v in counters.read())
            result[key].update(instance_programs_run=run, instance_programs_asked=asked, skipped_share=1.0 - run / asked)
        if not args.no_per_tape:
            spec = hip_util.Tape(program).specialize()
            result["union_per_tape_code"] = timed(lambda: m.k.ray_caster(size, None, spec, *frame, *scalars, 0, out))
            result["union_per_tape_code"]["same_pixels_as_interpreter"] = bool(numpy.array_equal(out.read(), union_pixels))
        base = result["union_interpreter"]
        result["skip_vs_union_interpreter"] = result["instances_skip"]["median_ms"] / base["median_ms"]
        result["union_interpreter_spread"] = (base["max_ms"] - base["min_ms"]) / base["median_ms"]
        with open(os.path.join(args.out, "assembly_picture_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)
        for b in (out, ids, depth, counters, colors, table):
            b.release()


if __name__ == "__main__":
    main()
