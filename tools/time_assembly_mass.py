#!/usr/bin/env python
"""Times the mass properties of an assembly (codecad_amd/assembly_mass.py) with and without retirement, and against the dense
definition, on the device.

Scenes: the gear train of tests/test_gpu_interference.py at 0.05 and the grid of 64 solids of tests/test_gpu_assembly_picture.py
at 1/256 of its longest side.  Over LAUNCHES calls after WARMUP:
  retire / descend   assembly_mass_properties() with retire True / False: `span_ms` is the device-event time from before its
                     first enqueue to after its last (uploads, every level, the read-back, and the host's gaps between them),
                     `wall_ms` the host clock around the call; `samples_evaluated`, and the rows every level listed
  dense              grid_eval of EVERY instance over the whole lattice through the interpreter, the dense definition: the sum
                     of the kernels' device-event times (it computes no sums: what it costs before any reduction)
Writes profiles/assembly_mass_<scene>.json (or under --out) and prints the same.  The device keeps no counter of retired
samples per level; the files hold the rows that survived each level and the evaluations of both arms instead.

usage: python tools/time_assembly_mass.py [--out DIR] [--launches 20] [--warmup 3] [--scenes gear_train,grid_64]
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
    from codecad_amd import hip_util, nodes
    from codecad_amd import _instance_cells as cells
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import test_gpu_assembly_picture

    listed = []
    run = cells._run

    def recording_run(*a, **k):
        counts, evaluations, acc = run(*a, **k)
        listed.append(counts)
        return counts, evaluations, acc

    cells._run = recording_run
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
        reports = {}
        for key, retire in (("retire", True), ("descend", False)):
            spans, walls = [], []
            for k in range(args.warmup + args.launches):
                t0 = time.perf_counter()
                ev = Event(m, m.queue)
                report = cc.assembly_mass_properties(asm, resolution, retire=retire)
                span = ev._done().elapsed_ms()
                if k >= args.warmup:
                    spans.append(span)
                    walls.append((time.perf_counter() - t0) * 1e3)
            reports[key] = report
            result[key] = {"span_ms": summary(spans), "wall_ms": summary(walls), "samples_evaluated": report.samples_evaluated,
                           "traversals": report.traversals, "rows_listed_per_level": listed[-1],
                           "evaluated_share": report.samples_evaluated / (samples * n)}
        result["same_sums"] = bool(all(a.sums == b.sums and a.owned_sums == b.owned_sums and a.index_box == b.index_box
                                       for a, b in zip(reports["retire"].parts, reports["descend"].parts)))
        result["total_mass"] = reports["retire"].total_mass
        out = hip_util.Buffer(numpy.float32, (samples, 4))
        tapes = [hip_util.Tape(nodes.make_program(i.shape())) for i in instances]
        shape = tuple(int(d) for d in dims)
        totals = []
        for k in range(args.warmup + args.launches):
            total = sum(m.k.grid_eval(shape, None, tape, corner, step, out).elapsed_ms() for tape in tapes)
            if k >= args.warmup:
                totals.append(total)
        out.release()
        result["dense"] = summary(totals)
        result["retire_vs_descend"] = result["retire"]["span_ms"]["median_ms"] / result["descend"]["span_ms"]["median_ms"]
        result["retire_vs_dense"] = result["retire"]["span_ms"]["median_ms"] / result["dense"]["median_ms"]
        with open(os.path.join(args.out, "assembly_mass_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
