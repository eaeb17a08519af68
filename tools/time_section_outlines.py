#!/usr/bin/env python
"""Times the outlines of an assembly's section (codecad_amd/section_outlines.py) against the section itself, on the device.

Scenes: the gear train of tests/test_gpu_interference.py and the grid of 64 solids of tests/test_gpu_assembly_picture.py, each
on the xz plane through its centre at the resolution that gives --samples (1024: the width of tools/time_assembly_picture.py's
image) samples along the longer side.  Over LAUNCHES calls after WARMUP:
  outlines_cull / outlines_no_cull   section_outlines() with cull True / False
  section_cull                       section() of the same scene: what a traversal of this lattice costs
`span_ms` is the device-event time from before a call's first enqueue to after its last (uploads, every level, the read-back
and the host's gaps between them), `wall_ms` the host clock around the call (with the stitching, for the outlines).
Writes profiles/section_outlines_<scene>.json (or under --out) and prints the same.

usage: python tools/time_section_outlines.py [--out DIR] [--launches 20] [--warmup 3] [--samples 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--warmup", type=int, default=3)
    ap_.add_argument("--samples", type=int, default=1024)
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd.section import Plane
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import test_gpu_assembly_picture

    scenes = {"gear_train": test_gpu_interference._gear_train(), "grid_64": test_gpu_assembly_picture._grid(64)}
    os.makedirs(args.out, exist_ok=True)
    for name, asm in scenes.items():
        box = asm.shape().bounding_box()
        plane = Plane.xz((box.a.y + box.b.y) / 2)
        resolution = max(box.size().x, box.size().z) / args.samples
        result = {"scene": name, "resolution": resolution, "device": m.device_name}
        got = {}
        for key, call in (("outlines_cull", lambda: cc.section_outlines(asm, plane, resolution)),
                          ("outlines_no_cull", lambda: cc.section_outlines(asm, plane, resolution, cull=False)),
                          ("section_cull", lambda: cc.section(asm, plane, resolution))):
            spans, walls = [], []
            for k in range(args.warmup + args.launches):
                t0 = time.perf_counter()
                ev = Event(m, m.queue)
                out = call()
                span = ev._done().elapsed_ms()
                if k >= args.warmup:
                    spans.append(span)
                    walls.append((time.perf_counter() - t0) * 1e3)
            got[key] = out
            result[key] = {"span_ms": summary(spans), "wall_ms": summary(walls), "evaluations": out.evaluations, "runs": out.runs}
        o = got["outlines_cull"]
        result.update(dims=list(o.dims), instances=len(o.instances), segments=int(len(o.segments)),
                      loops=sum(len(l) for l in o.loops), open_loops=sum(not l.closed for loops in o.loops for l in loops),
                      same_segments=bool(o.segments.tobytes() == got["outlines_no_cull"].segments.tobytes()))
        result["outlines_cull_vs_section_cull"] = result["outlines_cull"]["span_ms"]["median_ms"] / result["section_cull"]["span_ms"]["median_ms"]
        with open(os.path.join(args.out, "section_outlines_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
