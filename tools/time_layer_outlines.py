#!/usr/bin/env python
"""Times a stack of outlines (codecad_amd/layer_outlines.py) against the host loop over its layers, on the device.

Scenes: the gear train of tests/test_gpu_interference.py and the grid of 64 solids of tests/test_gpu_assembly_picture.py, each
on the xz plane through its centre at the resolution that gives --samples (1024) samples along the longer side, with --layers
(200) layers from layer_heights().  Over LAUNCHES calls after WARMUP:
  layers_cull / layers_no_cull   layer_outlines() with cull True / False
  loop                           section_outlines() on planes[l], one call per layer: the only way before layer_outlines()
`span_ms` is the device-event time from before a call's first enqueue to after its last (uploads, every level, the read-back
and the host's gaps between them), `wall_ms` the host clock around the call (with the sort; the loop's with its stitching).
Also: the evaluations, the segments, the top rows and the bytes of records read back.
Writes profiles/layer_outlines_<scene>.json (or under --out) and prints the same.

usage: python tools/time_layer_outlines.py [--out DIR] [--launches 20] [--warmup 3] [--samples 1024] [--layers 200]
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
    ap_.add_argument("--layers", type=int, default=200)
    args = ap_.parse_args()

    import numpy
    import codecad_amd as cc
    from codecad_amd import hip_util, _instance_cells as cells
    from codecad_amd.section import Plane
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import test_gpu_assembly_picture
    lo = sys.modules["codecad_amd.layer_outlines"]       # (the package's attribute of that name is the function)

    # the bytes of record buffers read back: every Buffer of (capacity, 4) uint32 a call reads
    read_back = [0]
    plain_read = hip_util.Buffer.read

    def counting_read(self, *a, **kw):
        if self.dtype == numpy.uint32 and len(self.shape) == 2 and self.shape[1] == 4:
            read_back[0] += self.size
        return plain_read(self, *a, **kw)
    hip_util.Buffer.read = counting_read

    scenes = {"gear_train": test_gpu_interference._gear_train(), "grid_64": test_gpu_assembly_picture._grid(64)}
    os.makedirs(args.out, exist_ok=True)
    for name, asm in scenes.items():
        box = asm.shape().bounding_box()
        plane = Plane.xz((box.a.y + box.b.y) / 2)
        resolution = max(box.size().x, box.size().z) / args.samples
        heights = cc.layer_heights(asm, plane, float(box.size().y) / args.layers)[:args.layers]
        planted = lo.seed(cells.visible(asm, resolution), plane, resolution, heights)
        planes = planted.planes
        result = {"scene": name, "resolution": resolution, "layers": len(heights), "device": m.device_name}
        got = {}

        def loop():
            return [cc.section_outlines(asm, p, resolution) for p in planes]

        for key, call in (("layers_cull", lambda: cc.layer_outlines(asm, plane, resolution, heights)),
                          ("layers_no_cull", lambda: cc.layer_outlines(asm, plane, resolution, heights, cull=False)),
                          ("loop", loop)):
            spans, walls = [], []
            for k in range(args.warmup + args.launches):
                read_back[0] = 0
                t0 = time.perf_counter()
                ev = Event(m, m.queue)
                out = call()
                span = ev._done().elapsed_ms()
                if k >= args.warmup:
                    spans.append(span)
                    walls.append((time.perf_counter() - t0) * 1e3)
            got[key] = out
            many = out if isinstance(out, list) else [out]
            result[key] = {"span_ms": summary(spans), "wall_ms": summary(walls), "evaluations": sum(o.evaluations for o in many),
                           "runs": sum(o.runs for o in many), "segments": sum(len(o.segments) for o in many),
                           "record_bytes_read_back": read_back[0]}
        stack = got["layers_cull"]
        same = all(stack.layer(l).segments.tobytes() == o.segments.tobytes() for l, o in enumerate(got["loop"]))
        result.update(dims=list(stack.dims), instances=len(stack.instances), top_rows=int(len(planted.top)),
                      layers_with_segments=int((stack.layer_counts.sum(axis=1) > 0).sum()), same_segments_as_loop=bool(same),
                      same_segments_no_cull=bool(stack.segments.tobytes() == got["layers_no_cull"].segments.tobytes()))
        result["loop_vs_layers_cull_span"] = result["loop"]["span_ms"]["median_ms"] / result["layers_cull"]["span_ms"]["median_ms"]
        result["loop_vs_layers_cull_wall"] = result["loop"]["wall_ms"]["median_ms"] / result["layers_cull"]["wall_ms"]["median_ms"]
        with open(os.path.join(args.out, "layer_outlines_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
