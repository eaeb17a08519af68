#!/usr/bin/env python
"""Times the surface meshes of an assembly's parts (codecad_amd/assembly_meshes.py) against the only way to one mesh per part
without them: a host loop of rendering.mesh.mesh_arrays(instance.shape()) over the visible instances, on the device.

Scenes: the gear train of tests/test_gpu_interference.py and the 64 solids of tests/assembly_mass_scenes.py, each at the
resolution that gives --samples (256) samples along the longest side of its box.  Over LAUNCHES calls after WARMUP:
  meshes_cull / meshes_no_cull   assembly_meshes() with cull True / False
  mesh_arrays_loop               mesh_arrays(instance.shape()) per visible instance: a subdivision hierarchy, a tape upload and
                                 several synchronisations each, every mesh on a lattice of its own (at its own feature size:
                                 not the same triangles -- what it costs to get one mesh per part today)
`span_ms` is the device-event time from before a call's first enqueue to after its last (uploads, every level, the read-back
and the host's gaps between them), `wall_ms` the host clock around the call (with the sorting, for the meshes).
Writes profiles/assembly_meshes_<scene>.json (or under --out) and prints the same.

usage: python tools/time_assembly_meshes.py [--out DIR] [--launches 20] [--warmup 3] [--samples 256]
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
    ap_.add_argument("--samples", type=int, default=256)
    args = ap_.parse_args()

    import codecad_amd as cc
    from codecad_amd import _instance_cells
    from codecad_amd.rendering import mesh
    from codecad_amd.hip_util import manager as m
    from codecad_amd.hip_util.manager import Event
    import test_gpu_interference
    import assembly_mass_scenes

    scenes = {"gear_train": test_gpu_interference._gear_train(), "solids_64": assembly_mass_scenes._solids(64)}
    os.makedirs(args.out, exist_ok=True)
    for name, asm in scenes.items():
        resolution = max(asm.shape().bounding_box().size()) / args.samples
        shapes = [i.shape() for i in _instance_cells.visible(asm, resolution)]
        result = {"scene": name, "resolution": resolution, "device": m.device_name}
        got = {}

        def loop():
            return [mesh.mesh_arrays(s) for s in shapes]

        for key, call in (("meshes_cull", lambda: cc.assembly_meshes(asm, resolution)),
                          ("meshes_no_cull", lambda: cc.assembly_meshes(asm, resolution, cull=False)),
                          ("mesh_arrays_loop", loop)):
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
            result[key] = {"span_ms": summary(spans), "wall_ms": summary(walls)}
            if key != "mesh_arrays_loop":
                result[key].update(evaluations=out.evaluations, runs=out.runs)
            print("%s: %s timed" % (name, key), file=sys.stderr, flush=True)
        o = got["meshes_cull"]
        result.update(dims=[int(d) for d in o.dims], instances=len(o.instances), triangles=int(len(o.triangles)),
                      same_triangles=bool(o.triangles.tobytes() == got["meshes_no_cull"].triangles.tobytes()),
                      mesh_arrays_triangles=int(sum(x.n_triangles for x in got["mesh_arrays_loop"])))
        result["meshes_cull_vs_mesh_arrays_loop"] = result["meshes_cull"]["span_ms"]["median_ms"] / result["mesh_arrays_loop"]["span_ms"]["median_ms"]
        with open(os.path.join(args.out, "assembly_meshes_%s.json" % name), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
