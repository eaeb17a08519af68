"""Times separation() on the gear train and the 64 solids of the tests against clearance() asked for the same number.

    python tools/time_separation.py [--scenes gears solids64] [--reps 20] [--out profiles/separation_SCENE.json]

Per scene two resolutions: the one tools/time_clearance.py uses for the gear train (0.1; the solids' 0.07 of the tests) and
one 16 times finer.  Arms: `separation()`, and the parent commit's only way to the same number, `clearance()` with min_gap =
the assembly's diagonal, at the coarser resolution only (at the finer one it would evaluate 4096 times the samples, minutes a call; it is not
attempted and the record says so).  Every figure is the median (min, max) over --reps calls after three warm-up calls, taken with device
events recorded on the library's stream around the whole call, which ends in its one synchronisation.  Evaluations and
rows per level come from the reports.  Prints one JSON line per scene and writes it to --out (SCENE replaced).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import codecad_amd as cc  # noqa: E402
from codecad_amd import hip_util  # noqa: E402
from codecad_amd.hip_util import manager as hip_manager  # noqa: E402
import assembly_mass_scenes as mass_scenes  # noqa: E402

SCENES = {"gears": (mass_scenes._gear_train, 0.1), "solids64": (lambda: mass_scenes._solids(64), 0.07)}


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        ev = hip_util.Event(hip_manager, hip_manager.queue)
        out = fn()
        ev._done()
        times.append(ev.elapsed_ms())
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for name in args.scenes:
        build, coarse = SCENES[name]
        asm = build()
        box = asm.shape().bounding_box()
        diagonal = float(sum(s * s for s in box.size()) ** 0.5)
        record = {"scene": name, "reps": args.reps, "diagonal": diagonal, "arms": []}
        for resolution in (coarse, coarse / 16):
            times, r = device_ms(lambda: cc.separation(asm, resolution), args.reps)
            record["arms"].append(dict(times, arm="separation", resolution=resolution, dims=[int(d) for d in r.dims],
                                       instances=len(r.instances), samples_evaluated=r.samples_evaluated, level_rows=list(r.level_rows),
                                       traversals=r.traversals))
        times, r = device_ms(lambda: cc.clearance(asm, coarse, diagonal), args.reps)
        record["arms"].append(dict(times, arm="clearance", resolution=coarse, min_gap=diagonal, dims=[int(d) for d in r.dims],
                                   samples_evaluated=r.samples_evaluated, pairs=len(r.pairs)))
        record["arms"].append({"arm": "clearance", "resolution": coarse / 16, "not_timed": "not attempted: 4096 times the samples of the coarser lattice, every one of them evaluated"})
        line = json.dumps(record)
        print(line)
        if args.out:
            with open(args.out.replace("SCENE", name), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
