"""Times clearance() on the gear train of tests/test_gpu_clearance.py against interference() and the naive route.

    python tools/time_clearance.py [--resolutions 0.1 0.05] [--min-gap 0.5] [--reps 5] [--out FILE]

Every figure is the median over --reps calls after two warm-up calls, taken with device events recorded on the
library's stream around the call (clearance() and interference() end in their one synchronisation, so the span covers
the whole call).  The naive route is a device grid_eval of every instance over the clearance lattice (events around the
eight launches, the tapes compiled before); the pairing that would follow it is timed separately, on the host over the
read-back distances, and only where --host-pairing-max (samples) allows.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import codecad_amd as cc  # noqa: E402
from codecad_amd import hip_util, nodes  # noqa: E402
from codecad_amd.hip_util import manager as hip_manager  # noqa: E402
from codecad_amd.clearance import half_gap, windows  # noqa: E402
from test_gpu_clearance import _gear_train  # noqa: E402


def device_ms(fn, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        ev = hip_util.Event(hip_manager, hip_manager.queue)
        out = fn()
        ev._done()
        times.append(ev.elapsed_ms())
    return statistics.median(times), out


def naive_eval(tapes, corner, step, dims):
    queue = hip_manager.queue
    c4 = numpy.zeros(4, numpy.float32)
    c4[:3] = corner
    outs = []
    for tape in tapes:
        out = hip_util.Buffer(cc.grid_eval.FLOAT4, tuple(int(d) for d in dims), queue=queue)
        hip_manager.k.grid_eval(tuple(int(d) for d in dims), None, tape, c4, numpy.float32(step), out, queue=queue)
        outs.append(out)
    return outs


def host_pairing(outs, insts, report):
    t = half_gap(report.min_gap)
    wins = windows(insts, report.corner, report.step, report.dims, t)
    near = []
    for out, (lo, hi) in zip(outs, wins):
        w = out.read().view(numpy.float32).reshape(tuple(int(d) for d in report.dims) + (4,))[..., 3]
        inwin = numpy.zeros(w.shape, dtype=bool)
        inwin[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
        near.append((w, inwin & (w < t)))
    pairs = 0
    for i in range(len(near)):
        for j in range(i + 1, len(near)):
            both = near[i][1] & near[j][1]
            if both.any():
                numpy.maximum(near[i][0][both], near[j][0][both]).min()
                pairs += 1
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=float, nargs="+", default=[0.1, 0.05])
    ap.add_argument("--min-gap", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairing-max", type=int, default=20_000_000, help="largest lattice whose host pairing is timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hip_manager.use_device(0)
    asm = _gear_train()
    rows = []
    for res in args.resolutions:
        row = {"resolution": res, "min_gap": args.min_gap}
        row["clearance_ms"], r = device_ms(lambda: cc.clearance(asm, res, args.min_gap), args.reps)
        row["interference_ms"], ri = device_ms(lambda: cc.interference(asm, res), args.reps)
        row["dims"] = [int(d) for d in r.dims]
        row["pairs"] = len(r.pairs)
        row["interference_pairs"] = len(ri.pairs)
        row["evaluated_share"] = r.samples_evaluated / (float(numpy.prod(r.dims)) * len(r.instances))
        row["interference_evaluated_share"] = ri.samples_evaluated / (float(numpy.prod(ri.dims)) * len(ri.instances))
        insts = [i.instance for i in r.instances]
        tapes = [nodes.make_program_buffer(i.shape()) for i in insts]
        row["naive_grid_eval_ms"], outs = device_ms(lambda: naive_eval(tapes, r.corner, r.step, r.dims), args.reps)
        if int(numpy.prod(r.dims)) <= args.host_pairing_max:
            t0 = time.perf_counter()
            host_pairing(outs, insts, r)
            row["naive_host_pairing_ms"] = (time.perf_counter() - t0) * 1e3
        else:
            row["naive_host_pairing_ms"] = "not measured"
        for o in outs:
            o.release()
        rows.append(row)
        print(json.dumps(row), flush=True)
    line = json.dumps({"device": hip_manager.device_name, "gear_train": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
