"""clearance() on the device against the dense definition: every instance evaluated by the oracle over the report's
lattice, the windows, near = in both windows and w < t (strictly) for both, v = max(w_i, w_j), in numpy.  Counts, index
sums, index boxes, the float32 bits of the separation and the witness must match bit for bit."""
import math
import random

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, nodes
from codecad_amd.clearance import half_gap, windows
import oracle
import random_trees

pytestmark = pytest.mark.gpu


def dense_near(report):
    """{(i, j): (count, index sums, index box, separation bits, witness)} of the dense evaluation over the report's lattice."""
    t = half_gap(report.min_gap)
    insts = [inst.instance for inst in report.instances]
    wins = windows(insts, report.corner, report.step, report.dims, t)
    w, near = [], []
    for inst, (lo, hi) in zip(insts, wins):
        d = oracle.grid_eval(nodes.make_program(inst.shape()), report.corner, report.step, report.dims, threads=8)[..., 3]
        inwin = numpy.zeros(d.shape, dtype=bool)
        inwin[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
        w.append(d)
        near.append(inwin & (d < t))
    out = {}
    for i in range(len(w)):
        for j in range(i + 1, len(w)):
            both = near[i] & near[j]
            idx = numpy.argwhere(both)                     # lexicographic, the order of w[i][both]
            if len(idx):
                v = numpy.maximum(w[i][both], w[j][both])
                sep = v.min()
                witness = tuple(int(k) for k in idx[numpy.nonzero(v == sep)[0][0]])
                out[(i, j)] = (len(idx), tuple(int(k) for k in idx.sum(axis=0)),
                               (tuple(int(k) for k in idx.min(axis=0)), tuple(int(k) for k in idx.max(axis=0))),
                               int((sep + numpy.float32(0)).view(numpy.uint32)), witness)
    return out


def device_near(report):
    return {(p.i, p.j): (p.count, p.index_sums, p.index_box, int(numpy.float32(p.separation).view(numpy.uint32)), p.witness)
            for p in report.pairs}


def check_against_dense(report):
    assert device_near(report) == dense_near(report)


def evaluations_share(report):
    return report.samples_evaluated / (float(numpy.prod(report.dims)) * len(report.instances))


def _same_as_interference(report, inter):
    assert [(p.i, p.j, p.count, p.index_sums, p.index_box) for p in report.pairs] == \
           [(p.i, p.j, p.count, p.index_sums, p.index_box) for p in inter.pairs]


# the random assemblies and the gear train of test_gpu_interference.py

def _safe_random_shape(rng):
    """A random tree whose distance is a lower bound (no repetition, no twist) and whose box is finite and not huge."""
    while True:
        s = random_trees.random_3d(rng, 2)
        names = {ins.name for ins in nodes.make_schedule(s)[1]}
        box = s.bounding_box()
        if names & {"repetition", "circular_repetition_to", "twist_revolution_to"}:
            continue
        if not all(math.isfinite(v) for v in tuple(box.a) + tuple(box.b)) or max(box.size()) > 8:
            continue
        return s


def _random_assembly(seed, k, blended):
    rng = random.Random(seed)
    parts = [_safe_random_shape(rng).make_part("p%d" % i) for i in range(max(2, k // 3))]
    if blended:
        parts.append(shapes.union([shapes.box(2, 1, 1), shapes.sphere(1.5).translated_x(1)], r=0.3).make_part("blend"))

    def place(inst):
        axis = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.1, 1))
        return inst.rotated(axis, rng.uniform(-180, 180)).translated(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3))

    inner = cc.assembly("inner", [place(rng.choice(parts)) for _ in range(3)])
    instances = [place(inner)] + [place(rng.choice(parts)) for _ in range(k - 3)]
    instances.append(place(rng.choice(parts)).hidden())
    return cc.assembly("random", instances)


def _gear_train():
    m, h = 1.0, 4.0
    sun = shapes.gears.InvoluteGear(12, m).extruded(h).make_part("sun")
    planet = shapes.gears.InvoluteGear(9, m).extruded(h).make_part("planet")
    pin = shapes.cylinder(h=h + 4, d=2.0).make_part("pin")
    carrier = (shapes.cylinder(h=2, d=30) - shapes.cylinder(h=3, d=6)).make_part("carrier")
    orbit = (12 + 9) * m / 2
    instances = [sun]
    for k in range(3):
        instances.append(planet.rotated_z(7 + 40 * k).translated_x(orbit).rotated_z(120 * k))
    for k in range(3):
        instances.append(pin.translated(orbit, 0, 1).rotated_z(120 * k))
    instances.append(carrier.translated_z(h / 2 + 1.5))
    return cc.assembly("planetary", instances)


RANDOM = [(1, 4, False), (2, 9, False), (3, 16, False), (4, 6, True), (5, 12, True)]


@pytest.mark.parametrize("gap_steps", [0, 2, 8])
@pytest.mark.parametrize("seed,k,blended", RANDOM)
def test_random_assemblies_match_the_dense_oracle(hip, seed, k, blended, gap_steps):
    asm = _random_assembly(seed, k, blended)
    box = asm.shape().bounding_box()
    resolution = max(box.size()) / 90
    r = cc.clearance(asm, resolution, gap_steps * resolution)
    assert len(r.instances) == k and max(r.dims) <= 96 + gap_steps + 2
    check_against_dense(r)
    assert r.pairs, "the random placement should make some pair come close"


@pytest.mark.parametrize("seed,k,blended", [RANDOM[1], RANDOM[4]])
def test_zero_gap_is_interference_on_random_assemblies(hip, seed, k, blended):
    asm = _random_assembly(seed, k, blended)
    resolution = max(asm.shape().bounding_box().size()) / 90
    r = cc.clearance(asm, resolution, 0)
    inter = cc.interference(asm, resolution)
    assert r.corner.tolist() == inter.corner.tolist() and r.dims.tolist() == inter.dims.tolist()
    _same_as_interference(r, inter)
    assert all(p.separation < 0 for p in r.pairs)


def test_zero_gap_is_interference_on_the_gear_train(hip):
    asm = _gear_train()
    _same_as_interference(cc.clearance(asm, 0.1, 0.0), cc.interference(asm, 0.1))


def _gap_bound(p, gap, step):
    sep2 = 2 * float(p.separation)
    assert gap - 1e-5 <= sep2 <= gap + float(step) * math.sqrt(3) + 1e-5, (sep2, gap)


def test_two_spheres(hip):
    ball = shapes.sphere(r=1).make_part("ball")
    asm = cc.assembly("spheres", [ball, ball.translated(2.3, 0, 0)])       # gap 0.3
    r = cc.clearance(asm, 0.02, 0.5)
    assert [(p.i, p.j) for p in r.pairs] == [(0, 1)]
    p = r.pairs[0]
    _gap_bound(p, 0.3, r.step)
    assert 1.0 - 0.05 <= p.witness_point.x <= 1.3 + 0.05 and abs(p.witness_point.y) < 0.05 and abs(p.witness_point.z) < 0.05
    check_against_dense(r)
    assert cc.clearance(asm, 0.02, 0.2).pairs == []


def test_two_boxes_along_x(hip):
    a = shapes.box(1, 1, 1).make_part("a")
    asm = cc.assembly("boxes", [a, a.translated_x(1.25)])                   # faces at 0.5 and 0.75
    r = cc.clearance(asm, 0.02, 0.4)
    assert [(p.i, p.j) for p in r.pairs] == [(0, 1)]
    p = r.pairs[0]
    _gap_bound(p, 0.25, r.step)
    assert 0.5 <= p.witness_point.x <= 0.75
    check_against_dense(r)


def test_overlapping_pair_has_negative_separation(hip):
    ball = shapes.sphere(r=1).make_part("ball")
    r = cc.clearance(cc.assembly("lens", [ball, ball.translated(1.2, 0, 0).rotated_z(17)]), 0.05, 0.3)
    assert len(r.pairs) == 1 and r.pairs[0].separation < 0
    check_against_dense(r)


def test_gear_train_is_reproducible_and_survives_overflow(hip):
    asm = _gear_train()
    first = cc.clearance(asm, 0.1, 0.5)
    assert len(first.instances) == 8 and first.traversals == 1
    again = cc.clearance(asm, 0.1, 0.5)
    assert first.pairs == again.pairs and first.samples_evaluated == again.samples_evaluated
    small = cc.clearance(asm, 0.1, 0.5, initial_capacity=32)
    assert small.traversals > 1 and small.pairs == first.pairs
    # every sample inside both instances is near them: the interfering pairs are there, with more samples
    near = {(p.i, p.j): p for p in first.pairs}
    inside = cc.interference(asm, 0.1)
    assert {(1, 4), (2, 5), (3, 6), (4, 7), (5, 7), (6, 7)} <= set(near)
    for p in inside.pairs:
        assert near[(p.i, p.j)].count > p.count and near[(p.i, p.j)].separation < 0
    assert evaluations_share(first) <= 0.10
