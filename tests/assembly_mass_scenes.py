"""The scenarios of the assembly mass tests (test_assembly_mass_reference_host.py proves on the CPU that each holds the
edge it is there for; test_gpu_assembly_mass.py runs them on the device) and their CPU reference.

`reference_mass(instances, corner, step, dims, retire)` is written from the definitions in codecad_amd/assembly_mass.py:
  * the DENSE half evaluates every instance over the whole lattice (oracle.grid_eval) and gives, per instance, the ten
    index sums of V_k and of O_k and the index box of V_k;
  * the TRAVERSAL half applies the row, the threshold and the retire rule level by level, the centres of the children in
    float32 operation for operation as the kernels compute them (oracle.evaluate_points there), and gives the sums again,
    the number of evaluations, per level the numbers of retired and surviving children, and how often the rule called
    a child full although the dense half has a sample of it outside (the premise, broken).
"""
import collections
import functools
import math
import random

import numpy

import codecad_amd as cc
from codecad_amd import shapes, nodes, _instance_cells
import oracle

from test_gpu_interference import _random_assembly, _gear_train
import heavy_instances

Reference = collections.namedtuple("Reference", "w sums owned boxes traversal_sums traversal_owned evaluations levels leaf "
                                                "premise_broken union_count")
Level = collections.namedtuple("Level", "child retired surviving dropped mixed")       # mixed: survivors with a full candidate
Leaf = collections.namedtuple("Leaf", "cells mixed")                                    # mixed: a full and an evaluated candidate


def index_sums(weight):
    """The ten sums n, x, y, z, xx, yy, zz, xy, xz, yz of the indices of a lattice of integer weights, as Python ints."""
    c = weight.astype(numpy.int64)
    ix, iy, iz = (numpy.arange(d, dtype=numpy.int64) for d in c.shape)
    cx, cy, cz = c.sum(axis=(1, 2)), c.sum(axis=(0, 2)), c.sum(axis=(0, 1))
    cxy, cxz, cyz = c.sum(axis=2), c.sum(axis=1), c.sum(axis=0)
    return tuple(int(v) for v in (
        c.sum(), (cx * ix).sum(), (cy * iy).sum(), (cz * iz).sum(), (cx * ix * ix).sum(), (cy * iy * iy).sum(), (cz * iz * iz).sum(),
        (cxy * numpy.outer(ix, iy)).sum(), (cxz * numpy.outer(ix, iz)).sum(), (cyz * numpy.outer(iy, iz)).sum()))


def index_box(inside):
    idx = numpy.argwhere(inside)
    return (tuple(int(v) for v in idx.min(axis=0)), tuple(int(v) for v in idx.max(axis=0))) if len(idx) else None


def owners(inside):
    """Per instance the samples it owns: inside it and inside no instance of lower index."""
    taken = numpy.zeros_like(inside[0])
    out = []
    for m in inside:
        out.append(m & ~taken)
        taken = taken | m
    return out


def threshold(child, step):
    return numpy.float32(child * float(step) * math.sqrt(3) / 2 * (1 + 2.0 ** -10))


def top_rows(instances, corner, step, dims, side):
    """(x0, y0, z0, cand) of the top level: cell_rows(windows(...), dims, side, least=1), nothing full."""
    rows = _instance_cells.cell_rows(_instance_cells.windows(instances, corner, float(step), dims), dims, side, least=1)
    return [(int(r[0]) & 0xffff, int(r[0]) >> 16, int(r[1]), int(r[2]) | (int(r[3]) << 32)) for r in rows]


def dense_fields(instances, corner, step, dims):
    """float32 w_k over the whole lattice, per instance: the dense definition."""
    return [oracle.grid_eval(nodes.make_program(i.shape()), corner, step, dims, threads=8)[..., 3].copy() for i in instances]


def reference_mass(instances, corner, step, dims, retire, side=None, w=None):
    corner, step = numpy.asarray(corner, dtype=numpy.float32), numpy.float32(step)
    dims = numpy.asarray(dims, dtype=numpy.int64)
    n = len(instances)
    tapes = [nodes.make_program(i.shape()) for i in instances]
    if w is None:
        w = dense_fields(instances, corner, step, dims)
    inside = [f < 0 for f in w]                                  # (a NaN is not inside)
    own = owners(inside)
    sums, owned, boxes = [index_sums(m) for m in inside], [index_sums(m) for m in own], [index_box(m) for m in inside]
    # how many samples of any index box are inside k: a table of prefix sums
    prefix = [numpy.pad(m.astype(numpy.int64).cumsum(0).cumsum(1).cumsum(2), ((1, 0), (1, 0), (1, 0))) for m in inside]

    def inside_count(k, lo, hi):                                 # lo, hi: int64[m, 3], hi exclusive
        p = prefix[k]
        total = 0
        for corner_bits in range(8):
            at = [(hi if corner_bits >> a & 1 else lo)[:, a] for a in range(3)]
            sign = -1 if (3 - bin(corner_bits).count("1")) % 2 else 1
            total = total + sign * p[at[0], at[1], at[2]]
        return total

    # ---- the traversal ------------------------------------------------------------------------------------------------
    side = _instance_cells.top_side(dims) if side is None else side
    rows = top_rows(instances, corner, step, dims, side)
    origin = numpy.array([r[:3] for r in rows], dtype=numpy.int64).reshape(-1, 3)
    cand = numpy.array([r[3] for r in rows], dtype=numpy.uint64)
    full = numpy.zeros_like(cand)
    got_v = [numpy.zeros(tuple(dims), dtype=numpy.int32) for _ in range(n)]      # how often a sample was added to V_k
    got_o = [numpy.zeros(tuple(dims), dtype=numpy.int32) for _ in range(n)]
    lanes = numpy.arange(64)
    offsets = numpy.stack([lanes >> 4, (lanes >> 2) & 3, lanes & 3], axis=-1)     # lane = 16 x + 4 y + z
    evaluations, levels, premise_broken = 0, [], 0
    one = numpy.uint64(1)
    while side > 4:
        child = side // 4
        thr = threshold(child, step)
        first = origin[:, None, :] + offsets[None, :, :] * child                 # [m, 64, 3]
        live = (first < dims).all(axis=-1)
        h = numpy.float32(0.5) * numpy.float32(child - 1)
        centre = corner + step * (first.astype(numpy.float32) + h)               # float32, one rounding per operation
        assert centre.dtype == numpy.float32
        keep = numpy.repeat(full[:, None], 64, axis=1)
        filled = keep.copy()
        todo = cand & ~full
        for k in range(n):
            bit = one << numpy.uint64(k)
            at = ((todo & bit) != 0)[:, None] & live
            if not at.any():
                continue
            values = oracle.evaluate_points(tapes[k], centre[at])[:, 3]
            evaluations += len(values)
            keep[at] |= numpy.where(~(values >= thr), bit, numpy.uint64(0))
            if retire:
                now_full = values < -thr
                filled[at] |= numpy.where(now_full, bit, numpy.uint64(0))
                lo = first[at][now_full]
                hi = numpy.minimum(lo + child, dims)
                premise_broken += int((inside_count(k, lo, hi) != (hi - lo).prod(axis=-1)).sum())
        filled &= keep
        retired = live & (keep != 0) & (keep == filled)
        going = live & (keep != filled)
        for cell, lane in numpy.argwhere(retired):
            lo = first[cell, lane]
            hi = numpy.minimum(lo + child, dims)
            box = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
            mask = int(filled[cell, lane])
            for k in range(n):
                if mask >> k & 1:
                    got_v[k][box] += 1
            got_o[(mask & -mask).bit_length() - 1][box] += 1
        levels.append(Level(child, int(retired.sum()), int(going.sum()), int((live & (keep == 0)).sum()),
                            int((going & (filled != 0)).sum())))
        origin, cand, full = first[going], keep[going], filled[going]
        side = child
    leaf_mixed = 0
    for (x0, y0, z0), c, f in zip(origin.tolist(), cand.tolist(), full.tolist()):
        box = tuple(slice(a, min(a + 4, int(d))) for a, d in zip((x0, y0, z0), dims))
        live = int(numpy.prod([s.stop - s.start for s in box]))
        todo = c & ~f
        evaluations += live * bin(todo).count("1")
        leaf_mixed += bool(f and todo)
        taken = numpy.zeros([s.stop - s.start for s in box], dtype=bool)
        for k in range(n):
            if not c >> k & 1:
                continue
            m = numpy.ones_like(taken) if f >> k & 1 else inside[k][box]
            got_v[k][box] += m
            got_o[k][box] += m & ~taken
            taken |= m
    union = numpy.zeros(tuple(dims), dtype=bool)
    for m in inside:
        union |= m
    return Reference(w, sums, owned, boxes, [index_sums(g) for g in got_v], [index_sums(g) for g in got_o], evaluations, levels,
                     Leaf(len(origin), leaf_mixed), premise_broken, int(union.sum()))


# ---- the scenarios ----------------------------------------------------------------------------------------------------

Scene = collections.namedtuple("Scene", "build resolution side densities", defaults=(None, None))
Scene.__doc__ = """`build()` -> the assembly weighed at `resolution`; `side`: the top side forced on it (None: what top_side() gives);
`densities`: what the call passes."""

BOX_A, BOX_B = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), ((0.5, -0.25, -2.0), (2.5, 0.75, 1.0))
BOX_DENSITIES = (2.0, 0.5)


def _boxes():
    """Faces on multiples of 1/8, samples half-way between; `b` overlaps `a`, so O_1 != V_1."""
    a = shapes.box(2, 2, 2).make_part("a")
    b = shapes.box(2, 1, 3).make_part("b")
    return cc.assembly("boxes", [a, b.translated(1.5, 0.25, -0.5)])


def _sphere():
    """A ball of radius 1 with a small block inside it: cells deep in the ball that the block's surface crosses."""
    return cc.assembly("ball", [shapes.sphere(r=1).make_part("ball"), shapes.box(0.6).make_part("core").translated(0.2, 0.1, 0.0)])


def _coarse():
    """A box 80 samples wide and a small ball beside it (the lattice is wider than the box): 91 x 80 x 80."""
    return cc.assembly("coarse", [shapes.box(5, 5, 5).make_part("block"), shapes.sphere(r=0.25).make_part("ball").translated(2.9, 0, 0)])


def _coarse_160():
    """One box of 160 samples a side: its middle children of side 64 lie 64 samples deep, more than the 55.4 that side needs."""
    return cc.assembly("block", [shapes.box(5, 5, 5).make_part("block")])


OWNERSHIP_ORDERS = ((0, 1, 2), (2, 0, 1), (1, 2, 0))


def _ownership(order):
    """Three parts that overlap pairwise and all together, listed in `order`, a hidden instance between them and one in
    a subassembly of its own; the placements do not depend on the order."""
    placed = [shapes.sphere(r=1).make_part("ball"),
              shapes.box(1.6).make_part("block").translated(0.7, 0.2, 0.0),
              shapes.cylinder(h=1.5, d=1.4).make_part("peg").translated(0.3, 0.6, 0.2)]
    ghost = shapes.box(3).make_part("ghost").hidden()
    return cc.assembly("own", [placed[order[0]], ghost, cc.assembly("inner", [placed[order[1]]]), placed[order[2]]])


def _solids(n_visible):
    """`n_visible` visible instances on a 4 x 4 x 4 arrangement 0.8 apart, index 16 x + 4 y + z and then, from 48 on, one
    more layer BESIDE the indices 0..15: small boxes, balls, pegs and differences of them, each large enough to overlap its
    neighbours -- so the instances 48.. (and 32 in the arrangement of 33) overlap instances below 32.  A hidden instance
    and a nested subassembly sit between them."""
    rng = random.Random(6433)
    parts = [shapes.sphere(r=0.55).make_part("ball"), shapes.box(0.9, 0.8, 1.0).make_part("block"),
             shapes.cylinder(h=1.1, d=0.8).make_part("peg"),
             (shapes.box(1.0) - shapes.sphere(r=0.45).translated(0.3, 0.3, 0.3)).make_part("bitten"),
             (shapes.cylinder(h=1.0, d=1.0) - shapes.cylinder(h=2, d=0.4)).make_part("tube")]

    def place(k):
        where = [k // 16, (k // 4) % 4, k % 4] if k < 32 else [(k - 32) // 16, ((k - 32) // 4) % 4, (k - 32) % 4]
        shift = 0.0 if k < 32 else 0.4                             # the second half sits between the cells of the first
        axis = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.1, 1))
        return parts[(k + k // 4) % 5].rotated(axis, rng.uniform(-180, 180)).translated(*(0.8 * c + shift + rng.uniform(-0.05, 0.05) for c in where))

    placed = [place(k) for k in range(n_visible)]
    ghost = parts[1].translated(1.0, 1.0, 1.0).hidden()
    listed = placed[:5] + [ghost, cc.assembly("inner", placed[5:8] + [ghost.translated_x(0.5)] + placed[8:10])] + placed[10:]
    return cc.assembly("solids", listed)


def _rims():
    """13 x 9 x 11 samples: no axis a multiple of 4, the box reaches the last index of every axis."""
    return cc.assembly("rims", [shapes.box(1.625, 1.125, 1.375).make_part("block"),
                                shapes.sphere(r=0.4).make_part("ball").translated(0.3, 0.1, 0.2)])


def _strict():
    """The dyadic construction of test_instance_cells_reference_host.py: a lattice of step 2^-4 whose samples lie ON the
    faces of the two halves (corner = -1 exactly)."""
    outer = shapes.box(2.0625).make_part("outer")
    half = shapes.box(1).make_part("half")
    return cc.assembly("dyadic", [outer, half.translated_x(0.5), half.translated_x(-0.5)])


def blend_part(r=0.3):
    return shapes.union([shapes.box(2, 1, 1), shapes.sphere(1.5).translated_x(1)], r=r)


def _blend():
    return cc.assembly("blend", [blend_part().make_part("blend"), shapes.box(1, 3, 1).make_part("bar").translated(0.5, 0, 0.2)])


def _random(seed, k, blended):
    return functools.partial(_random_assembly, seed, k, blended)


RANDOM = ((1, 4, False), (2, 9, False), (5, 12, True))

SCENES = {
    "boxes": Scene(_boxes, 0.125, None, BOX_DENSITIES),
    "sphere": Scene(_sphere, 0.0625),
    "coarse_64": Scene(_coarse, 0.0625, 64),
    "coarse_256": Scene(_coarse, 0.0625, 256),
    "coarse_160": Scene(_coarse_160, 0.03125, 256),
    "solids33": Scene(functools.partial(_solids, 33), 0.07),
    "solids64": Scene(functools.partial(_solids, 64), 0.07),
    "rims": Scene(_rims, 0.125),
    "strict": Scene(_strict, 0.0625),
    "blend": Scene(_blend, 0.06),
    "gears": Scene(_gear_train, 0.3),
}
for _order in OWNERSHIP_ORDERS:
    SCENES["ownership_%d%d%d" % _order] = Scene(functools.partial(_ownership, _order), 0.08)
for _seed, _k, _blended in RANDOM:
    SCENES["random_%d" % _seed] = Scene(_random(_seed, _k, _blended), None)
SCENES.update(heavy_instances.mass_scenes(Scene))        # parts with wide register files among light ones


def forced_top_cells(dims, side):
    """The _MAX_TOP_CELLS that makes top_side(dims) return `side` on a lattice that would take 16."""
    return int(numpy.prod(-(-numpy.asarray(dims, dtype=numpy.int64) // side)))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scenario."""
    sc = SCENES[name]
    asm = sc.build()
    resolution = sc.resolution if sc.resolution is not None else max(asm.shape().bounding_box().size()) / 90
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims = _instance_cells.checked_lattice(instances, resolution)
    return asm, resolution, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def reference(name, retire=True):
    """The Reference of a scenario, computed once and shared; nobody changes it."""
    asm, resolution, instances, corner, step, dims = scene(name)
    return reference_mass(instances, corner, step, dims, retire, side=SCENES[name].side, w=_fields(name))


@functools.lru_cache(maxsize=None)
def _fields(name):
    asm, resolution, instances, corner, step, dims = scene(name)
    return dense_fields(instances, corner, step, dims)
