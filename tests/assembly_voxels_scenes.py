"""The CPU reference of the assembly voxel tests (test_assembly_voxels_host.py proves on the CPU that each scenario holds
the edge it is there for; test_gpu_assembly_voxels.py runs them on the device).  The scenarios are those of
assembly_mass_scenes.py, dense fields included: both features are defined on one lattice.

`reference_voxels(instances, corner, step, dims, retire, side)` is written from the definitions in
codecad_amd/assembly_voxels.py:
  * the DENSE half takes every instance's field over the whole lattice (oracle.grid_eval, cached per scenario) and gives
    the part ids -- the lowest index with w < 0, else 255 -- and the samples each instance owns;
  * the TRAVERSAL half applies the row {x0, y0, z0, capped, cand}, the thresholds and the owner-retire rule level by
    level: float32 centres operation for operation as the kernels compute them (oracle.evaluate_points there), candidates
    in ascending index, a lane closed above its lowest full candidate, the wavefront's early stop per parent of 64
    children over its live lanes, the capped top bit inherited.  It gives the volume the traversal writes, its counts, the
    number of evaluations, per level how many children were dropped, retired, retired although a candidate ABOVE the owner
    is a boundary candidate there (evaluated for this figure alone, never counted), listed and listed capped, the bytes
    the retired children fill in a volume of pitch pz, and how often the rule called a child full although the dense half
    has a sample of it outside (the premise, broken).  `touched` marks the samples it wrote; `capacity` cuts every list to
    its first rows, as a list that overflows on the device is cut.
"""
import collections
import functools

import numpy

import codecad_amd as cc
from codecad_amd import shapes, nodes, _instance_cells
import oracle

import assembly_mass_scenes as mass
from assembly_mass_scenes import SCENES, scene, owners, forced_top_cells, threshold    # noqa: F401 (shared with the tests)

EMPTY = 255
NONE = 64                                                        # a lane without a full candidate

Reference = collections.namedtuple("Reference", "ids counts written touched traversal_counts evaluations levels leaf premise_broken")
Level = collections.namedtuple("Level", "child dropped retired retired_under_boundary listed listed_capped filled_bytes")
Leaf = collections.namedtuple("Leaf", "cells capped")


def dense_ids(inside):
    """uint8 ids and per-instance owned counts of the dense definition."""
    ids = numpy.full(inside[0].shape, EMPTY, dtype=numpy.uint8)
    own = owners(inside)
    for k, m in enumerate(own):
        ids[m] = k
    return ids, [int(m.sum()) for m in own]


def top_rows(instances, corner, step, dims, side):
    """(x0, y0, z0, cand) of the top level: cell_rows(windows(...), dims, side, least=1), nothing capped."""
    return mass.top_rows(instances, corner, step, dims, side)


def _top_bit(cand):
    """The index of the highest set bit of every uint64 of `cand` (0 for 0)."""
    out = numpy.zeros(cand.shape, dtype=numpy.int64)
    for k in range(64):
        out[(cand >> numpy.uint64(k)) & numpy.uint64(1) != 0] = k
    return out


def reference_voxels(instances, corner, step, dims, retire, side=None, w=None, capacity=None):
    corner, step = numpy.asarray(corner, dtype=numpy.float32), numpy.float32(step)
    dims = numpy.asarray(dims, dtype=numpy.int64)
    n = len(instances)
    tapes = [nodes.make_program(i.shape()) for i in instances]
    if w is None:
        w = mass.dense_fields(instances, corner, step, dims)
    inside = [f < 0 for f in w]                                  # (a NaN is not inside)
    ids, counts = dense_ids(inside)
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
    capped = numpy.zeros(len(rows), dtype=bool)
    pz = -(-int(dims[2]) // 16) * 16
    written = numpy.full(tuple(dims), EMPTY, dtype=numpy.uint8)  # the prefill
    touched = numpy.zeros(tuple(dims), dtype=bool)
    got = [0] * n
    lanes = numpy.arange(64)
    offsets = numpy.stack([lanes >> 4, (lanes >> 2) & 3, lanes & 3], axis=-1)     # lane = 16 x + 4 y + z
    evaluations, levels, premise_broken = 0, [], 0
    one, zero = numpy.uint64(1), numpy.uint64(0)
    while side > 4:
        child = side // 4
        thr = threshold(child, step)
        first = origin[:, None, :] + offsets[None, :, :] * child                 # [m, 64, 3]
        live = (first < dims).all(axis=-1)
        h = numpy.float32(0.5) * numpy.float32(child - 1)
        centre = corner + step * (first.astype(numpy.float32) + h)               # float32, one rounding per operation
        assert centre.dtype == numpy.float32
        top = _top_bit(cand)
        todo = numpy.where(capped, cand & ~(one << top.astype(numpy.uint64)), cand)
        keep = numpy.zeros((len(cand), 64), dtype=numpy.uint64)
        owner = numpy.full((len(cand), 64), NONE, dtype=numpy.int64)
        for k in range(n):                                                       # ascending
            bit = one << numpy.uint64(k)
            wave = ((todo & bit) != 0) & (live & (owner == NONE)).any(axis=1)    # the wavefront's early stop, per parent
            at = wave[:, None] & live
            if not at.any():
                continue
            values = oracle.evaluate_points(tapes[k], centre[at])[:, 3]
            evaluations += len(values)                                            # live lanes x candidates evaluated
            open_ = owner[at] == NONE
            keep[at] |= numpy.where(open_ & ~(values >= thr), bit, zero)
            if retire:
                now_full = open_ & (values < -thr)
                owner[at] = numpy.where(now_full, k, owner[at])
                lo = first[at][now_full]
                hi = numpy.minimum(lo + child, dims)
                premise_broken += int((inside_count(k, lo, hi) != (hi - lo).prod(axis=-1)).sum())
        inherit = capped[:, None] & (owner == NONE)
        keep |= numpy.where(inherit, (one << top.astype(numpy.uint64))[:, None], zero)
        owner = numpy.where(inherit, top[:, None], owner)
        lane_capped = owner != NONE
        retired = live & lane_capped & (keep != 0) & ((keep & (keep - one)) == 0)
        going = live & (keep != 0) & ~retired
        under_boundary, filled_bytes = 0, 0
        for cell, lane in numpy.argwhere(retired):
            lo = first[cell, lane]
            hi = numpy.minimum(lo + child, dims)
            box = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
            k = int(owner[cell, lane])
            assert int(keep[cell, lane]) == 1 << k
            written[box] = k
            touched[box] = True
            got[k] += int((hi - lo).prod())
            filled_bytes += int((hi[0] - lo[0]) * (hi[1] - lo[1]) * (min(lo[2] + child, pz) - lo[2]))
            # is a candidate above the owner a boundary candidate here?  (the traversal never asks)
            above = [j for j in range(k + 1, n) if int(todo[cell]) >> j & 1]
            for j in above:
                value = oracle.evaluate_points(tapes[j], centre[cell, lane][None, :])[0, 3]
                if not value >= thr and not value < -thr:
                    under_boundary += 1
                    break
        levels.append(Level(child, int((live & (keep == 0)).sum()), int(retired.sum()), under_boundary, int(going.sum()),
                            int((going & lane_capped).sum()), filled_bytes))
        origin, cand, capped = first[going][:capacity], keep[going][:capacity], lane_capped[going][:capacity]
        side = child
    leaf_capped = 0
    for (x0, y0, z0), c, cap in zip(origin.tolist(), cand.tolist(), capped.tolist()):
        box = tuple(slice(a, min(a + 4, int(d))) for a, d in zip((x0, y0, z0), dims))
        live = int(numpy.prod([s.stop - s.start for s in box]))
        top = c.bit_length() - 1
        todo = c & ~(1 << top) if cap else c
        evaluations += live * bin(todo).count("1")
        leaf_capped += bool(cap)
        cell = numpy.full([s.stop - s.start for s in box], top if cap else EMPTY, dtype=numpy.uint8)
        for k in reversed(range(n)):                              # (the lowest inside wins)
            if todo >> k & 1:
                cell[inside[k][box]] = k
        written[box] = cell
        touched[box] = True
        for k in range(n):
            if c >> k & 1:
                got[k] += int((cell == k).sum())
    return Reference(ids, counts, written, touched, got, evaluations, levels, Leaf(len(origin), leaf_capped), premise_broken)


@functools.lru_cache(maxsize=None)
def reference(name, retire=True):
    """The Reference of a scenario, computed once and shared; nobody changes it."""
    asm, resolution, instances, corner, step, dims = scene(name)
    ref = reference_voxels(instances, corner, step, dims, retire, side=SCENES[name].side, w=mass._fields(name))
    ref.ids.setflags(write=False)
    ref.written.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def strict_reversed():
    """(assembly, resolution, dense fields, Reference) of the dyadic scenario `strict` with the outer box LAST: a sample ON a
    face of a half is not inside that half, so it falls to the outer box (index 2) -- in `strict` itself the outer box
    has index 0 and owns every sample whatever the halves say."""
    outer, half = shapes.box(2.0625).make_part("outer"), shapes.box(1).make_part("half")
    asm = cc.assembly("dyadic", [half.translated_x(0.5), half.translated_x(-0.5), outer])
    resolution = 0.0625
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims = _instance_cells.checked_lattice(instances, resolution)
    w = mass.dense_fields(instances, corner, step, dims)
    ref = reference_voxels(instances, corner, step, dims, True, w=w)
    ref.ids.setflags(write=False)
    return asm, resolution, w, ref
