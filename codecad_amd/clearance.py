"""Clearance between the instances of an assembly: which pairs come closer than a gap, how close, and where.

`clearance(asm, resolution, min_gap) -> ClearanceReport`.  Like `interference` (interference.py), the answer is defined on
a lattice of samples, densely, with t = float32(min_gap / 2):
  * the lattice is `interference.lattice` of the visible instances' bounding boxes grown by t on every side (in float64);
    for min_gap = 0 it is the interference lattice;
  * the WINDOW of instance n is an index box computed on the host, lo = clip(floor((A - t - corner - step) / step), 0,
    dims - 1), hi = clip(ceil((B + t - corner + step) / step), 0, dims - 1) for its box [A, B]; outside it the instance
    is never near, so the answer does not depend on how far out a loose distance bound stays small;
  * a sample is NEAR the pair (i, j) when it lies in both windows, w_i < t and w_j < t (strictly; a NaN is never near),
    w being each instance's own tape evaluated exactly as `interference` evaluates it; there v = max(w_i, w_j).
A pair's count, index sums and index box are those of its near samples; its `separation` is the least v (a zero as +0.0)
and its `witness` the lexicographically smallest (x, y, z) index whose v equals it (-0.0 == +0.0).  With well-formed
bounding boxes and min_gap = 0, near means inside both, and the pairs are `interference`'s.

What `separation` means: for exact distance functions (spheres, boxes along a face normal) the true gap between the two
parts satisfies gap <= 2 * separation <= gap + step * sqrt(3).  The lower bound is the triangle inequality (a sample
at distance w_i from one part and w_j from the other puts them at most w_i + w_j <= 2 v apart); the upper bound comes
from the sample nearest to the mid-point of the closest pair of points, at most step * sqrt(3) / 2 from it.  For shapes
whose w underestimates the distance, 2 * separation can be smaller than the gap: the safe direction for a clearance
check, which may then report a near miss that is none but never hides a real one.  Overlapping pairs have separation < 0.

It is computed sparsely, on the device, one synchronisation in all (csrc/clearance.hip), by interference's traversal:
  * the host seeds the top level from the windows and keeps the cells that two windows or more reach;
  * every coarser level drops a candidate from a child when the child misses its window or w(child centre) >= thr,
    thr = float32((t + side * step * sqrt(3) / 2) * (1 + 2^-10)) for a child of `side` samples: the samples lie within
    (side - 1) * step * sqrt(3) / 2 of the centre, so each has w >= t there (interference.py states the margin);
  * the finest level (cells of 4^3 samples) evaluates every remaining candidate at every sample and adds each pair's
    near samples to its accumulators, the least v as an order-preserving uint32 key; a second launch over the same
    cells evaluates again and takes, per pair, the least packed index x << 32 | y << 16 | z whose v has that key.
`samples_evaluated` counts every level and both launches.  The culling assumes what `interference` assumes: every
instance's distance is a lower bound on the true distance (Lipschitz constant at most 1).
"""
import collections
import ctypes
import math

import numpy

from . import util
from . import hip_util
from . import subdivision
from .interference import Instance, lattice as _lattice, _visible, _top_side, _windows, _cell_rows, _device_table, _levels
from .hip_util import manager as hip_manager, check

# the accumulators of a pair (launchers.hpp hu_clearance::PairAcc)
_PAIR = numpy.dtype([("sums", "<u8", (4,)), ("witness", "<u8"), ("lo", "<u4", (3,)), ("hi", "<u4", (3,)), ("key", "<u4"),
                     ("pad", "<u4")])


class NearMiss(collections.namedtuple("NearMiss", "i j count volume centroid index_box bounding_box index_sums "
                                                  "separation witness witness_point")):
    """Samples near both instances i < j: the first eight fields as in interference.Overlap, over the near samples;
    `separation` (float32), the least v = max(w_i, w_j) over them; `witness`, the lexicographically smallest (x, y, z)
    index whose v equals it; `witness_point`, that sample's position (Vector)."""

    __slots__ = ()


class ClearanceReport(collections.namedtuple("ClearanceReport",
                                             "instances corner step dims min_gap pairs samples_evaluated traversals")):
    """As interference.InterferenceReport, with `min_gap` and `pairs`: a NearMiss per pair with near samples, ordered
    by (i, j)."""

    __slots__ = ()


def half_gap(min_gap):
    """t = float32(min_gap / 2); ValueError unless min_gap is a finite number >= 0."""
    if not (isinstance(min_gap, (int, float, numpy.floating, numpy.integer)) and math.isfinite(min_gap) and min_gap >= 0):
        raise ValueError("min_gap must be a finite number >= 0, not %r" % (min_gap,))
    return numpy.float32(min_gap / 2)


def lattice(instances, resolution, t):
    """(corner, step, dims) of the lattice over the instances' boxes grown by t."""
    return _lattice(instances, resolution, grow=float(t))


def windows(instances, corner, step, dims, t):
    """int64[n, 2, 3]: the first and last lattice index per axis at which each instance may be near."""
    return _windows(instances, corner, float(step), dims, grow=float(t))


def _key_to_float(key):
    """The float32 of an order key (clearance.hip order_key)."""
    bits = key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff
    return numpy.array([bits], dtype=numpy.uint32).view(numpy.float32)[0]


def _traverse(table, n, distance_only, lane_bytes, wins, t, top, sides, corner, step, dims, capacities, queue):
    """Every level enqueued back to back, ONE synchronisation -> (list counts, evaluations, pair accumulators)."""
    lib = hip_manager.lib
    n_levels = len(sides)                   # levels of cells above the finest one
    # one device buffer of everything the host reads: [list headers: 16 B per level | evaluations: 16 B | pairs]
    head = 16 * n_levels + 16
    init = numpy.zeros(head + n * n * _PAIR.itemsize, dtype=numpy.uint8)
    pairs0 = init[head:].view(_PAIR)
    pairs0["lo"] = 0xffffffff
    pairs0["key"] = 0xffffffff
    pairs0["witness"] = 0xffffffffffffffff
    results = hip_util.Buffer(numpy.uint8, (init.size,), queue=queue)
    results.enqueue_write(init)
    first = numpy.zeros((len(top) + 1, 4), dtype=numpy.uint32)
    first[0, 0] = len(top)
    first[1:] = top
    parents = hip_util.Buffer(numpy.uint32, first.shape, queue=queue)
    parents.enqueue_write(first)
    buffers, max_parents = [parents], len(top)
    d = (ctypes.c_uint32 * 3)(*(int(v) for v in dims))
    c = (ctypes.c_float * 3)(*(float(v) for v in corner))
    evaluations = results.device_ptr + 16 * n_levels
    for level, (side, capacity) in enumerate(zip(sides, capacities)):
        child = side // 4
        thr = numpy.float32((float(t) + child * float(step) * math.sqrt(3) / 2) * (1 + 2.0 ** -10))
        children = hip_util.Buffer(numpy.uint32, (capacity + 1, 4), queue=queue)
        check(lib.hu_memset(children.device_ptr, 0, 16, queue.handle), "hu_memset")
        check(lib.hu_clearance_cells_indirect(table.device_ptr, n, distance_only, lane_bytes, wins.device_ptr,
                                              parents.device_ptr + 16, parents.device_ptr, max_parents, child, d, c, step,
                                              thr, children.device_ptr, children.device_ptr + 16, capacity, evaluations,
                                              queue.handle), "hu_clearance_cells_indirect")
        check(lib.hu_memcpy_d2d(results.device_ptr + 16 * level, children.device_ptr, 16, queue.handle), "hu_memcpy_d2d")
        buffers.append(children)
        parents, max_parents = children, capacity
    for name in ("hu_clearance_leaf_indirect", "hu_clearance_witness_indirect"):     # the witness needs the leaf's keys
        check(getattr(lib, name)(table.device_ptr, n, distance_only, lane_bytes, wins.device_ptr, parents.device_ptr + 16,
                                 parents.device_ptr, max_parents, d, c, step, t, results.device_ptr + head, evaluations,
                                 queue.handle), name)
    got = results.read()                    # the one synchronisation
    for b in buffers + [results]:
        b.release()
    counts = [int(v) for v in got[:16 * n_levels].view(numpy.uint32).reshape(n_levels, 4)[:, 0]]
    return counts, int(got[16 * n_levels:head].view(numpy.uint64)[0]), got[head:].view(_PAIR).reshape(n, n).copy()


def clearance(asm, resolution, min_gap, initial_capacity=None):
    """Pairs of visible instances of the 3D assembly `asm` that come closer than `min_gap` on the lattice at `resolution`
    (the module's docstring defines the lattice, the windows, what "near" means and what `separation` bounds) ->
    ClearanceReport.

    Raises ValueError as `interference` does, and for a min_gap that is not a finite number >= 0.  `initial_capacity`
    caps the first guess of every cell list (rows); lists that overflow are regrown, so it changes how often the
    traversal runs, never the result."""
    instances = _visible(asm, resolution)
    t = half_gap(min_gap)
    corner, step, dims = lattice(instances, resolution, t) if instances else (numpy.zeros(3, numpy.float32), numpy.float32(resolution), numpy.ones(3, numpy.int64))
    if dims[0] > 65536 or dims[1] > 65536 or dims[2] > 65536:
        raise ValueError("resolution %g gives a lattice of %s samples: at most 65536 per axis" % (resolution, dims.tolist()))
    named = [Instance(i.name, i) for i in instances]
    empty = ClearanceReport(named, corner, step, dims, min_gap, [], 0, 0)
    if len(instances) < 2:
        return empty
    side = _top_side(dims)
    wins = windows(instances, corner, step, dims, t)
    top = _cell_rows(wins, dims, side)
    if len(top) == 0:
        return empty

    queue = hip_manager.queue
    n = len(instances)
    table, distance_only, lane_bytes = _device_table(instances, queue)
    host_wins = numpy.ascontiguousarray(wins.reshape(n, 6).astype(numpy.uint32))
    wins_dev = hip_util.Buffer(numpy.uint32, host_wins.shape, queue=queue)
    wins_dev.enqueue_write(host_wins)
    sides, capacities = _levels(side, len(top), initial_capacity)
    traversals = 0
    while True:
        traversals += 1
        counts, evaluations, acc = _traverse(table, n, distance_only, lane_bytes, wins_dev, t, top, sides, corner, step,
                                             dims, capacities, queue)
        if all(k <= c for k, c in zip(counts, capacities)):
            break
        capacities = [subdivision.checked_capacity(max(c, int(k * 1.125) + 16)) for k, c in zip(counts, capacities)]
    table.release()
    wins_dev.release()

    pairs = []
    cell = float(step) ** 3
    for i in range(n):
        for j in range(i + 1, n):
            a = acc[i, j]
            count = int(a["sums"][0])
            if count == 0:
                continue
            sums = tuple(int(v) for v in a["sums"][1:])
            lo, hi = tuple(int(v) for v in a["lo"]), tuple(int(v) for v in a["hi"])
            centroid = util.Vector(*(float(corner[k]) + float(step) * sums[k] / count for k in range(3)))
            box = util.BoundingBox(util.Vector(*(float(corner[k] + step * numpy.float32(lo[k])) for k in range(3))),
                                   util.Vector(*(float(corner[k] + step * numpy.float32(hi[k])) for k in range(3))))
            w = int(a["witness"])
            witness = (w >> 32, (w >> 16) & 0xffff, w & 0xffff)
            point = util.Vector(*(float(corner[k] + step * numpy.float32(witness[k])) for k in range(3)))
            pairs.append(NearMiss(i, j, count, count * cell, centroid, (lo, hi), box, sums, _key_to_float(int(a["key"])),
                                  witness, point))
    return ClearanceReport(named, corner, step, dims, min_gap, pairs, evaluations, traversals)
