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

It is computed sparsely, on the device, one synchronisation in all (csrc/instance_pairs.hip), by interference's traversal
(_instance_cells.py):
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
import math

import numpy

from . import _instance_cells as cells
from ._instance_cells import Instance

# the accumulators of a pair (instance_args.hpp NearAcc)
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
    return cells.lattice(instances, resolution, grow=float(t))


def windows(instances, corner, step, dims, t):
    """int64[n, 2, 3]: the first and last lattice index per axis at which each instance may be near."""
    return cells.windows(instances, corner, float(step), dims, grow=float(t))


def _key_to_float(key):
    """The float32 of an order key (instance_pairs.hip order_key)."""
    bits = key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff
    return numpy.array([bits], dtype=numpy.uint32).view(numpy.float32)[0]


def clearance(asm, resolution, min_gap, initial_capacity=None):
    """Pairs of visible instances of the 3D assembly `asm` that come closer than `min_gap` on the lattice at `resolution`
    (the module's docstring defines the lattice, the windows, what "near" means and what `separation` bounds) ->
    ClearanceReport.

    Raises ValueError as `interference` does, and for a min_gap that is not a finite number >= 0.  `initial_capacity`
    caps the first guess of every cell list (rows); lists that overflow are regrown, so it changes how often the
    traversal runs, never the result."""
    instances = cells.visible(asm, resolution)
    t = half_gap(min_gap)
    corner, step, dims = cells.checked_lattice(instances, resolution, grow=float(t))
    named = [Instance(i.name, i) for i in instances]
    empty = ClearanceReport(named, corner, step, dims, min_gap, [], 0, 0)
    if len(instances) < 2:
        return empty
    side = cells.top_side(dims)
    wins = windows(instances, corner, step, dims, t)
    top = cells.cell_rows(wins, dims, side)
    if len(top) == 0:
        return empty

    def thr(child):
        return numpy.float32((float(t) + child * float(step) * math.sqrt(3) / 2) * (1 + 2.0 ** -10))

    evaluations, acc, traversals = cells.traverse(
        instances, top, side, corner, step, dims, initial_capacity, pair_dtype=_PAIR,
        pair_init={"lo": 0xffffffff, "key": 0xffffffff, "witness": 0xffffffffffffffff}, thr=thr, wins=wins,
        cells="hu_clearance_cells_indirect",
        finest=[("hu_clearance_leaf_indirect", (t,)), ("hu_clearance_witness_indirect", (t,))])   # the witness needs the leaf's keys
    pairs = []
    for fields, a in cells.pair_fields(acc, corner, step):
        w = int(a["witness"])
        witness = (w >> 32, (w >> 16) & 0xffff, w & 0xffff)
        pairs.append(NearMiss(*fields, _key_to_float(int(a["key"])), witness, cells.index_position(corner, step, witness)))
    return ClearanceReport(named, corner, step, dims, min_gap, pairs, evaluations, traversals)
