"""Interference between the instances of an assembly: which pairs overlap, and by how much.

`interference(asm, resolution) -> InterferenceReport`.  The answer is defined on a lattice of samples, densely: sample
(i, j, k) sits at `corner + step * (float)index` per axis in float32 (kernels.hpp sample(), the lattice of
oracle.grid_eval), and it is inside instance n when the tape of that instance alone, `nodes.make_program(
instance.shape())` (its placement inside the tape), gives w < 0 there -- strictly: surfaces that touch do not
interfere.  A pair's count, index sums and index box are, bit for bit, what evaluating every instance over the whole
lattice would give.

The lattice: step = float32(resolution); the union of the visible instances' bounding boxes [a, b] is covered by
dims = ceil((b - a) / step) cells of that size per axis, and the samples are their centres, corner = a + step / 2
(rounded to float32).

It is computed sparsely, on the device, one synchronisation in all (_instance_cells.py, csrc/instance_pairs.hip):
  * the lattice is cut into cubic cells of 4^k samples, each with a 64-bit mask of candidate instances; the host seeds
    the top level from the instances' bounding boxes (grown by one step) and keeps the cells with two candidates or more;
  * every coarser level evaluates each candidate at the centre of each child cell and drops it when the distance
    proves that it has no sample inside the child: w >= thr, thr = (side * step * sqrt(3) / 2) * (1 + 2^-10) for a
    child of `side` samples.  side * step * sqrt(3) / 2 is the bound k_classify uses for a cell of that size (a
    subdivision cell of side * step); the child's samples lie within (side - 1) * step * sqrt(3) / 2 of its centre,
    so the bound leaves step * sqrt(3) / 2 plus 2^-10 of itself for the rounding of the centre and of w.  Children
    with two candidates or more go on, compacted on the device;
  * the finest level (cells of 4^3 samples) evaluates every remaining candidate at every sample and adds each pair's
    samples inside both to its accumulators.
The list lengths stay on the device between levels; when a list overflowed its capacity the whole traversal is run
again with the sizes it reported.

The culling assumes what `subdivision()` assumes: every instance's distance is a lower bound on the true distance
(Lipschitz constant at most 1).  Shapes from `shapes.unsafe` may break that, and then pairs may be missed.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from ._instance_cells import MAX_INSTANCES, Instance, lattice  # noqa: F401
# the names these helpers had while they lived in this module stay importable from it
from ._instance_cells import (visible as _visible, top_side as _top_side, windows as _windows, cell_rows as _cell_rows,  # noqa: F401
                              top_cells as _top_cells, instance_tape as _instance_tape, device_table as _device_table,
                              levels as _levels)

_PAIR = numpy.dtype([("sums", "<u8", (4,)), ("lo", "<u4", (3,)), ("hi", "<u4", (3,)), ("pad", "<u4", (2,))])   # OverlapAcc


class Overlap(collections.namedtuple("Overlap", "i j count volume centroid index_box bounding_box index_sums")):
    """Samples inside both instances i < j: `count` of them, `volume` = count * step^3, their `centroid` (Vector), the
    min and max lattice index per axis (`index_box`, ((x, y, z), (x, y, z))), the same in world coordinates
    (`bounding_box`, the samples' positions) and the sums of their x, y, z indices (`index_sums`)."""

    __slots__ = ()


class InterferenceReport(collections.namedtuple("InterferenceReport",
                                                 "instances corner step dims pairs samples_evaluated traversals")):
    """`instances`: the visible instances in all_instances() order, as Instance(name, instance); `corner` (float32[3]),
    `step` (float32) and `dims` (int[3]): the lattice; `pairs`: an Overlap per pair with samples inside both, ordered by
    (i, j); `samples_evaluated`: per-instance sample evaluations the last traversal did, on every level; `traversals`:
    how often the traversal ran (more than once when a cell list overflowed its first capacity; 0 when no top-level
    cell had two candidates)."""

    __slots__ = ()


def interference(asm, resolution, initial_capacity=None):
    """Pairs of visible instances of the 3D assembly `asm` that share lattice samples at `resolution` (the module's
    docstring defines the lattice, what "inside" means and what the culling assumes) -> InterferenceReport.

    Raises ValueError for a 2D assembly, more than 64 visible instances or a resolution that is not a positive finite
    number.  `initial_capacity` caps the first guess of every cell list (rows); lists that overflow are regrown, so it
    changes how often the traversal runs, never the result."""
    instances = cells.visible(asm, resolution)
    corner, step, dims = cells.checked_lattice(instances, resolution)
    named = [Instance(i.name, i) for i in instances]
    empty = InterferenceReport(named, corner, step, dims, [], 0, 0)
    if len(instances) < 2:
        return empty
    side = cells.top_side(dims)
    top = cells.top_cells(instances, corner, float(step), dims, side)
    if len(top) == 0:
        return empty

    def thr(child):
        return numpy.float32(child * float(step) * math.sqrt(3) / 2 * (1 + 2.0 ** -10))

    evaluations, acc, traversals = cells.traverse(
        instances, top, side, corner, step, dims, initial_capacity, pair_dtype=_PAIR, pair_init={"lo": 0xffffffff}, thr=thr,
        cells="hu_interference_cells_indirect", finest=[("hu_interference_leaf_indirect", ())])
    pairs = [Overlap(*fields) for fields, _ in cells.pair_fields(acc, corner, step)]
    return InterferenceReport(named, corner, step, dims, pairs, evaluations, traversals)
