"""Separation of the instances of an assembly: how far apart every pair of parts is, and where they come closest.

`separation(asm, resolution) -> SeparationReport`.  `clearance` (clearance.py) answers "which pairs come closer than this
gap"; this answers "how far apart are these two", for every pair, without a gap to choose.  Like every check here the
answer is defined on a lattice of samples, densely:
  * the instances and the lattice are those of `interference(asm, resolution)` (no margin around the boxes, no windows);
  * for a pair i < j, v(p) = max(w_i(p), w_j(p)) at every lattice sample p where both values are numbers (a sample with a
    NaN does not take part), w being each instance's own tape evaluated exactly as `interference` evaluates it;
  * the pair's `separation` is the least v as float32 (a zero as +0.0), None when no sample has both values; its
    `witness` the lexicographically smallest (x, y, z) index whose v equals it (-0.0 == +0.0), `witness_point` that
    sample's position.
EVERY pair is reported, ordered by (i, j).  Overlapping pairs have separation < 0: exactly the pairs `interference`
reports, whose samples inside both are those with v < 0.

What `separation` means, `gap_bounds`: for exact distance functions (spheres, boxes along a face normal) the true gap
between the two parts satisfies gap <= 2 * separation <= gap + step * sqrt(3), so
gap_bounds = (2 * separation - step * sqrt(3), 2 * separation), in float64, contains it.  The upper end is the triangle
inequality (a sample at distance w_i from one part and w_j from the other puts them at most w_i + w_j <= 2 v apart); the
lower end comes from the sample nearest to the mid-point of the closest pair of points, at most step * sqrt(3) / 2 from
it, where both distances are at most gap / 2 + step * sqrt(3) / 2.  For shapes whose w UNDERESTIMATES the distance (a
scaled or blended shape), 2 * separation can be smaller than the gap and the lower end can lie below it by as much: the
interval then still never overstates the gap, the safe direction for a clearance, but it is not a bound from below any
more.  Both ends hold only where the closest points lie inside the lattice, which they do for separate parts (the
mid-point lies between the boxes); for an overlapping pair the number is a depth, not a gap.

It is computed sparsely, on the device, one synchronisation in all (csrc/instance_gap.hip), by the traversal under
`interference` (_instance_cells.py) with a pruning rule of its own, a BRANCH AND BOUND:
  * the top level is every cell of the top side with every instance a candidate; the top side is the smallest 16 * 4^k
    that gives at most _MAX_TOP_CELLS cells (the first level knows no bound yet and keeps every child, so it is kept
    small; the result does not depend on it);
  * per level boundary there is an array of bounds U_0 .. U_L, [n][n] order keys of float32 values, U_0 "nothing known".
    Level l starts from U_{l+1} = U_l, prunes with U_l only and lowers U_{l+1}: what it prunes with is final when it
    reads it, so the rows, the evaluations and the results are the same on every run;
  * a level evaluates every candidate of a parent at one lattice sample q of each child (side s): the sample at
    min(first + s / 2, dims - 1) per axis.  v(q) is the value at a sample, so it bounds the pair's least v from above
    whatever the fields are, and lowers U_{l+1}.  Every sample of the child lies within (s / 2) * step * sqrt(3) of q;
    with r = float32((s / 2) * step * sqrt(3) * (1 + 2^-10)) the pair is DROPPED in the child iff (v(q) - U_l[i][j]) > r in
    float32 (the subtraction first; strictly, so that ties survive; a NaN keeps the pair).  The child keeps the union
    of the bits of its kept pairs and is listed when there is one;
  * the finest level (cells of 4^3 samples) evaluates every candidate at every sample and lowers the final array; the
    coarser levels' samples are lattice samples too, so the final bound is the dense minimum.  A second launch over
    the same cells evaluates again and takes, per pair, the least packed index x << 32 | y << 16 | z whose v has the
    final key: a sample that attains the minimum is in a kept child of every level, since v(q) <= v + r there.
`samples_evaluated` counts every level and both launches, `level_rows` the rows each level listed (the last the cells of
4^3 samples).  The pruning assumes what `interference` assumes: every instance's distance has Lipschitz constant at
most 1.  More than 64 instances, 2D assemblies and several devices are not handled.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from ._instance_cells import Instance

_MAX_TOP_CELLS = 512        # cells of the top level at most: it has no bound yet and keeps every child
_WORD = numpy.dtype([("w", "<u8")])     # the accumulators are read as words (instance_gap.hip GapLayout says what lies where)


class PairSeparation(collections.namedtuple("PairSeparation", "i j separation witness witness_point gap_bounds")):
    """The instances i < j: `separation` (float32), the least v = max(w_i, w_j) over the lattice, `witness`, the
    lexicographically smallest (x, y, z) index whose v equals it, `witness_point`, that sample's position (Vector), and
    `gap_bounds`, (2 * separation - step * sqrt(3), 2 * separation) in float64, which contains the true gap of exact
    distance functions (the module's docstring derives it and says what it is worth for others).  All four are None
    for a pair without a sample where both values are numbers."""

    __slots__ = ()


class SeparationReport(collections.namedtuple("SeparationReport",
                                              "instances corner step dims pairs samples_evaluated traversals level_rows")):
    """As interference.InterferenceReport, with `pairs`: a PairSeparation for EVERY pair, ordered by (i, j), and
    `level_rows`: the rows each level of the last traversal listed."""

    __slots__ = ()


def top_side(dims):
    """The side of the top level's cells: the smallest 16 * 4^k with at most _MAX_TOP_CELLS of them."""
    return cells.top_side(dims, most=_MAX_TOP_CELLS)


top_rows = cells.all_rows


def radius(child, step):
    """r of a child of `child` samples a side: a little more than the farthest one of its samples lies from q."""
    return numpy.float32((child // 2) * float(step) * math.sqrt(3) * (1 + 2.0 ** -10))


def key_to_float(key):
    """The float32 of an order key (instance_gap.hip order_key), None for the key of all ones: no sample."""
    if key == 0xffffffff:
        return None
    bits = key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff
    return numpy.array([bits], dtype=numpy.uint32).view(numpy.float32)[0]


def gap_bounds(value, step):
    """(2 * separation - step * sqrt(3), 2 * separation) in float64."""
    return (2.0 * float(value) - float(step) * math.sqrt(3), 2.0 * float(value))


def _separation(asm, resolution, initial_capacity=None, side=None):
    """separation(), from cells of `side` samples when it is given (16 * 4^k)."""
    instances = cells.visible(asm, resolution)
    corner, step, dims = cells.checked_lattice(instances, resolution)
    named = [Instance(i.name, i) for i in instances]
    n = len(instances)
    if n < 2:
        return SeparationReport(named, corner, step, dims, [], 0, 0, ())
    side = top_side(dims) if side is None else int(side)
    top = top_rows(n, dims, side)
    n_levels = len(cells.levels(side, len(top), None)[0])
    # [n * n uint64 witnesses | n_levels + 2 arrays of n * n uint32 keys | n_levels uint32 rows], all ones to begin with
    nbytes = 8 * n * n + 4 * (n_levels + 2) * n * n + 4 * n_levels
    evaluations, acc, traversals = cells.traverse(
        instances, top, side, corner, step, dims, initial_capacity, pair_dtype=_WORD, pair_init={"w": 0xffffffffffffffff},
        thr=lambda child: radius(child, step), cells="hu_separation_cells", cells_extra=(side,),
        finest=[("hu_separation_leaf", (side,)), ("hu_separation_witness", (side,))],     # the witness needs the leaf's keys
        accumulators=-(-nbytes // 8))
    raw = acc.view(numpy.uint8)
    witnesses = raw[:8 * n * n].view(numpy.uint64).reshape(n, n)
    words = raw[8 * n * n:nbytes].view(numpy.uint32)
    final = words[(n_levels + 1) * n * n:(n_levels + 2) * n * n].reshape(n, n)
    level_rows = tuple(int(v) for v in words[(n_levels + 2) * n * n:])
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            value = key_to_float(int(final[i, j]))
            if value is None:
                pairs.append(PairSeparation(i, j, None, None, None, None))
                continue
            w = int(witnesses[i, j])
            witness = (w >> 32, (w >> 16) & 0xffff, w & 0xffff)
            pairs.append(PairSeparation(i, j, value, witness, cells.index_position(corner, step, witness), gap_bounds(value, step)))
    return SeparationReport(named, corner, step, dims, pairs, evaluations, traversals, level_rows)


def separation(asm, resolution, initial_capacity=None):
    """The least v = max(w_i, w_j) of every pair of visible instances of the 3D assembly `asm` on the lattice of
    `interference(asm, resolution)`, and the sample that attains it (the module's docstring defines them, says what the
    numbers bound and what the traversal assumes) -> SeparationReport.

    Raises ValueError as `interference` does.  Fewer than two visible instances give a report without pairs and no
    traversal.  `initial_capacity` caps the first guess of every cell list (rows); lists that overflow are regrown, so it
    changes how often the traversal runs, never the result."""
    return _separation(asm, resolution, initial_capacity)
