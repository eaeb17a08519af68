"""The outlines of an assembly's section, as vectors: per part, the closed contours of its cut on the plane.

`section_outlines(asm, plane, resolution) -> Outlines`.  The instances, the plane and the lattice are those of `section()`
(section.py): `corner`, `step`, `dims = (nu, nv)` and `first`.  Here every visible instance k is taken at the section's
samples AND a ring around them: the sample indices i = -1 .. nu, j = -1 .. nv, at `section.sample_positions` -- the same
formula, evaluated at -1 and at dims; no value is assumed.  s = (i + 1, j + 1) is the SHIFTED index, 0 .. nu + 1 by
0 .. nv + 1.  The ring lies half a step outside every projected box, so a part with an honest bounding box closes its
contours; one that still reaches the rim gives an open loop.

SQUARE (a, b), 0 <= a <= nu, 0 <= b <= nv, has the corner samples s = (a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1) and the
edges 0 bottom, 1 right, 2 top, 3 left, each from its lower-index sample p to its higher-index sample q.  Inside is w < 0,
strictly (a NaN is not inside).  Instance k crosses an edge when exactly one of p, q is inside, at t = w_p / (w_p - w_q)
-- one binary32 subtraction, one correctly rounded binary32 division; 0.5 where that is no number --, the vertex
(a + t, b) or (a, b + t) in shifted index coordinates; the two squares that share an edge compute it from the same bits.
A square has 0, 1 or 2 SEGMENTS per instance, each from a crossed edge to a crossed edge, directed with the inside on its
left (u to the right, v up): material runs counter-clockwise, holes clockwise.  Diagonal inside corners give two
segments, each cutting off one inside corner: they are never joined across the square.  `segments` holds them as records
(SEGMENT), sorted by (k, b, a, e_from); `stitch` joins them into loops on the host, over exact keys.

It is computed sparsely on the device, with one synchronisation, by the traversal of `section()` over the lattice of
squares (csrc/instance_outline.hip): tiles of 8^k squares; a level evaluates each candidate at the centre of each of a
tile's 8 x 8 children -- of S squares: the sample index (a - 1) + S / 2 -- and keeps k when its window of squares
(`square_windows`) reaches the child and neither w >= r (outside at every corner sample) nor w <= -r (inside at every one),
r = `radius(S, step)`; a NaN keeps its candidate.  The finest tiles (8 x 8 squares) evaluate their 9 x 9 samples.
`cull=False` takes every square with every instance, on one level.  The culling assumes what `section()` assumes.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from . import section as _section
from ._instance_cells import Instance
from .section import Plane

_TILE = 8
MAX_SAMPLES_PER_AXIS = 65535        # the squares have one more index per axis, and a row 16 bits for it

# a segment as the device writes it: 16 bytes {a | b << 16, k | e_from << 8 | e_to << 16, t_from, t_to}
SEGMENT = numpy.dtype([("a", "<u2"), ("b", "<u2"), ("k", "u1"), ("e_from", "u1"), ("e_to", "u1"), ("unused", "u1"),
                       ("t_from", "<f4"), ("t_to", "<f4")])
assert SEGMENT.itemsize == 16

Loop = collections.namedtuple("Loop", "points closed area")
Loop.__doc__ = """One contour of an instance: `points`, float64 (m, 2) in plane coordinates about the origin (along u, along
v), in the segments' direction -- the inside on the left; `closed`: the last point joins the first (an open loop was cut
by the lattice's rim and lists both its ends); `area`: the shoelace area of the points, signed: positive round material,
negative round a hole."""


class Outlines(collections.namedtuple("Outlines", "instances plane corner step dims segments loops counts evaluations runs")):
    """`instances`, `plane`, `corner`, `step`, `dims`: as Section's; `segments`: the SEGMENT records sorted by
    (k, b, a, e_from); `loops[k]`: the Loops of instance k, each starting at its smallest (b, a, e_from) (an open one at
    its open end) and ordered by that key; `counts[k]`: the segments of instance k; `evaluations`: per-instance sample
    evaluations of the last traversal, on every level; `runs`: how often the traversal ran (0: no tile had a candidate)."""

    __slots__ = ()

    def points3d(self, loop):
        """float64 (m, 3): the loop's points in space, origin + u * pu + v * pv."""
        o, u, v = (x.astype(numpy.float64) for x in (self.plane.origin, self.plane.u, self.plane.v))
        p = numpy.asarray(loop.points, dtype=numpy.float64).reshape(-1, 2)
        return o + p[:, :1] * u + p[:, 1:] * v


def square_windows(wins):
    """int64[n, 2, 3]: the windows of section.windows (sample indices lo .. hi) as windows of squares: the samples'
    shifted indices are lo + 1 .. hi + 1, and the squares with such a corner are lo .. hi + 1.  An empty window stays empty."""
    out = numpy.array(wins, dtype=numpy.int64)
    out[:, 1, :2] += 1
    return out


def radius(child, step):
    """float32 r of a child tile of `child` squares (the module's docstring): its corner samples lie within
    child * step * sqrt(2) / 2 of its centre; r leaves the step * sqrt(2) / 2 and the 2^-10 that section.radius leaves."""
    return numpy.float32(((child + 1) * float(step) * math.sqrt(2) / 2) * (1 + 2.0 ** -10))


def sort_segments(records):
    """The records (SEGMENT) sorted by (k, b, a, e_from)."""
    records = numpy.asarray(records, dtype=SEGMENT)
    return records[numpy.lexsort((records["e_from"], records["a"], records["b"], records["k"]))]


_EDGE_STRIDE = 1 << 17


def edge_ids(a, b, e):
    """The lattice-wide id of edge `e` of square (a, b): its lower-index sample and whether it runs along u or along v --
    the same for both squares that share it."""
    a, b, e = numpy.asarray(a, numpy.int64), numpy.asarray(b, numpy.int64), numpy.asarray(e, numpy.int64)
    pa, pb = a + (e == 1), b + (e == 2)
    return ((pb * _EDGE_STRIDE + pa) << 1) | (e & 1)


def vertices(a, b, e, t):
    """float64 (..., 2): the crossing at `t` of edge `e` of square (a, b), in shifted index coordinates."""
    a, b, e = numpy.asarray(a, numpy.float64), numpy.asarray(b, numpy.float64), numpy.asarray(e, numpy.int64)
    t = numpy.asarray(t, numpy.float32).astype(numpy.float64)
    along_u = (e & 1) == 0
    return numpy.stack([a + numpy.where(along_u, t, e == 1), b + numpy.where(along_u, e == 2, t)], axis=-1)


def stitch(segments, n, first=(0.0, 0.0), step=1.0):
    """[the Loops of instance k for k < n] from segments sorted by (k, b, a, e_from): a segment is followed by the one of
    the same instance that starts from the edge it ends on -- exact keys (k, edge id), at most one segment ending on a
    key and one starting from it (ValueError else).  Chains with an end nothing continues (cut by the rim) come out as
    open loops, from their open start; every other loop starts at its smallest (b, a, e_from).  Points are
    first + step * (shifted index - 1)."""
    segments = numpy.asarray(segments, dtype=SEGMENT)
    m = len(segments)
    loops = [[] for _ in range(n)]
    if m == 0:
        return loops
    k = segments["k"].astype(numpy.int64)
    key_from = (k << 40) | edge_ids(segments["a"], segments["b"], segments["e_from"])
    key_to = (k << 40) | edge_ids(segments["a"], segments["b"], segments["e_to"])
    if len(numpy.unique(key_from)) != m or len(numpy.unique(key_to)) != m:
        raise ValueError("two segments of one instance start from, or end on, the same edge")
    order = numpy.argsort(key_from)
    at = numpy.searchsorted(key_from[order], key_to)
    at = numpy.minimum(at, m - 1)
    follower = numpy.where(key_from[order][at] == key_to, order[at], -1)      # the segment that continues each, or -1
    has_previous = numpy.zeros(m, dtype=bool)
    has_previous[follower[follower >= 0]] = True
    start = vertices(segments["a"], segments["b"], segments["e_from"], segments["t_from"])
    end = vertices(segments["a"], segments["b"], segments["e_to"], segments["t_to"])
    first, step = numpy.asarray(first, dtype=numpy.float64), float(step)
    seen = numpy.zeros(m, dtype=bool)
    follower = follower.tolist()
    found = []
    for closed, heads in ((False, numpy.flatnonzero(~has_previous).tolist()), (True, range(m))):
        for head in heads:
            if seen[head]:
                continue
            chain, s = [], head
            while s >= 0 and not seen[s]:
                seen[s] = True
                chain.append(s)
                s = follower[s]
            points = start[chain] if closed else numpy.concatenate([start[chain], end[chain[-1:]]])
            points = first + step * (points - 1.0)
            x, y = points[:, 0], points[:, 1]
            area = 0.5 * float(numpy.sum(x * numpy.roll(y, -1) - numpy.roll(x, -1) * y))
            found.append((int(k[head]), min(chain) if not closed else head, Loop(points, closed, area)))
    for instance, key, loop in sorted(found, key=lambda f: f[:2]):       # (sorted segments: an index orders as (b, a, e_from))
        loops[instance].append(loop)
    return loops


def checked_samples(resolution, dims):
    """ValueError for a section of more than MAX_SAMPLES_PER_AXIS samples along u or v."""
    if dims[0] > MAX_SAMPLES_PER_AXIS or dims[1] > MAX_SAMPLES_PER_AXIS:
        raise ValueError("resolution %g gives a section of %s samples: outlines take at most 65535 per axis" % (resolution, dims.tolist()))


def _empty(named, plane, corner, step, dims, n):
    return Outlines(named, plane, corner, step, tuple(int(d) for d in dims), numpy.zeros(0, dtype=SEGMENT), [[] for _ in range(n)],
                    numpy.zeros(n, dtype=numpy.int64), 0, 0)


def section_outlines(asm, plane, resolution, cull=True, initial_capacity=None, segment_capacity=None):
    """The outlines of the section of the 3D assembly `asm` on `plane` at `resolution` (the module's docstring) -> Outlines.

    `cull=False` evaluates every instance at every sample (the same segments, slower); `initial_capacity` caps the first
    guess of every tile list, as in section(); `segment_capacity` is the first capacity of the segment buffer (default: a
    guess from the lattice's perimeter) -- the traversal runs again when it was too small.  Raises the ValueErrors of
    section(), and ValueError for more than 65535 samples on an axis."""
    if not isinstance(plane, Plane):
        raise ValueError("section_outlines takes a codecad_amd.Plane, not %r" % (plane,))
    instances = cells.visible(asm, resolution)
    corner, step, dims, first, projected = _section.lattice(instances, plane, resolution)
    checked_samples(resolution, dims)
    n = len(instances)
    named = [Instance(i.name, i) for i in instances]
    wins = square_windows(_section.windows(projected, first, step, dims))
    squares = numpy.array([dims[0] + 1, dims[1] + 1, 1], dtype=numpy.int64)
    side = cells.top_side(squares, first=_TILE * _TILE, factor=_TILE) if cull else _TILE
    top = _section.top_tiles(wins, squares[:2], side, everywhere=not cull) if n else []
    if len(top) == 0:
        return _empty(named, plane, corner, step, dims, n)
    capacity = 8 * int(squares[0] + squares[1]) + 64 if segment_capacity is None else max(1, int(segment_capacity))
    evaluations, totals, runs, rows = cells.traverse_records(
        instances, top, side, corner, step, squares, initial_capacity, capacity, 4, thr=lambda child: radius(child, step),
        cells="hu_outline_tiles", leaf="hu_outline_leaf", wins=wins, factor=_TILE, frame=plane.frame())
    segments = sort_segments(rows.view(SEGMENT).reshape(-1))
    return Outlines(named, plane, corner, step, tuple(int(d) for d in dims), segments, stitch(segments, n, first, float(step)),
                    totals[1:].astype(numpy.int64), evaluations, runs)
