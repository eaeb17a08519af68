"""The surface of every part of an assembly, as placed: one triangle mesh per visible instance, all on one lattice.

`assembly_meshes(asm, resolution) -> Meshes`.  The instances and the lattice are those of `interference()`
(_instance_cells.py): `visible`, then `checked_lattice` giving `corner`, `step` and `dims = (nx, ny, nz)`.  Here every visible
instance k is taken at those samples AND a ring around them: the sample indices -1 .. nx by -1 .. ny by -1 .. nz.
s = index + 1 is the SHIFTED index, 0 .. dims + 1 per axis, and a sample sits at `corner + step * ((float)s - 1.0f)` per axis in
binary32, one multiplication and one addition -- for s >= 1 that is sample() of kernels.hpp bit for bit, so the samples
0 .. dims - 1 are exactly those of `interference()` and `assembly_mass_properties()`; no value is assumed on the ring.  The
ring lies half a step outside every bounding box, so a part with an honest box has a closed surface.

CUBE (a, b, c), 0 <= a <= nx and likewise b and c, has its corner m at the shifted index (a, b, c) + CORNERS[m] and its edges
EDGES[e], the numbering of tools/gen_mc_table.py.  Inside is w < 0, strictly (a NaN is not inside; the mesher of one shape,
mesh.hip, uses <=).  Bit m of a cube's case is set when its corner m is inside, and its triangles are kMcTriangles[case] of
csrc/mc_table.hpp, in the table's order and with its winding (anticlockwise seen from outside the part); degenerate
triangles are kept.  An edge is crossed when exactly one end is inside, at t = w_p / (w_p - w_q), p the end with the LOWER
lattice index along the edge's axis whatever direction EDGES lists it in -- one binary32 subtraction and one correctly
rounded binary32 division; 0.5 where that is no number --, so both cubes that share an edge compute t from the same bits.
`triangles` holds the records (TRIANGLE: the cube, the instance, the triangle's number within its case, the case, its three
edges and their three t), sorted by (k, c, b, a, which); `Meshes.mesh(k)` welds them on the host, over exact keys.

It is computed sparsely on the device, with one synchronisation, by the traversal of `interference()` over the lattice of
cubes (csrc/instance_mesh.hip): cells of 4^k cubes; a level evaluates each candidate at the centre of each of a cell's 4^3
children -- of S cubes a side: the shifted index a + S / 2 per axis -- and keeps k when its window of cubes
(`cube_windows`) reaches the child and neither w >= r (outside at every corner sample) nor w <= -r (inside at every one),
r = `radius(S, step)`; a NaN keeps its candidate.  The finest cells (4^3 cubes) evaluate their 5^3 samples.  `cull=False`
takes every cube with every instance, on one level.  The culling assumes what `interference()` assumes: |w| is no more than
the distance to the surface, on both sides of it.  `evaluations` counts, per level of cells, the children inside the lattice
times their parent's candidates and, per finest cell, its candidates times those of its 5^3 samples that exist (shifted
index <= dims + 1 per axis).
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from ._instance_cells import Instance

_CELL = 4
MAX_SAMPLES_PER_AXIS = 65535        # the cubes have one more index per axis, and a row 16 bits for it

# the numbering of tools/gen_mc_table.py: a cube's corners, and its edges as pairs of corners
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
# per edge, its end with the lower lattice index (as an offset from the cube's corner 0) and the axis it runs along
EDGE_LOWER = numpy.array([numpy.minimum(CORNERS[p], CORNERS[q]) for p, q in EDGES], dtype=numpy.int64)
EDGE_AXIS = numpy.array([int(numpy.argmax(numpy.abs(numpy.subtract(CORNERS[p], CORNERS[q])))) for p, q in EDGES], dtype=numpy.int64)

# a triangle as the device writes it: 32 bytes {a | b << 16, c | k << 16 | which << 24, case | e0 << 8 | e1 << 16 | e2 << 24, 0,
# t0, t1, t2, 0}
TRIANGLE = numpy.dtype([("a", "<u2"), ("b", "<u2"), ("c", "<u2"), ("k", "u1"), ("which", "u1"), ("case", "u1"), ("e", "u1", (3,)),
                        ("zero", "<u4"), ("t", "<f4", (3,)), ("unused", "<u4")])
assert TRIANGLE.itemsize == 32

_KEY_STRIDE = 1 << 17


def vertex_keys(records):
    """int64 (m, 3): per triangle corner, the lattice edge it lies on -- the shifted index of the edge's lower end and its
    axis --, the same for every cube that shares the edge."""
    records = numpy.asarray(records, dtype=TRIANGLE)
    e = records["e"].astype(numpy.int64)
    low = numpy.stack([records["a"], records["b"], records["c"]], axis=-1).astype(numpy.int64)[:, None, :] + EDGE_LOWER[e]
    return (((low[..., 2] * _KEY_STRIDE + low[..., 1]) * _KEY_STRIDE + low[..., 0]) << 2) | EDGE_AXIS[e]


def vertex_points(records):
    """float64 (m, 3, 3): the triangles' corners in shifted index coordinates: an edge's lower end plus t along its axis,
    the float32 t widened."""
    records = numpy.asarray(records, dtype=TRIANGLE)
    e = records["e"].astype(numpy.int64)
    low = numpy.stack([records["a"], records["b"], records["c"]], axis=-1).astype(numpy.float64)[:, None, :] + EDGE_LOWER[e]
    t = records["t"].astype(numpy.float64)
    return low + t[..., None] * (EDGE_AXIS[e][..., None] == numpy.arange(3))


def weld(records, corner=(0.0, 0.0, 0.0), step=1.0):
    """(vertices float64 (m, 3), triangles uint32 (t, 3)) of the records of ONE instance, in their order: a vertex is the
    lattice edge it lies on (`vertex_keys`), vertices are ordered by first use, and a position is
    float64(corner) + float64(step) * (shifted index - 1)."""
    records = numpy.asarray(records, dtype=TRIANGLE)
    if len(records) == 0:
        return numpy.zeros((0, 3), dtype=numpy.float64), numpy.zeros((0, 3), dtype=numpy.uint32)
    keys = vertex_keys(records).reshape(-1)
    unique, first, inverse = numpy.unique(keys, return_index=True, return_inverse=True)
    order = numpy.argsort(first, kind="stable")                 # the unique keys by first use
    rank = numpy.empty(len(unique), dtype=numpy.int64)
    rank[order] = numpy.arange(len(unique))
    points = vertex_points(records).reshape(-1, 3)[first[order]]
    corner = numpy.asarray(corner, dtype=numpy.float32).astype(numpy.float64)
    return corner + float(step) * (points - 1.0), rank[inverse.reshape(-1)].reshape(-1, 3).astype(numpy.uint32)


class Meshes(collections.namedtuple("Meshes", "instances corner step dims triangles counts evaluations runs")):
    """`instances`, `corner`, `step`, `dims`: as InterferenceReport's; `triangles`: the TRIANGLE records sorted by
    (k, c, b, a, which); `counts[k]`: the triangles of instance k; `evaluations`: per-instance sample evaluations of the
    last traversal, on every level; `runs`: how often the traversal ran (0: no cell had a candidate)."""

    __slots__ = ()

    def mesh(self, k):
        """(vertices float64 (m, 3), triangles uint32 (t, 3)) of instance k, welded over exact keys (`weld`)."""
        if not 0 <= k < len(self.instances):
            raise IndexError("instance %r of %d" % (k, len(self.instances)))
        start = int(numpy.sum(self.counts[:k]))
        return weld(self.triangles[start:start + int(self.counts[k])], self.corner, self.step)


def cube_windows(wins):
    """int64[n, 2, 3]: the windows of _instance_cells.windows (sample indices lo .. hi) as windows of cubes: the samples'
    shifted indices are lo + 1 .. hi + 1, and the cubes with such a corner are lo .. hi + 1."""
    out = numpy.array(wins, dtype=numpy.int64)
    out[:, 1, :] += 1
    return out


def radius(child, step):
    """float32 r of a child cell of `child` cubes a side (the module's docstring): its corner samples lie within
    child * step * sqrt(3) / 2 of its centre; r leaves the step * sqrt(3) / 2 and the 2^-10 that the checks' cells leave."""
    return numpy.float32(((child + 1) * float(step) * math.sqrt(3) / 2) * (1 + 2.0 ** -10))


def sort_triangles(records):
    """The records (TRIANGLE) sorted by (k, c, b, a, which)."""
    records = numpy.asarray(records, dtype=TRIANGLE)
    return records[numpy.lexsort((records["which"], records["a"], records["b"], records["c"], records["k"]))]


def top_cells(wins, cubes, side, everywhere=False):
    """uint32[m, 4] rows of the top level: the cells of `side` cubes that a window reaches, each with the instances whose
    windows do; `everywhere`: every cell with every instance."""
    return cells.all_rows(len(wins), cubes, side) if everywhere else cells.cell_rows(wins, cubes, side, least=1)


def first_capacity(wins):
    """The first capacity of the triangle buffer: per instance four triangles for every cube on the faces of its window."""
    ext = numpy.maximum(wins[:, 1] - wins[:, 0] + 1, 0)
    return int(4 * (ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 0] * ext[:, 2]).sum()) + 64


def assembly_meshes(asm, resolution, cull=True, initial_capacity=None, triangle_capacity=None):
    """The surface meshes of the visible instances of the 3D assembly `asm` at `resolution` (the module's docstring) -> Meshes.

    `cull=False` evaluates every instance at every sample (the same triangles, slower); `initial_capacity` caps the first
    guess of every cell list, as in interference(); `triangle_capacity` is the first capacity of the triangle buffer
    (default: `first_capacity` of the windows) -- the traversal runs again when it was too small.  Raises the ValueErrors
    of interference(), and ValueError for more than 65535 samples on an axis."""
    instances = cells.visible(asm, resolution)
    corner, step, dims = cells.checked_lattice(instances, resolution)
    if max(dims) > MAX_SAMPLES_PER_AXIS:
        raise ValueError("resolution %g gives a lattice of %s samples: meshes take at most 65535 per axis" % (resolution, dims.tolist()))
    n = len(instances)
    named = [Instance(i.name, i) for i in instances]
    empty = Meshes(named, corner, step, dims, numpy.zeros(0, dtype=TRIANGLE), numpy.zeros(n, dtype=numpy.int64), 0, 0)
    if n == 0:
        return empty
    wins = cube_windows(cells.windows(instances, corner, float(step), dims))
    cubes = dims + 1
    side = cells.top_side(cubes) if cull else _CELL
    top = top_cells(wins, cubes, side, everywhere=not cull)
    if len(top) == 0:
        return empty
    capacity = first_capacity(wins) if triangle_capacity is None else max(1, int(triangle_capacity))
    evaluations, totals, runs, rows = cells.traverse_records(
        instances, top, side, corner, step, cubes, initial_capacity, capacity, 8, thr=lambda child: radius(child, step),
        cells="hu_mesh_cells", leaf="hu_mesh_leaf_instances", wins=wins, factor=_CELL)
    return Meshes(named, corner, step, dims, sort_triangles(rows.view(TRIANGLE).reshape(-1)), totals[1:].astype(numpy.int64), evaluations, runs)
