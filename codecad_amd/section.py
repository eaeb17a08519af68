"""A planar section of an assembly: which part owns each point of a cut, and where parts overlap on it.

`section(asm, plane, resolution) -> Section`.  The answer is defined on a 2D lattice of samples on the plane, densely.
With the plane's `origin` and unit vectors `u`, `v` (`u x v = normal`) as float32 triples, `corner` the float32 position
of sample (0, 0) and `step = float32(resolution)`, sample (i, j) sits at

    p_c = (corner_c + u_c * (step * (float)i)) + v_c * (step * (float)j)        per coordinate c,

every operation rounded in binary32 and none contracted (`sample_positions`; csrc/instance_section.hip plane_point).
For `Plane.xy`, `Plane.xz` and `Plane.yz` that is `corner + step * (float)index` on two axes, the lattice of
`interference()` and `oracle.grid_eval`.  With w_k(p) what the tape of instance k alone gives there,
  * `part_ids[j, i]` is the lowest k with w_k(p) < 0 -- strictly, as in `interference()`: a surface through a sample
    does not own it -- or -1, and `inside_count[j, i]` the number of such k;
  * with `distance=True`, `distance[j, i]` is min_k w_k(p), the hardware minimum chain, and `nearest[j, i]` the LOWEST
    k that attains it, the tie rule of `rendering.render_assembly_pixels`;
  * `parts` and `overlaps` count, exactly, the samples inside each instance and inside both of each pair.
All of it is, bit for bit, what evaluating every instance at every sample gives (`cull=False` does just that).

The lattice: the eight corners of every visible instance's bounding box are projected onto (u, v) about the origin, in
float64; their min-max rectangle [a, b] is covered by dims = ceil((b - a) / step) cells per axis (at least one), the
samples are the cells' centres, and `corner` is origin + u * (a_u + step / 2) + v * (a_v + step / 2), rounded once.

It is computed sparsely on the device, with one synchronisation, by the traversal under `interference()`
(_instance_cells.py) one dimension down: the lattice is cut into square tiles of 8^k samples with a 64-bit mask of
candidate instances each.  The host seeds the top tiles from the instances' projected index windows (an instance whose box
lies on one side of the plane, by more than a step, is inside nowhere); every coarser level evaluates each candidate at
the centre of each of a tile's 8 x 8 children -- the position formula at the half-integer indices x + (s - 1) / 2 for
a child of s samples from x -- and keeps candidate k in the child when
    w_k < r                and k's window reaches the child: it may be inside somewhere in the child, or
    w_k <= m + 2 r         (`distance=True` only; m the least w there): it may be the least, or tie, somewhere in it,
with r = (s * step * sqrt(2) / 2) * (1 + 2^-10).  The child's samples lie within (s - 1) * step * sqrt(2) / 2 of its
centre, so r leaves step * sqrt(2) / 2 and 2^-10 of itself for the rounding of positions and of w, as the cell levels
of `interference()` do.  A value that is no number keeps its candidate.  The finest level (tiles of 8 x 8 samples)
evaluates what is left at every sample.

The culling assumes what `interference()` assumes: a distance with Lipschitz constant at most 1 and a bounding box that
holds the instance.  Shapes from `shapes.unsafe` may break the first, and then the maps may differ from `cull=False`.
"""
import collections
import ctypes
import math

import numpy

from . import _instance_cells as cells
from . import hip_util
from . import util
from .hip_util import manager as hip_manager
from ._instance_cells import Instance
from .interference import _PAIR

MAX_SAMPLES = 1 << 28
_TILE = 8                   # samples per axis of a finest tile, and children per axis of a coarser one


class Plane(collections.namedtuple("Plane", "origin u v normal")):
    """A plane with a frame: `origin`, unit vectors `u` and `v` spanning it and `normal = u x v`, float32 triples.
    `Plane(origin, normal, u=None)`: the normal is normalised and `u` (default: the coordinate axis least aligned with
    the normal) projected into the plane and normalised, in float64; `v = normal x u`; each is rounded once to float32.
    ValueError for a zero or non-finite normal or origin, or a `u` parallel to the normal."""

    __slots__ = ()

    def __new__(cls, origin, normal, u=None):
        o = numpy.array([float(c) for c in origin], dtype=numpy.float64)
        n = numpy.array([float(c) for c in normal], dtype=numpy.float64)
        if o.shape != (3,) or n.shape != (3,) or not (numpy.isfinite(o).all() and numpy.isfinite(n).all()):
            raise ValueError("a plane needs a finite 3D origin and normal")
        length = math.sqrt(float(n @ n))
        if length == 0:
            raise ValueError("a plane's normal must not be zero")
        n = n / length
        if u is None:
            a = numpy.zeros(3)
            a[int(numpy.argmin(numpy.abs(n)))] = 1.0
        else:
            a = numpy.array([float(c) for c in u], dtype=numpy.float64)
            if a.shape != (3,) or not numpy.isfinite(a).all():
                raise ValueError("a plane's u must be a finite 3D vector")
        size = math.sqrt(float(a @ a))
        a = a - (a @ n) * n
        length = math.sqrt(float(a @ a))
        if size == 0 or length <= 1e-6 * size:
            raise ValueError("a plane's u must not be parallel to its normal")
        a = a / length
        b = numpy.cross(n, a)
        f32 = lambda x: (x + 0.0).astype(numpy.float32)       # (+ 0.0: no negative zeros)
        return super().__new__(cls, f32(o), f32(a), f32(b), f32(n))

    @classmethod
    def xy(cls, z=0.0):
        """u = +x, v = +y, seen from +z."""
        return cls((0, 0, z), (0, 0, 1), (1, 0, 0))

    @classmethod
    def xz(cls, y=0.0):
        """u = +x, v = +z, seen along +y like the ray-cast pictures."""
        return cls((0, y, 0), (0, -1, 0), (1, 0, 0))

    @classmethod
    def yz(cls, x=0.0):
        """u = +y, v = +z, seen from +x."""
        return cls((x, 0, 0), (1, 0, 0), (0, 1, 0))

    def frame(self):
        """(u, v) as the entry points of the section and of its outlines take them: two float[3]."""
        return tuple((ctypes.c_float * 3)(*(float(c) for c in x)) for x in (self.u, self.v))


# the samples inside one instance (`parts`) or inside both of a pair (`overlaps`)
Cut = collections.namedtuple("Cut", "i j count area centroid index_box bounding_box index_sums")
Cut.__doc__ = """Samples of the section inside instance i (`parts`: j == i) or inside both i < j (`overlaps`): `count` of
them, `area` = count * step^2, their `centroid` (a 3D Vector on the plane), the min and max sample index (`index_box`,
((i, j), (i, j)) along u and v), the same in plane coordinates about the origin (`bounding_box`, ((u, v), (u, v))) and the
sums of their indices (`index_sums`)."""


class Section(collections.namedtuple("Section", "instances plane corner step dims part_ids inside_count distance nearest "
                                                "parts overlaps evaluations runs")):
    """`instances`: the visible instances in all_instances() order, as Instance(name, instance); `plane`; `corner`
    (float32[3]), `step` (float32) and `dims` (samples along u, along v): the lattice; the maps `part_ids` (int32),
    `inside_count` (uint8), `distance` (float32) and `nearest` (int32; both None without distance=True), of shape
    (dims v, dims u); `parts`: a Cut per instance with samples inside it; `overlaps`: a Cut per pair with samples inside
    both, ordered by (i, j); `evaluations`: per-instance sample evaluations of the last traversal, on every level;
    `runs`: how often the traversal ran (more than once when a tile list overflowed; 0 when no tile had a candidate)."""

    __slots__ = ()

    def position(self, i, j):
        """The 3D point of sample (i, j) -- along u, along v --, as the kernels compute it."""
        return util.Vector(*(float(c) for c in sample_positions(self.plane, self.corner, self.step, [i], [j])[0, 0]))

    def part_at(self, i, j):
        """The Instance that owns sample (i, j), or None."""
        k = int(self.part_ids[j, i])
        return None if k < 0 else self.instances[k]


def sample_positions(plane, corner, step, i, j):
    """float32 (len(j), len(i), 3): the positions of the samples at the indices `i` (along u) and `j` (along v) -- whole
    numbers for samples, half-integers for the centres of tiles --, operation for operation what the kernels compute."""
    step = numpy.float32(step)
    a = (step * numpy.asarray(i, dtype=numpy.float32))[None, :, None]
    b = (step * numpy.asarray(j, dtype=numpy.float32))[:, None, None]
    corner = numpy.asarray(corner, dtype=numpy.float32)
    return ((corner + plane.u * a) + plane.v * b).astype(numpy.float32)


def _projected(instances, plane):
    """float64 (n, 8, 3): the corners of every instance's bounding box in plane coordinates (along u, v, the normal)."""
    frame = numpy.stack([plane.u, plane.v, plane.normal]).astype(numpy.float64)
    out = numpy.zeros((len(instances), 8, 3))
    for n, inst in enumerate(instances):
        box = inst.shape().bounding_box()
        a, b = numpy.array(tuple(box.a), dtype=numpy.float64), numpy.array(tuple(box.b), dtype=numpy.float64)
        if not (numpy.isfinite(a).all() and numpy.isfinite(b).all()):
            raise ValueError("a section needs instances with finite bounding boxes")
        corners = numpy.array([[(a, b)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])
        out[n] = (corners - plane.origin.astype(numpy.float64)) @ frame.T
    return out


def lattice(instances, plane, resolution):
    """(corner float32[3], step float32, dims int64[2], first float64[2], projected): the lattice over the instances'
    projected boxes; `first` is sample (0, 0) in plane coordinates.  One sample at the origin for no instance at all."""
    step = numpy.float32(resolution)
    projected = _projected(instances, plane)
    if len(instances):
        a, b = projected[:, :, :2].min(axis=(0, 1)), projected[:, :, :2].max(axis=(0, 1))
        dims = numpy.maximum(1, numpy.ceil((b - a) / float(step))).astype(numpy.int64)
        first = a + float(step) / 2
    else:
        dims, first = numpy.ones(2, numpy.int64), numpy.zeros(2)
    if dims[0] > 65536 or dims[1] > 65536 or int(dims[0]) * int(dims[1]) > MAX_SAMPLES:
        raise ValueError("resolution %g gives a section of %s samples: at most 65536 per axis and 2^28 in all" % (resolution, dims.tolist()))
    o, u, v = (x.astype(numpy.float64) for x in (plane.origin, plane.u, plane.v))
    corner = (o + u * first[0] + v * first[1]).astype(numpy.float32)
    return corner, step, dims, first, projected


def windows(projected, first, step, dims):
    """int64[n, 2, 3]: per instance, the first and last sample index along u and v (the third is 0) of its projected box
    grown by a step, clipped to the lattice; an instance whose box lies on one side of the plane by more than a step gets
    an empty window (lo > hi): it is inside at no sample."""
    step = float(step)
    out = numpy.zeros((len(projected), 2, 3), dtype=numpy.int64)
    for n, corners in enumerate(projected):
        if corners[:, 2].min() > step or corners[:, 2].max() < -step:
            out[n, 0, :2], out[n, 1, :2] = 65536, 0
            continue
        lo = numpy.floor((corners[:, :2].min(axis=0) - first - step) / step)
        hi = numpy.ceil((corners[:, :2].max(axis=0) - first + step) / step)
        out[n, 0, :2] = numpy.clip(lo, 0, dims - 1)
        out[n, 1, :2] = numpy.clip(hi, 0, dims - 1)
    return out


def top_tiles(wins, dims, side, everywhere=False):
    """Rows of the top level: tiles of `side` samples that a window reaches, with the instances whose windows do;
    `everywhere`: every tile of the lattice with every instance."""
    dims3 = numpy.array([dims[0], dims[1], 1], dtype=numpy.int64)
    if everywhere:
        wins = numpy.zeros_like(wins)
        wins[:, 1] = dims3 - 1
    return cells.cell_rows(wins, dims3, side, least=1)


def radius(child, step):
    """float32 r of a child tile of `child` samples (the module's docstring)."""
    return numpy.float32(child * float(step) * math.sqrt(2) / 2 * (1 + 2.0 ** -10))


def _cuts(acc, first, step, plane, corner):
    o = corner.astype(numpy.float64)
    u, v = plane.u.astype(numpy.float64), plane.v.astype(numpy.float64)
    parts, overlaps = [], []
    for f, _ in cells.pair_fields(acc, numpy.array([first[0], first[1], 0.0]), step, diagonal=True):
        along = [float(step) * f.index_sums[k] / f.count for k in range(2)]
        cut = Cut(f.i, f.j, f.count, f.count * float(step) ** 2, util.Vector(*(o + u * along[0] + v * along[1])),
                  (f.index_box[0][:2], f.index_box[1][:2]), (tuple(f.bounding_box.a)[:2], tuple(f.bounding_box.b)[:2]), f.index_sums[:2])
        (parts if f.i == f.j else overlaps).append(cut)
    return parts, overlaps


def section(asm, plane, resolution, distance=False, cull=True, initial_capacity=None):
    """The section of the 3D assembly `asm` on `plane` at `resolution` (the module's docstring defines the lattice, the
    maps and what the culling assumes) -> Section.

    `distance=True` also fills `distance` and `nearest`; `cull=False` evaluates every instance at every sample (the same
    arrays and accumulators, slower); `initial_capacity` caps the first guess of every tile list, as in interference().
    Raises ValueError for what interference() refuses (not an assembly, 2D, more than 64 visible instances, a bad
    resolution), for non-finite boxes and for more than 65536 samples on an axis or 2^28 in all."""
    if not isinstance(plane, Plane):
        raise ValueError("section takes a codecad_amd.Plane, not %r" % (plane,))
    instances = cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    n = len(instances)
    shape = (int(dims[1]), int(dims[0]))
    named = [Instance(i.name, i) for i in instances]
    wins = windows(projected, first, step, dims)
    dims3 = numpy.array([dims[0], dims[1], 1], dtype=numpy.int64)
    side = cells.top_side(dims3, first=_TILE * _TILE, factor=_TILE) if cull else _TILE
    top = top_tiles(wins, dims, side, everywhere=distance or not cull) if n else []
    if len(top) == 0:
        return Section(named, plane, corner, step, tuple(int(d) for d in dims), numpy.full(shape, -1, numpy.int32),
                       numpy.zeros(shape, numpy.uint8), numpy.full(shape, numpy.inf, numpy.float32) if distance else None,
                       numpy.full(shape, -1, numpy.int32) if distance else None, [], [], 0, 0)
    queue = hip_manager.queue
    # the maps, prefilled once: a traversal that overflowed wrote final values where it wrote at all
    part_ids = hip_util.Buffer(numpy.int32, shape, queue=queue)
    part_ids.enqueue_fill(0xff)              # -1
    inside_count = hip_util.Buffer(numpy.uint8, shape, queue=queue)
    inside_count.enqueue_fill(0)
    maps = [part_ids, inside_count]
    if distance:        # (every sample lies in a surviving tile)
        maps += [hip_util.Buffer(numpy.float32, shape, queue=queue), hip_util.Buffer(numpy.int32, shape, queue=queue)]
    frame = plane.frame() + (int(bool(distance)),)
    pointers = tuple(m.device_ptr for m in maps) + ((None, None) if not distance else ())
    evaluations, acc, runs = cells.traverse(
        instances, top, side, corner, step, dims3, initial_capacity, pair_dtype=_PAIR, pair_init={"lo": 0xffffffff},
        thr=lambda child: radius(child, step), cells="hu_section_tiles", finest=[("hu_section_leaf", pointers)], wins=wins,
        factor=_TILE, frame=frame)
    got = [m.read().copy() for m in maps] + ([None, None] if not distance else [])
    for m in maps:
        m.release()
    parts, overlaps = _cuts(acc, first, step, plane, corner)
    return Section(named, plane, corner, step, tuple(int(d) for d in dims), *got, parts, overlaps, evaluations, runs)

