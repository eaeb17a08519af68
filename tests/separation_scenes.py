"""The scenarios of the separation tests (test_separation_host.py holds the traversal to the dense definition on the CPU;
test_gpu_separation.py holds the device to both; test_separation_edges_host.py and test_gpu_separation_edges.py do the
same for the scenarios at the edges of the branch and bound, at the end of this file) and their CPU reference, written from codecad_amd/separation.py's
definitions over the oracle:
  * the DENSE half (`dense`) evaluates every instance over the whole lattice (oracle.grid_eval) and gives, per pair, the
    order key of the least v = max(w_i, w_j) over the samples where both are numbers and the first sample, in (x, y, z)
    order, that attains it;
  * the TRAVERSAL half (`traverse`) applies the rows, the snapshot keys U_l and the drop rule level by level in float32,
    operation for operation as the kernels do, and gives the final keys and witnesses again, the evaluations and the
    rows every level listed.  It takes its values from the dense fields where there are some, and from
    oracle.evaluate_points at the samples' float32 positions where the lattice is too fine to evaluate densely.
"""
import collections
import functools
import math

import numpy

import codecad_amd as cc
from codecad_amd import shapes, nodes, _instance_cells
import oracle

import assembly_mass_scenes as mass_scenes

NOTHING = 0xffffffff                     # the key of "no sample"
Dense = collections.namedtuple("Dense", "keys witness inside_both")          # keys [n, n] uint32; {(i, j): (x, y, z)}; {(i, j): count}
Traversal = collections.namedtuple("Traversal", "keys witness evaluations level_rows side")


def order_keys(v):
    """uint32 keys that order as the float32 values do, either zero with the key of +0.0; a NaN gets NOTHING."""
    v = numpy.asarray(v, dtype=numpy.float32)
    bits = numpy.where(v == 0, numpy.float32(0), v).view(numpy.uint32)
    keys = numpy.where(bits & numpy.uint32(0x80000000), ~bits, bits | numpy.uint32(0x80000000))
    return numpy.where(numpy.isnan(v), numpy.uint32(NOTHING), keys).astype(numpy.uint32)


def key_value(keys):
    """The float32 of keys; NOTHING gives a NaN."""
    keys = numpy.asarray(keys, dtype=numpy.uint32)
    bits = numpy.where(keys & numpy.uint32(0x80000000), keys & numpy.uint32(0x7fffffff), ~keys)
    return bits.astype(numpy.uint32).view(numpy.float32)


def pair_value(wi, wj):
    """v = max(w_i, w_j) where both are numbers, else a NaN."""
    return numpy.where(numpy.isnan(wi) | numpy.isnan(wj), numpy.float32(numpy.nan), numpy.maximum(wi, wj)).astype(numpy.float32)


def dense(w):
    n = len(w)
    keys = numpy.full((n, n), NOTHING, dtype=numpy.uint32)
    witness, inside_both = {}, {}
    for i in range(n):
        for j in range(i + 1, n):
            k = order_keys(pair_value(w[i], w[j]))
            keys[i, j] = k.min()
            if keys[i, j] != NOTHING:
                witness[(i, j)] = tuple(int(c) for c in numpy.argwhere(k == keys[i, j])[0])      # C order is (x, y, z) order
            inside_both[(i, j)] = int(((w[i] < 0) & (w[j] < 0)).sum())
    return Dense(keys, witness, inside_both)


def top_side(dims, max_top_cells=512):
    side = 16
    while numpy.prod(-(-numpy.asarray(dims, dtype=numpy.int64) // side)) > max_top_cells:
        side *= 4
    return side


def radius(child, step):
    return numpy.float32((child / 2) * float(step) * math.sqrt(3) * (1 + 2.0 ** -10))


def field_values(w):
    """values(k, index[m, 3]) -> float32[m] from dense fields."""
    return lambda k, index: w[k][index[:, 0], index[:, 1], index[:, 2]]


def point_values(instances, corner, step):
    """values(k, index[m, 3]) -> float32[m] from the oracle at the samples' positions, computed as kernels.hpp sample()."""
    tapes = [nodes.make_program(i.shape()) for i in instances]
    corner, step = numpy.asarray(corner, dtype=numpy.float32), numpy.float32(step)

    def values(k, index):
        points = corner + step * index.astype(numpy.float32)
        assert points.dtype == numpy.float32
        return oracle.evaluate_points(tapes[k], points)[:, 3]
    return values


_LANES = numpy.arange(64)
_OFFSETS = numpy.stack([_LANES >> 4, (_LANES >> 2) & 3, _LANES & 3], axis=-1)      # lane = 16 x + 4 y + z


def _cells(values, n, origin, mask, child, dims):
    """The children (child >= 4, judged at q) or samples (child == 1) of the rows: (first index [m, 64, 3], live [m, 64],
    w [n, m, 64] with a NaN where an instance is no candidate, evaluations)."""
    first = origin[:, None, :] + _OFFSETS[None, :, :] * child
    live = (first < dims).all(axis=-1)
    q = numpy.minimum(first + child // 2, dims - 1)
    w = numpy.full((n,) + live.shape, numpy.nan, dtype=numpy.float32)
    evaluations = 0
    for k in range(n):
        at = (((mask >> numpy.uint64(k)) & numpy.uint64(1)) != 0)[:, None] & live
        if at.any():
            w[k][at] = values(k, q[at])
            evaluations += int(at.sum())
    return first, live, w, evaluations


def _pairs_of(mask, n):
    """The pairs i < j some row has both bits of, with the rows that do."""
    bits = [((mask >> numpy.uint64(k)) & numpy.uint64(1)) != 0 for k in range(n)]
    for i in range(n):
        if not bits[i].any():
            continue
        for j in range(i + 1, n):
            both = bits[i] & bits[j]
            if both.any():
                yield i, j, both


def traverse(values, n, dims, step, side=None, max_top_cells=512, dropped=numpy.greater, watch=None, listed=None):
    """`dropped(difference, r)` is the drop rule, strictly greater as the kernels have it (the edge tests show what another
    one would change); `watch(level, i, j, first, at, v, bound, difference, r)` sees every pair of every level: the first
    indices [m, 64, 3] of the children, which of them are live children of rows with both bits, and the float32 operands;
    `listed`, a list, gets the origins [m, 3] of the rows every level lists."""
    dims = numpy.asarray(dims, dtype=numpy.int64)
    side = top_side(dims, max_top_cells) if side is None else side
    counts = [int(-(-d // side)) for d in dims]
    origin = numpy.stack(numpy.meshgrid(*(numpy.arange(c, dtype=numpy.int64) * side for c in counts), indexing="ij"), axis=-1).reshape(-1, 3)
    mask = numpy.full(len(origin), (1 << n) - 1, dtype=numpy.uint64)
    keys = numpy.full((n, n), NOTHING, dtype=numpy.uint32)                    # U_0
    evaluations, level_rows, top = 0, [], side
    one = numpy.uint64(1)
    with numpy.errstate(invalid="ignore"):
        while side > 4:
            child = side // 4
            r = radius(child, step)
            first, live, w, count = _cells(values, n, origin, mask, child, dims)
            evaluations += count
            keep = numpy.zeros(live.shape, dtype=numpy.uint64)
            lowered = keys.copy()                                             # U_{l+1} starts as U_l; the level reads U_l only
            for i, j, both in _pairs_of(mask, n):
                at = both[:, None] & live
                v = pair_value(w[i], w[j])
                difference = v - key_value(keys[i, j])                        # float32 - float32, rounded once
                assert difference.dtype == numpy.float32
                kept = at & ~dropped(difference, r)                           # (a NaN keeps the pair)
                if watch is not None:
                    watch(len(level_rows), i, j, first, at, v, key_value(keys[i, j]), difference, r)
                keep[kept] |= (one << numpy.uint64(i)) | (one << numpy.uint64(j))
                lowered[i, j] = min(lowered[i, j], order_keys(v[at]).min())
            going = keep != 0
            origin, mask, keys = first[going], keep[going], lowered
            level_rows.append(len(origin))
            if listed is not None:
                listed.append(origin)
            side = child
        # the finest cells, twice: the least keys, then the witnesses
        first, live, w, count = _cells(values, n, origin, mask, 1, dims)
        evaluations += 2 * count
        final, witness = keys.copy(), {}
        packed = (first[..., 0] << 32) | (first[..., 1] << 16) | first[..., 2]
        found = []
        for i, j, both in _pairs_of(mask, n):
            at = both[:, None] & live
            k = numpy.where(at, order_keys(pair_value(w[i], w[j])), numpy.uint32(NOTHING))
            final[i, j] = min(final[i, j], k.min())
            found.append((i, j, k))
        for i, j, k in found:
            hit = (k == final[i, j]) & (k != NOTHING)
            if hit.any():
                p = int(packed[hit].min())
                witness[(i, j)] = (p >> 32, (p >> 16) & 0xffff, p & 0xffff)
    return Traversal(final, witness, evaluations, tuple(level_rows), top)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

SPHERES_GAP, BOXES_GAP = 0.3, 0.25


def _spheres():
    """Two balls of radius 1 on the x axis, 0.3 apart."""
    ball = shapes.sphere(r=1).make_part("ball")
    return cc.assembly("spheres", [ball, ball.translated(2.0 + SPHERES_GAP, 0, 0)])


def _boxes():
    """Two unit boxes face to face, 0.25 apart: the least v is attained on a whole plane of samples (ties)."""
    a = shapes.box(1, 1, 1).make_part("a")
    return cc.assembly("boxes", [a, a.translated_x(1.0 + BOXES_GAP)])


def _lens():
    """Two overlapping balls: a negative separation."""
    ball = shapes.sphere(r=1).make_part("ball")
    return cc.assembly("lens", [ball, ball.translated(1.2, 0, 0).rotated_z(17)])


# name -> (build, resolution); the names of assembly_mass_scenes share its assemblies, lattices and dense fields
OWN = {"spheres": (_spheres, 0.05), "boxes": (_boxes, 0.05), "lens": (_lens, 0.05)}
SHARED = ("gears", "random_1", "random_2", "random_5", "rims", "solids64")
NAMES = tuple(OWN) + SHARED
FORCED = ("spheres", "rims", "random_1")          # the scenes the forced top sides and cell limits run on
FINE_RESOLUTION = (2.0 + 2.0 + SPHERES_GAP) / 4000      # the two balls at 4000 samples along x


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scenario."""
    if name in SHARED:
        return mass_scenes.scene(name)
    build, resolution = OWN[name]
    asm = build()
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims = _instance_cells.checked_lattice(instances, resolution)
    return asm, resolution, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def fields(name):
    if name in SHARED:
        return mass_scenes._fields(name)
    asm, resolution, instances, corner, step, dims = scene(name)
    return mass_scenes.dense_fields(instances, corner, step, dims)


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    """The Dense of a scenario, computed once and shared; nobody changes it."""
    return dense(fields(name))


@functools.lru_cache(maxsize=None)
def traversal_reference(name, side=None, max_top_cells=512):
    asm, resolution, instances, corner, step, dims = scene(name)
    return traverse(field_values(fields(name)), len(instances), dims, step, side, max_top_cells)


@functools.lru_cache(maxsize=None)
def fine_spheres():
    """(assembly, resolution, dims, Traversal) of the two balls on the fine lattice, values from the oracle at points."""
    asm = _spheres()
    instances = _instance_cells.visible(asm, FINE_RESOLUTION)
    corner, step, dims = _instance_cells.checked_lattice(instances, FINE_RESOLUTION)
    return asm, FINE_RESOLUTION, dims, traverse(point_values(instances, corner, step), 2, dims, step)


# ---- the scenarios at the edges of the branch and bound (test_separation_edges_host.py proves each holds its edge) ------

DEEP_SIDES = (1024, 4096, 65536)            # forced on `spheres` and `rims`: 4, 5 and 7 levels, the last all gap_layout() takes
LONG_RESOLUTION = 2.0 ** -6
LONG_RADII = (0.26, 0.25)                   # the larger ball first: the least v lies past the middle, at index 32768
LONG_DISTANCE = 1023.485                    # (0.26 + 1023.485 + 0.25) * 64 = 65535.68: 65536 samples
FAR = (1000, -2000, 500)
ZERO_STEP = 2.0 ** -4
# near_r: the small ball's y; found once by bisection over the binary32 numbers between 0.1 and 0.11 on the child at
# (36, 28, 16) of the level of side 4 (test_separation_edges_host.py measures what they give)
NEAR_R_EQUAL = 0.10416899621486664          # v(q) - U_1 == r: kept, strictly
NEAR_R_DROPPED = 0.10416898876428604        # the binary32 number before it: four ulps above r, dropped
NEAR_R_SIDE = 64


def _long(axis, extra=0.0):
    """Two small balls 1023.485 apart along `axis`: 65536 samples on it, 34 on the other two (`extra` lengthens it)."""
    at = [0.0, 0.0, 0.0]
    at[axis] = LONG_DISTANCE + extra
    return cc.assembly("long", [shapes.sphere(r=LONG_RADII[0]).make_part("big"), shapes.sphere(r=LONG_RADII[1]).make_part("small").translated(*at)])


def _touching():
    """Two boxes with the face x = 0 in common, on a plane of samples (corner x = -1 exactly, step 2^-4).  The right one
    is a plain box where y > 0 and a large box cut off at x = 0 by a difference where y < 0: its w on the plane
    is +0.0 there and -(+0.0) = -0.0 here, the left one's is +0.0."""
    wide = 1 + ZERO_STEP / 2
    left = shapes.box(wide, 1, 1).translated_x(-wide / 2)
    plain = shapes.box(wide, 0.5, 1).translated(wide / 2, 0.25, 0)
    cut = (shapes.box(2 * wide, 0.5, 1).translated(0, -0.25, 0) - shapes.box(2, 2, 2).translated_x(-1))
    return cc.assembly("touching", [left.make_part("left"), shapes.union([plain, cut]).make_part("right")])


def _near_r(t):
    """A ball of radius 1 and one of radius 0.5 beside it, 0.05 apart at t = 0, moved along y by t: inside the large ball's
    extent, so the lattice does not move with it."""
    return cc.assembly("near_r", [shapes.sphere(r=1).make_part("a"), shapes.sphere(r=0.5).make_part("b").translated(1.55, float(t), 0)])


NAN_SCALES = (1e-39, 1e-46)                 # a binary32 denormal; a scale that rounds to 0 in binary32
NAN_SIDE = 64


def _nans():
    """Four parts: a unit ball placed so that the lattice's corner is -0.875 exactly (step 2^-4: index 14 of every axis is
    the coordinate 0.0, and index 14 is the sample q of a child of side 4); a ball scaled by a denormal, whose field is a NaN
    on the three planes through the origin (0 / denormal times infinity) and +inf elsewhere; a ball scaled by what rounds to
    0, whose field is a NaN everywhere; a small ball beside them.  The pairs of `ghost` have no sample with two numbers,
    those of `speck` have numbers (+inf) at some samples only, and (ball, bead) is an ordinary pair."""
    return cc.assembly("nans", [shapes.sphere(r=1).make_part("ball").translated(3 / 32, 3 / 32, 3 / 32),
                                shapes.sphere(r=1).scaled(NAN_SCALES[0]).make_part("speck"),
                                shapes.sphere(r=1).scaled(NAN_SCALES[1]).make_part("ghost"),
                                shapes.sphere(r=0.5).make_part("bead").translated(1.8, 0, 0)])


Edge = collections.namedtuple("Edge", "build resolution side dense", defaults=(None, True))
EDGES = {
    "long_x": Edge(functools.partial(_long, 0), LONG_RESOLUTION, None, False),
    "long_y": Edge(functools.partial(_long, 1), LONG_RESOLUTION, None, False),
    "long_z": Edge(functools.partial(_long, 2), LONG_RESOLUTION, None, False),
    "near_r_equal": Edge(functools.partial(_near_r, NEAR_R_EQUAL), 0.05, NEAR_R_SIDE),
    "near_r_dropped": Edge(functools.partial(_near_r, NEAR_R_DROPPED), 0.05, NEAR_R_SIDE),
    "touching": Edge(_touching, ZERO_STEP),
    "far_boxes": Edge(lambda: _boxes().translated(*FAR), 0.05),
    "far_random_2": Edge(lambda: mass_scenes.scene("random_2")[0].translated(*FAR), None),      # (at random_2's own resolution)
    "nans": Edge(_nans, ZERO_STEP),
    "nans_64": Edge(_nans, ZERO_STEP, NAN_SIDE),            # a second level: NaNs against a bound that is a number
}


@functools.lru_cache(maxsize=None)
def edge_scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of an edge scenario."""
    asm = EDGES[name].build()
    resolution = EDGES[name].resolution if EDGES[name].resolution is not None else mass_scenes.scene("random_2")[1]
    instances = _instance_cells.visible(asm, resolution)
    return (asm, resolution, instances) + tuple(_instance_cells.checked_lattice(instances, resolution))


@functools.lru_cache(maxsize=None)
def edge_fields(name):
    asm, resolution, instances, corner, step, dims = edge_scene(name)
    return mass_scenes.dense_fields(instances, corner, step, dims)


def edge_values(name):
    """The values the reference traversal of an edge scenario reads: its dense fields, or the oracle at the samples where
    the lattice is too long to evaluate densely."""
    asm, resolution, instances, corner, step, dims = edge_scene(name)
    return field_values(edge_fields(name)) if EDGES[name].dense else point_values(instances, corner, step)


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """(Dense or None, Traversal) of an edge scenario, computed once and shared; nobody changes it."""
    asm, resolution, instances, corner, step, dims = edge_scene(name)
    traversal = traverse(edge_values(name), len(instances), dims, step, EDGES[name].side)
    return (dense(edge_fields(name)) if EDGES[name].dense else None), traversal


def report_keys(report):
    """(keys [n, n], {(i, j): witness}) of a SeparationReport, in the reference's terms."""
    n = len(report.instances)
    keys = numpy.full((n, n), NOTHING, dtype=numpy.uint32)
    witness = {}
    for p in report.pairs:
        if p.separation is not None:
            keys[p.i, p.j] = order_keys(numpy.float32(p.separation))
            assert numpy.float32(p.separation).view(numpy.uint32) == key_value(keys[p.i, p.j]).view(numpy.uint32)    # (+0.0, never -0.0)
            witness[(p.i, p.j)] = tuple(int(c) for c in p.witness)
    return keys, witness
