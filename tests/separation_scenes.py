"""The scenarios of the separation tests (test_separation_host.py holds the traversal to the dense definition on the CPU;
test_gpu_separation.py holds the device to both) and their CPU reference, written from codecad_amd/separation.py's
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


def traverse(values, n, dims, step, side=None, max_top_cells=512):
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
                kept = at & ~(difference > r)                                 # (a NaN keeps the pair)
                keep[kept] |= (one << numpy.uint64(i)) | (one << numpy.uint64(j))
                lowered[i, j] = min(lowered[i, j], order_keys(v[at]).min())
            going = keep != 0
            origin, mask, keys = first[going], keep[going], lowered
            level_rows.append(len(origin))
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
