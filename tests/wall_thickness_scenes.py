"""The scenarios and the CPU references of the wall-thickness tests (test_wall_thickness_host.py proves on the CPU that the two
references agree and that each scenario holds what it is there for; test_gpu_wall_thickness.py runs the scenarios through
wall_thickness() on the device, test_gpu_thickness_local.py the raw cases through hu_thickness_local alone).

`raw_local(field, in_set, r2)` is the rule of hu_thickness_local written from its statement, offset by offset with shifted
arrays: in = field on S and 0 elsewhere (outside the lattice too); a sample with in > 0 takes the greatest in(p + o) over the
offsets o with |o|^2 < in(p + o).  Only offsets with |o|^2 <= r2 and |o_i| < dims_i can qualify (values are at most r2 + 1, and
a tap outside the lattice reads 0), so only those are walked.
`reference_thickness(ids, of, r2, n)` is REFERENCE 1 of wall_thickness(): depth_sq offset by offset as thin_walls_scenes does
it, raw_local on it, and the per-part fields restated.
`opening_thickness(ids, of, r2, n)` is REFERENCE 2: 1 + the greatest v in 0..r2 whose opening (the `cover` of
thin_walls_scenes.reference_thin with both radii v) keeps the sample.

The scenarios are blocks in SAMPLE units at step 1/16, those of thin_walls_scenes and a few of their kind."""
import collections
import functools
import itertools

import numpy

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_voxels_scenes as voxels
import raw_volume_scenes as raw
import thin_walls_scenes as thin
from thin_walls_scenes import STEP, SOLID, EMPTY, in_set_of, isqrt

Reference = collections.namedtuple("Reference", "ids in_set depth_sq thickness_sq counts core_counts capped_counts min_sq thinnest")
Case = collections.namedtuple("Case", "name scene of r2")
RawCase = collections.namedtuple("RawCase", "name ids field of r2")
TILE = (8, 8, 16)               # include/hip_util.h HU_COMPONENTS_TILE_*
MAX_RADIUS_SQ = 1024
NO_KEY = 0xffffffffffffffff


# ---- the references ---------------------------------------------------------------------------------------------------

def offsets(limit_sq, dims):
    """int64[m, 3]: every offset with |o|^2 <= limit_sq and |o_i| < dims_i, the nearest first, and their |o|^2."""
    k = isqrt(limit_sq)
    axes = [numpy.arange(-min(k, int(d) - 1), min(k, int(d) - 1) + 1, dtype=numpy.int64) for d in dims]
    o = numpy.stack(numpy.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    sq = (o * o).sum(axis=1)
    keep = numpy.argsort(sq, kind="stable")
    keep = keep[sq[keep] <= limit_sq]
    return o[keep], sq[keep]


def raw_local(field, in_set, r2):
    """int64 like `field`: the rule of hu_thickness_local (the module's docstring)."""
    shape = field.shape
    counted = numpy.where(in_set, field.astype(numpy.int64), 0)
    pad = [min(isqrt(r2), d - 1) for d in shape]
    padded = numpy.pad(counted, [(p, p) for p in pad])
    out = numpy.zeros(shape, dtype=numpy.int64)
    for o, sq in zip(*offsets(r2, shape)):
        there = thin._shifted(padded, pad, o, shape)
        out = numpy.where(there > sq, numpy.maximum(out, there), out)
    return numpy.where(counted > 0, out, 0)


def depth_of(in_set, r2):
    """int64: min(D1, r2 + 1) on S, 0 elsewhere, D1 the squared distance to the nearest point not in S (outside the lattice is
    none of S), offset by offset."""
    shape = in_set.shape
    pad = [min(isqrt(r2) + 1, d) for d in shape]
    padded = numpy.pad(in_set, [(p, p) for p in pad])
    depth = numpy.full(shape, r2 + 1, dtype=numpy.int64)
    for o, sq in zip(*thin.offsets(r2, shape)):
        depth = numpy.where(thin._shifted(padded, pad, o, shape), depth, numpy.minimum(depth, sq))
    return numpy.where(in_set, depth, 0)


def per_part(ids, values, n):
    """(min_sq, thinnest) of `values` > 0 per id 0..n-1: the least value and the lexicographically first sample that has it."""
    least, where = [], []
    for k in range(n):
        own = (ids == k) & (values > 0)
        if not own.any():
            least.append(None), where.append(None)
            continue
        v = int(values[own].min())
        least.append(v)
        where.append(tuple(int(c) for c in numpy.argwhere(own & (values == v))[0]))        # (argwhere: in C order, x slowest)
    return least, where


def reference_thickness(ids, of, r2, n):
    s = in_set_of(ids, of)
    depth = depth_of(s, r2)
    thickness = raw_local(depth, s, r2)
    least, where = per_part(ids, thickness, n)
    for a in (depth, thickness):
        a.setflags(write=False)
    return Reference(ids, s, depth.astype(numpy.uint16), thickness.astype(numpy.uint16), [int((ids == k).sum()) for k in range(n)],
                     [int(((depth == r2 + 1) & (ids == k)).sum()) for k in range(n)],
                     [int(((thickness == r2 + 1) & (ids == k)).sum()) for k in range(n)], least, where)


def uncapped_thickness(in_set):
    """int64: the thickness with no cap at all.  No sample is deeper than half the lattice's shortest side, rounded up: a cap
    above that square is never met, by the depth or by a ball."""
    far = ((min(in_set.shape) + 1) // 2) ** 2
    depth = depth_of(in_set, far)
    assert depth.max() <= far
    return raw_local(depth, in_set, far)


def opening_thickness(ids, of, r2, n):
    """int64: on S, 1 + the greatest v in 0..r2 for which the opening by the digital ball of squared radius v keeps the sample.
    The CORES {D1 > v} are nested though the openings are not: once a core is empty, and its opening with it, every greater v
    has an empty core and keeps nothing, and the walk over v ends there."""
    s = in_set_of(ids, of)
    out = numpy.zeros(ids.shape, dtype=numpy.int64)
    for v in range(r2 + 1):
        opened = thin.reference_thin(ids, of, v, v, n)
        if not opened.core.any():
            assert not opened.cover.any()
            break
        out = numpy.where(opened.cover, v + 1, out)
    assert (out[s] >= 1).all() and (out[~s] == 0).all()                                      # v = 0 keeps all of S
    return out


def keys_of(ids, out):
    """uint64[64]: what hu_thickness_local leaves in keys_dev over all ones."""
    keys = numpy.full(64, NO_KEY, dtype=numpy.uint64)
    least, where = per_part(ids, out, 64)
    for p in range(64):
        if least[p] is not None:
            x, y, z = where[p]
            keys[p] = least[p] << 48 | x << 32 | y << 16 | z
    return keys


# ---- the scenarios of wall_thickness() --------------------------------------------------------------------------------

PLATE = thin.PLATE
SLAB_R2 = 9                     # K = 3: slabs of 1..6 samples read ceil(w / 2)^2 <= 9, the slab of 7 reads the cap
SLAB_WIDTHS = tuple(range(1, 8))
BALL_RADIUS = 10                # samples


def _ball():
    return cc.assembly("ball", [shapes.sphere(r=BALL_RADIUS * STEP).make_part("ball")])


SCENES = dict(thin.SCENES)
SCENES["ball"] = _ball
for _axis, _w in itertools.product(range(3), SLAB_WIDTHS):
    SCENES["slab_%s_%d" % ("xyz"[_axis], _w)] = functools.partial(thin._slab, _axis, _w)

CASES = [Case("slab_%s_w%d" % ("xyz"[_axis], _w), "slab_%s_%d" % ("xyz"[_axis], _w), SOLID, SLAB_R2)
         for _axis, _w in itertools.product(range(3), SLAB_WIDTHS)]
CASES += [
    Case("cuboid_5", "cuboid_5", SOLID, 4),                 # every side 2 K + 1: one core sample, every sample within its ball but the corners
    Case("cuboid_5_r0", "cuboid_5", SOLID, 0),              # R2 = 0: L = 1 on S
    Case("rib", "rib", SOLID, 4),                           # the body reads the cap, the rib and the floor their width
    Case("rib_r25", "rib", SOLID, 25),                      # K = 5: the second LDS kernel
    Case("wedge", "wedge", SOLID, 9),                       # steps of 2, 4, 6 and 8 samples: 1, 4, 9 and the cap
    Case("ball_r16", "ball", SOLID, 16),
    Case("ball_r81", "ball", SOLID, 81),                    # K = 9, the second LDS kernel: the ball's middle, 86 deep, reads the cap
    Case("ball_r144", "ball", SOLID, 144),                  # K = 12, the third: nothing reaches the cap
    Case("glued_solid", "plate_on_block", SOLID, 4),
    Case("glued_plate", "plate_on_block", 0, 4),            # as its own part the plate is thin, in the solid it is backed
    Case("glued_block", "plate_on_block", 1, 4),
    Case("pressed_pin", "pin_in_block", 0, 4),
    Case("pressed_block", "pin_in_block", 1, 4),            # the block with the pin's hole through it
    Case("ragged", "ragged", SOLID, 2),                     # nz = 11, pz = 16: a ragged lattice
    Case("ragged_r400", "ragged", SOLID, 400),              # K = 20 > 16 on a lattice narrower than K: the halo is chosen after the scan
    Case("ragged_r1024", "ragged", SOLID, MAX_RADIUS_SQ),
    Case("tower", "tower", SOLID, 9),                       # nz = 70: five tiles along z
    Case("shell", "shell", SOLID, 16),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scene."""
    asm = SCENES[name]()
    instances = _instance_cells.visible(asm, STEP)
    corner, step, dims = _instance_cells.checked_lattice(instances, STEP)
    return asm, STEP, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def part_ids(name):
    """The dense part ids of a scene: assembly_voxels_scenes.reference_voxels', computed once."""
    asm, resolution, instances, corner, step, dims = scene(name)
    ids = voxels.reference_voxels(instances, corner, step, dims, True).ids
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def reference(case):
    """The Reference of a case (by name), computed once and shared; nobody changes it."""
    c = BY_NAME[case]
    return reference_thickness(part_ids(c.scene), c.of, c.r2, len(scene(c.scene)[2]))


def random_volume(seed):
    """(ids, of, r2, n): a small seeded volume of blobs of up to three parts."""
    rng = numpy.random.default_rng(9100 + seed)
    shape = tuple(int(v) for v in rng.integers(3, 11, size=3))
    n = int(rng.integers(1, 4))
    ids = rng.integers(0, n, size=shape).astype(numpy.uint8)
    noise = rng.random(shape)
    for axis in range(3):                                                                    # smooth the holes into blobs
        noise = (noise + numpy.roll(noise, 1, axis) + numpy.roll(noise, -1, axis)) / 3
    ids[noise < numpy.quantile(noise, float(rng.uniform(0.1, 0.5)))] = EMPTY
    of = SOLID if seed % 3 else int(rng.integers(0, n))
    return ids, of, int(rng.choice([0, 1, 2, 3, 4, 5, 8, 9, 12])), n


# ---- the raw cases of hu_thickness_local ------------------------------------------------------------------------------

def sparse_field(rng, shape, cap, density=0.3):
    """Values 1..cap on about `density` of the samples, 0 on the rest: no distance transform."""
    field = rng.integers(1, cap + 1, size=shape)
    field[rng.random(shape) >= density] = 0
    return field.astype(numpy.uint16)


def some_ids(rng, shape, empty=0.15):
    """Ids from 0..63 (a fifth of them 3, so that of = 3 has samples) with some empty samples."""
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.2] = 3
    ids[rng.random(shape) < empty] = EMPTY
    return ids


def _raw_cases():
    cases = []

    def add(name, ids, field, of, r2):
        ids, field = numpy.ascontiguousarray(ids, numpy.uint8), numpy.ascontiguousarray(field, numpy.uint16)
        assert ids.shape == field.shape and int(field.max()) <= r2 + 1 and 0 <= r2 <= MAX_RADIUS_SQ
        ids.setflags(write=False), field.setflags(write=False)
        cases.append(RawCase(name, ids, field, of, r2))

    rng = numpy.random.default_rng(77001)
    # random fields that are no distance transforms, on three tiles a side and a ragged end; every kernel of the entry point
    for r2, of in ((0, SOLID), (1, 3), (5, SOLID), (16, 3), (17, SOLID), (81, SOLID), (100, 3), (144, SOLID)):
        shape = (19, 18, 37)
        add("random_r%d_of%s" % (r2, of), some_ids(rng, shape), sparse_field(rng, shape, r2 + 1, 0.02 if r2 > 20 else 0.3), of, r2)
    # single lines along each axis and single samples
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = 40
        add("line_%s" % "xyz"[axis], some_ids(rng, shape, 0.1), sparse_field(rng, shape, 10, 0.4), SOLID, 9)
    add("one_sample_cap", numpy.zeros((1, 1, 1)), numpy.full((1, 1, 1), 5), SOLID, 4)
    add("one_sample_low", numpy.zeros((1, 1, 1)), numpy.full((1, 1, 1), 1), 0, 4)
    add("one_sample_empty", numpy.full((1, 1, 1), EMPTY), numpy.full((1, 1, 1), 5), SOLID, 4)
    # dims around the tile's edges, and around 64
    for axis, sides in ((0, (7, 8, 9)), (1, (7, 8, 9)), (2, (15, 16, 17))):
        for side in sides:
            shape = [9, 9, 17]
            shape[axis] = side
            add("edge_%s%d" % ("xyz"[axis], side), some_ids(rng, shape), sparse_field(rng, shape, 6), SOLID, 5)
    for axis, side in itertools.product(range(3), (63, 64, 65)):
        shape = [2, 3, 5]
        shape[axis] = side
        add("long_%s%d" % ("xyz"[axis], side), some_ids(rng, shape), sparse_field(rng, shape, 10), SOLID, 9)
    # one ball whose centre sits on a tile corner: its reach crosses three faces, into eight tiles
    shape = (16, 16, 32)
    field = numpy.ones(shape, numpy.uint16)
    field[8, 8, 16] = 50
    add("ball_on_a_corner", numpy.zeros(shape), field, SOLID, 64)
    # K = 0, 1, 9 (a halo wider than a tile side) and 32, on a lattice narrower than K
    shape = (5, 20, 7)
    for r2 in (0, 1, 81, MAX_RADIUS_SQ):
        add("narrow_r%d" % r2, some_ids(rng, shape), sparse_field(rng, shape, r2 + 1, 0.1), SOLID, r2)
    # a greatest value that is small under a large R2: the shrunken radius; the same bytes as with R2 = that value - 1
    shape = (12, 11, 21)
    low_ids, low = some_ids(rng, shape), sparse_field(rng, shape, 10)
    for r2 in (9, 100, 256, MAX_RADIUS_SQ):
        add("low_r%d" % r2, low_ids, low, SOLID, r2)
    # all cap: every wavefront leaves at once
    shape = (9, 10, 33)
    for r2 in (16, 400):
        add("all_cap_r%d" % r2, rng.integers(0, 64, size=shape), numpy.full(shape, r2 + 1), SOLID, r2)
    # the keys' tie rule: every sample reads 1, so every part's key is its lexicographically first sample
    shape = (10, 9, 20)
    add("ties", rng.integers(0, 3, size=shape), numpy.ones(shape), SOLID, 4)
    return cases


RAW_CASES = _raw_cases()
RAW_BY_NAME = {c.name: c for c in RAW_CASES}
RAW_NAMES = [c.name for c in RAW_CASES]
LOW_NAMES = [n for n in RAW_NAMES if n.startswith("low_")]


def raw_buffers(case, pitch=None):
    """(ids uint8[nx][ny][pz], field uint16[nx][ny][pz], pz) as the device takes them, POISONED: the padding of the ids lies in
    S, the padding of the field and its entries outside S hold the cap -- read as data, each would raise a neighbour's answer.
    pz is `pitch`, or ceil16(nz) without one."""
    cap = case.r2 + 1
    s = in_set_of(case.ids, case.of)
    ids, pz = raw.padded(case.ids, raw.constant(0 if case.of == SOLID else case.of), pitch)
    field, _ = raw.padded16(numpy.where(s, case.field, cap), raw.constant(cap), pitch)
    return ids, field, pz


@functools.lru_cache(maxsize=None)
def raw_reference(name):
    """(out int64, keys uint64[64], counts per id 0..63) of a raw case."""
    c = RAW_BY_NAME[name]
    s = in_set_of(c.ids, c.of)
    out = raw_local(c.field, s, c.r2)
    out.setflags(write=False)
    capped = (out == c.r2 + 1) & s
    return out, keys_of(numpy.where(s, c.ids, EMPTY), out), [int((capped & (c.ids == p)).sum()) for p in range(64)]
