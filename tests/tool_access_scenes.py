"""The scenarios, the raw volumes and the two CPU references of the tool-access tests (test_tool_access_host.py proves on the CPU
that the references agree and that each scenario holds what it is there for; test_gpu_tool_access.py and test_gpu_tool_raw.py
run them on the device).

`reference_tool_access(ids, axis, up, tool, of, n)` (n instances) is REFERENCE 1, written from the definitions in
codecad_amd/tool_access.py alone, with shifted arrays: the tops by a maximum along the axis, the tips and the cut by a loop over
the offsets of D on padded fields, the crowd by the greatest top of the neighbourhood and then the least id among the columns
that attain it (no keys), the holders by a walk of the layers from the spindle side down, the pockets by
assembly_components_scenes.reference_components' flood fill on the rest ids.
`physical_tool_access(ids, axis, up, tool, of)` is REFERENCE 2, independent and physical: it never forms a top.  For every tip
column of the padded domain it lowers the tool from above and keeps the lowest tip height at which the tool's body
{(c + n, h) : h >= z + g(n)} holds no sample of S (by the occupancy of S above a layer); then it marks what the tool sweeps
there, by scattering every tip's underside onto the columns under it; REST is the samples outside S under the lowest swept layer
of their column.

The scenarios are blocks in SAMPLE units at step 1/16, built with assembly_components_scenes._cut and _box, a few tens of
samples a side.  The raw volumes (in the manner of raw_volume_scenes.py) are seeded noise with planted columns; their padding is
poisoned with ids that would raise a top or make rest if a kernel read them as data.
"""
import collections
import functools
import math

import numpy

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_components_scenes as comp
import assembly_voxels_scenes as voxels
import overhangs_scenes as over
import raw_volume_scenes as raw
from assembly_components_scenes import _cut, _box, STEP, SOLID, NONE, EMPTY
from overhangs_scenes import in_set_of, layers, DIRECTIONS

TILE = 32                       # the side of the tile of the morphology kernels (include/hip_util.h HU_TOOL_TILE)

Reference = collections.namedtuple("Reference", "ids in_set tops top_ids tips cut crowd rest_ids undercut tight undercut_counts "
                                                "tight_counts pockets labels")
Case = collections.namedtuple("Case", "name scene axis up tool of")


# ---- the references ---------------------------------------------------------------------------------------------------

def offsets(tool):
    """[(du, dv, g)]: D and the tool's profile over it."""
    K = math.isqrt(tool.radius_sq)
    return [(du, dv, tool.profile[du * du + dv * dv]) for du in range(-K, K + 1) for dv in range(-K, K + 1)
            if du * du + dv * dv <= tool.radius_sq]


def field_of(volume, axis):
    """A [nu, nv] field as it lies beside the volume: broadcast along `axis`."""
    return numpy.expand_dims(volume, axis)


def reference_tool_access(ids, axis, up, tool, of, n, pockets=True):
    s = in_set_of(ids, of)
    shape = ids.shape
    h = layers(shape, axis, up)
    heights = numpy.where(s, h + 1, 0)
    tops = heights.max(axis=axis).astype(numpy.int64)
    highest = numpy.expand_dims(heights.argmax(axis=axis), axis)                    # (unique where the top is not 0)
    top_ids = numpy.where(tops > 0, numpy.take_along_axis(ids, highest, axis).squeeze(axis), EMPTY).astype(numpy.uint8)
    K = math.isqrt(tool.radius_sq)
    D = offsets(tool)
    nu, nv = tops.shape
    pu, pv = nu + 2 * K, nv + 2 * K
    padded = numpy.pad(tops, 2 * K)                                                 # T = 0 outside the lattice
    tips = numpy.full((pu, pv), -1, dtype=numpy.int64)
    for du, dv, g in D:                                                             # the tip column p is the lattice's p - K
        tips = numpy.maximum(tips, padded[K + du:K + du + pu, K + dv:K + dv + pv] - g)
    cut = numpy.full((nu, nv), numpy.iinfo(numpy.int64).max, dtype=numpy.int64)
    for du, dv, g in D:                                                             # c - n is always in the padded domain
        cut = numpy.minimum(cut, tips[K - du:K - du + nu, K - dv:K - dv + nv] + g)
    near_tops, near_ids = numpy.pad(tops, K), numpy.pad(top_ids, K, constant_values=EMPTY)
    greatest = numpy.zeros((nu, nv), dtype=numpy.int64)
    for du, dv, g in D:
        greatest = numpy.maximum(greatest, near_tops[K + du:K + du + nu, K + dv:K + dv + nv])
    crowd = numpy.full((nu, nv), EMPTY, dtype=numpy.uint8)
    for du, dv, g in D:
        attains = (near_tops[K + du:K + du + nu, K + dv:K + dv + nv] == greatest) & (greatest > 0)
        crowd = numpy.where(attains, numpy.minimum(crowd, near_ids[K + du:K + du + nu, K + dv:K + dv + nv]), crowd)
    rest = ~s & (h < field_of(cut, axis))
    undercut = rest & (h < field_of(tops, axis))
    tight = rest & ~undercut
    holders = numpy.full(shape, EMPTY, dtype=numpy.uint8)
    holder = numpy.full((nu, nv), EMPTY, dtype=numpy.uint8)
    for t in range(shape[axis]):                                                    # from the spindle side down
        at = [slice(None)] * 3
        at[axis] = shape[axis] - 1 - t if up else t
        at = tuple(at)
        holder = numpy.where(s[at], ids[at], holder)
        holders[at] = holder
    rest_ids = numpy.where(undercut, holders, numpy.where(tight, field_of(crowd, axis), EMPTY)).astype(numpy.uint8)
    found = comp.reference_components(rest_ids, SOLID) if pockets else None
    for a in (tops, top_ids, tips, cut, crowd, rest_ids):
        a.setflags(write=False)
    return Reference(ids, s, tops, top_ids, tips, cut, crowd, rest_ids, undercut, tight,
                     [int((undercut & (rest_ids == k)).sum()) for k in range(n)], [int((tight & (rest_ids == k)).sum()) for k in range(n)],
                     found.components if pockets else None, found.labels if pockets else None)


def physical_tool_access(ids, axis, up, tool, of):
    """(tips int64[nu + 2K, nv + 2K], rest bool[nx, ny, nz]) by lowering the tool over every tip column and sweeping."""
    s = in_set_of(ids, of)
    occupied = numpy.moveaxis(s if up else numpy.flip(s, axis), axis, 2)             # [nu, nv, layer]
    nu, nv, na = occupied.shape
    K = math.isqrt(tool.radius_sq)
    D = offsets(tool)
    pu, pv = nu + 2 * K, nv + 2 * K
    # above[c, l]: column c holds a sample of S in a layer >= l; False from l = na on, and outside the lattice
    above = numpy.zeros((nu + 4 * K, nv + 4 * K, na + 1), dtype=bool)
    above[2 * K:2 * K + nu, 2 * K:2 * K + nv, :na] = numpy.flip(numpy.maximum.accumulate(numpy.flip(occupied, 2), axis=2), 2)
    tips = numpy.full((pu, pv), -1, dtype=numpy.int64)
    for z in range(na + 1):                                                         # the tip never goes below the table
        free = tips < 0
        for du, dv, g in D:
            free &= ~above[K + du:K + du + pu, K + dv:K + dv + pv, min(z + g, na)]
        tips[free] = z
        if (tips >= 0).all():
            break
    assert (tips >= 0).all()
    lowest = numpy.full((pu + 2 * K, pv + 2 * K), numpy.iinfo(numpy.int64).max, dtype=numpy.int64)   # the lowest swept layer
    for du, dv, g in D:
        under = lowest[K + du:K + du + pu, K + dv:K + dv + pv]
        numpy.minimum(under, tips + g, out=under)
    lowest = lowest[2 * K:2 * K + nu, 2 * K:2 * K + nv]
    rest = ~occupied & (numpy.arange(na)[None, None, :] < lowest[:, :, None])
    rest = numpy.moveaxis(rest, 2, axis)
    return tips, rest if up else numpy.flip(rest, axis)


def canonical(ids, axis, up):
    """The ids with the axis moved to z and flipped to point up: the lateral axes keep their order."""
    moved = numpy.moveaxis(ids, axis, 2)
    return numpy.ascontiguousarray(moved if up else numpy.flip(moved, 2))


def filled(ref, fresh):
    """S' = S with REST added under the id `fresh`: the ids of the idempotence check."""
    return numpy.where(ref.rest_ids != EMPTY, fresh, numpy.where(ref.in_set, ref.ids, EMPTY)).astype(numpy.uint8)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _one(name, shape):
    return cc.assembly(name, [shape.make_part(name)])


POCKET = (20, 18, 12)
POCKET_HOLE = ((5, 4, 4), (15, 14, 12))


def _pocket():
    """A block with a blind square pocket, 10 x 10 samples, 8 deep, open to +z."""
    return _one("pocket", _cut(POCKET, [POCKET_HOLE]))


SLOT = (18, 16, 10)


def _slot():
    """Two parts with a slot 2 samples wide between them, x = 8 and 9, down to the table and open at both ends of y."""
    return cc.assembly("slot", [_box(SLOT, (0, 0, 0), (8, 16, 10)).make_part("left"), _box(SLOT, (10, 0, 0), (18, 16, 10)).make_part("right")])


CORNER = (14, 12, 10)


def _corner():
    """A floor of 2 samples and a wall of 4 x 5 samples up to the top in the lattice's corner x = y = 0."""
    return _one("corner", over._solid(CORNER, [((0, 0, 0), (14, 12, 2)), ((0, 0, 2), (4, 5, 10))]))


TEE = (16, 8, 20)


def _tee():
    """A stem and a bar across it: what lies under the arms is hidden from a spindle along +z."""
    return _one("tee", over._solid(TEE, [((6, 2, 0), (10, 6, 14)), ((0, 0, 14), (16, 8, 20))]))


WALL = (16, 12, 12)
WALL_CUT = [6, 4, 3, 3, 2]      # C at 1..5 columns from the wall under ball_tool(4), by hand (test_tool_access_host.py)


def _wall():
    """A floor of 2 samples and a wall x < 4 across the whole of y up to z = 12."""
    return _one("wall", over._solid(WALL, [((0, 0, 0), (16, 12, 2)), ((0, 0, 2), (4, 12, 12))]))


CUBOID = (12, 10, 9)


def _cuboid():
    return _one("cuboid", _box(CUBOID, (0, 0, 0), CUBOID))


TWO = (14, 12, 16)


def _two():
    """Two parts, no symmetry: part 0 a base with a column and an arm over the base, part 1 a block on the base under the arm's
    end and a post beside it up to the top.  Alone, each part has its own tops."""
    first = over._solid(TWO, [((0, 0, 0), (14, 12, 3)), ((0, 0, 3), (4, 5, 14)), ((0, 0, 10), (11, 5, 13))])
    second = over._solid(TWO, [((7, 1, 3), (11, 4, 7)), ((8, 7, 3), (11, 11, 16))])
    return cc.assembly("two", [first.make_part("frame"), second.make_part("rider")])


SCENES = {"pocket": _pocket, "slot": _slot, "corner": _corner, "tee": _tee, "wall": _wall, "cuboid": _cuboid, "two": _two,
          "shell": comp._shell, "ball": over._ball}


def _tool_name(tool):
    flat = not any(tool.profile)
    ball = math.isqrt(tool.radius_sq) ** 2 == tool.radius_sq and tool == cc.ball_tool(math.isqrt(tool.radius_sq))
    return "flat%d" % tool.radius_sq if flat else "ball%d" % math.isqrt(tool.radius_sq) if ball else "tool%d" % tool.radius_sq


def _case(scene, axis, up, tool, of=SOLID):
    name = "%s_%s%s_%s%s" % (scene, "xyz"[axis], "+" if up else "-", _tool_name(tool), "" if of == SOLID else "_of%d" % of)
    return Case(name, scene, axis, up, tool, of)


FLAT0, FLAT1, FLAT4, FLAT8, BALL3, BALL4 = cc.flat_tool(0), cc.flat_tool(1), cc.flat_tool(4), cc.flat_tool(8), cc.ball_tool(3), cc.ball_tool(4)
CASES = [
    _case("pocket", 2, True, FLAT4), _case("pocket", 2, True, BALL3), _case("pocket", 2, True, FLAT0), _case("pocket", 2, False, FLAT4),
    _case("pocket", 0, True, FLAT1),
    _case("slot", 2, True, FLAT0), _case("slot", 2, True, FLAT1), _case("slot", 2, True, FLAT4), _case("slot", 1, True, FLAT1),
    _case("corner", 2, True, FLAT4), _case("corner", 2, True, BALL3),
    _case("tee", 2, True, FLAT1), _case("tee", 2, False, FLAT1), _case("tee", 0, True, FLAT1), _case("tee", 2, True, FLAT0),
    _case("shell", 2, True, FLAT1), _case("shell", 1, False, cc.ball_tool(2)),
    _case("ball", 2, True, FLAT1), _case("ball", 2, True, FLAT1, 1), _case("ball", 2, True, FLAT1, 0), _case("ball", 2, False, cc.ball_tool(2)),
    _case("wall", 2, True, BALL4), _case("wall", 2, True, FLAT8),
    _case("two", 2, True, FLAT4, 0), _case("two", 2, True, FLAT4, 1), _case("two", 0, False, BALL3, 1),
    _case("cuboid", 2, True, FLAT4), _case("cuboid", 0, False, BALL4), _case("cuboid", 1, True, FLAT0),
]
SIX_CASES = [_case("two", axis, up, FLAT4) for axis, up in DIRECTIONS]
CASES += SIX_CASES
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
assert len(BY_NAME) == len(CASES)


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
    return reference_tool_access(part_ids(c.scene), c.axis, c.up, c.tool, c.of, len(scene(c.scene)[2]))


# ---- seeded random lattices, for the host test ------------------------------------------------------------------------

RANDOM_TOOLS = [cc.flat_tool(r) for r in (0, 1, 2, 5, 9)] + [cc.ball_tool(k) for k in (1, 2, 3, 4)]


def random_lattice(seed):
    """(ids, axis, up, tool, of, n): a lattice of up to 13^3 samples of up to 4 parts at a density of its own."""
    rng = numpy.random.default_rng(7700 + seed)
    shape = tuple(int(v) for v in rng.integers(1, 14, size=3))
    n = int(rng.integers(1, 5))
    ids = rng.integers(0, n, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < rng.choice([0.3, 0.6, 0.9])] = EMPTY
    axis, up = DIRECTIONS[seed % 6]
    of = SOLID if seed % 3 else int(rng.integers(0, n))
    return ids, axis, up, RANDOM_TOOLS[seed % len(RANDOM_TOOLS)], of, n


# ---- the raw volumes --------------------------------------------------------------------------------------------------

RawCase = collections.namedtuple("RawCase", "name ids axis up tool of")
RAW_POISON = raw.alternating(0, 63)         # in the padding: id 0 is in S for SOLID and 0, id 63 for SOLID and 63
RAW_OFS = (SOLID, 0, 63)
PLANTED = {(0, 0): (0, 0), (0, 1): (63, 63), (0, 2): (64, 0), (0, 3): (65, 63), (1, 0): (129, 0)}     # (x, y): (the top's z, its id)


@functools.lru_cache(maxsize=None)
def noise(shape, density, seed=0):
    """Ids 0..63, a fifth of them 63 and a tenth 0, at `density` of solid."""
    rng = numpy.random.default_rng(3100 + sum(shape) + 7 * seed + int(100 * density))
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.2] = 63
    ids[rng.random(shape) < 0.1] = 0
    ids[rng.random(shape) >= density] = EMPTY
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def planted():
    """3x5x130 at 5 %, with columns that end at z = 63, 64 and 65, one whose only sample is z = 0 and one that reaches z = 129."""
    ids = noise((3, 5, 130), 0.05).copy()
    for (x, y), (z, owner) in PLANTED.items():
        ids[x, y, :] = EMPTY
        ids[x, y, z] = owner
    ids[0, 3, 2], ids[0, 2, 30] = 0, 63                                             # something under two of the tops
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def tower():
    """2x2x65536: column (0, 0) solid to the top (T = 65536), (1, 1) a sample at z = 65535 over one at z = 3, the rest empty."""
    ids = numpy.full((2, 2, 65536), EMPTY, dtype=numpy.uint8)
    ids[0, 0, :] = 5
    ids[1, 1, 65535], ids[1, 1, 3] = 7, 0
    ids[0, 1, 40000] = 63
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def random_profile(radius_sq, seed=0):
    rng = numpy.random.default_rng(5200 + radius_sq + seed)
    steps = rng.integers(0, 3, size=radius_sq + 1)
    steps[0] = 0
    return cc.Tool(radius_sq, tuple(int(v) for v in numpy.cumsum(steps)))


STEEP = cc.Tool(1, (0, 65535))              # an entry of 65535: a needle


def _raw_cases():
    cases = []

    def add(name, ids, axis, up, tool, of=SOLID):
        cases.append(RawCase("%s_%s%s_%s%s" % (name, "xyz"[axis], "+" if up else "-", _tool_name(tool), "" if of == SOLID else "_of%d" % of),
                             ids, axis, up, tool, of))

    for shape, density in (((1, 1, 1), 0.7), ((2, 3, 64), 0.3), ((2, 3, 65), 0.3), ((3, 5, 130), 0.3)):
        name = "x".join(str(v) for v in shape)
        for axis, up in DIRECTIONS:
            for of in RAW_OFS:
                add(name, noise(shape, density), axis, up, FLAT1, of)
    for axis, up in DIRECTIONS:
        for of in RAW_OFS:
            add("planted", planted(), axis, up, BALL3, of)
    for density in (0.05, 0.7):
        for axis, up in ((2, True), (0, False), (1, True)):
            add("dense%d" % int(100 * density), noise((9, 7, 70), density), axis, up, cc.flat_tool(5))
    # the columns of a lateral axis: 1, tile - 1, tile, tile + 1 and 2 tile + 1, with K = 0, 1, 5 (radius_sq 25 and 26) and 32
    tools = (FLAT0, FLAT1, cc.flat_tool(25), cc.ball_tool(5), cc.flat_tool(26), cc.ball_tool(32), random_profile(1024))
    for nu, nv in ((1, 2 * TILE + 1), (TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (2 * TILE + 1, 1)):
        for k, tool in enumerate(tools):
            add("tiles%dx%d" % (nu, nv), noise((nu, nv, 5), 0.3), 2, bool(k % 2), tool)
    add("tiles33x65", noise((3, TILE + 1, 2 * TILE + 1), 0.3), 0, True, cc.ball_tool(5))        # (u, v) = (y, z)
    add("tiles33x65", noise((3, TILE + 1, 2 * TILE + 1), 0.3), 0, False, cc.flat_tool(1024))
    add("tiles65x31", noise((2 * TILE + 1, 2, TILE - 1), 0.3), 1, True, random_profile(1024))   # (u, v) = (x, z)
    add("tiles32x64", noise((TILE, 2, 2 * TILE), 0.3), 1, False, cc.flat_tool(26))
    for tool in (cc.flat_tool(1024), random_profile(1024, 1)):                      # K greater than the whole lattice
        add("small3x3", noise((3, 3, 4), 0.3, 1), 2, True, tool)
        add("small3x3", noise((3, 3, 4), 0.3, 1), 1, False, tool)
    for up in (True, False):                                                        # heights past 16 bits
        add("tower", tower(), 2, up, STEEP)
        add("tower", tower(), 2, up, BALL3)
    add("tower", tower(), 0, True, FLAT1)
    add("steep", noise((6, 5, 70), 0.3), 2, True, STEEP)
    add("steep", noise((6, 5, 70), 0.3), 0, False, cc.Tool(2, (0, 7, 65535)))
    return cases


RAW_CASES = _raw_cases()
RAW_BY_NAME = {c.name: c for c in RAW_CASES}
RAW_NAMES = [c.name for c in RAW_CASES]
assert len(RAW_BY_NAME) == len(RAW_CASES), [n for n in RAW_NAMES if RAW_NAMES.count(n) > 1]


@functools.lru_cache(maxsize=None)
def raw_reference(name):
    """The Reference of a raw case, without pockets (the raw tests call the four entry points alone)."""
    c = RAW_BY_NAME[name]
    return reference_tool_access(c.ids, c.axis, c.up, c.tool, c.of, 64, pockets=False)
