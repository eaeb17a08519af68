"""The scenarios and the CPU references of the drainage tests (test_drainage_host.py proves on the CPU that each scenario holds
what it is there for; test_gpu_drainage.py runs them on the device).

`escape_set(empty, axis, up)` is written from the definition in codecad_amd/drainage.py alone: the seeds -- E in layer 0 or at
a lateral border -- and then X grown by shifted arrays, "the sample below or a lateral neighbour is in X", to its fixed point.
`layered_escape` is the second way: every layer's 4-connected components by flood fill (`layer_labels`), and escape handed
upwards layer by layer, one sweep.  `synchronous(empty, axis, up, k)` is what k synchronous steps over all (sample, below) pairs
leave flagged when whole layer components carry the flags, as on the device.  The floors come from a walk up every line with a
running last solid id, the pools from assembly_components_scenes.reference_components' flood fill on the trapped ids.

The scenes of this module are boxes on the lattice in SAMPLE units at step 1/16, built with disassembly_scenes' helpers; the
hollow ball, the serpentine and the ball over a slab are their modules' own.  RAW volumes are id arrays that no assembly gives,
for the entry points alone.
"""
import collections
import functools

import numpy

import assembly_components_scenes as comp
import disassembly_scenes as dis_scenes
from disassembly_scenes import _scene, DIRECTIONS
from assembly_components_scenes import SOLID, NONE, EMPTY

Reference = collections.namedtuple("Reference", "ids counts escapes trapped trapped_ids trapped_counts pools labels")
# `frame`: the lattice the parts span, or None for a scene of another module; `trapped`: {(axis, up): the trapped samples} by
# hand for the directions named, every other direction of a scene of this module holds NOTHING unless `others` says "any"
Scene = collections.namedtuple("Scene", "build frame trapped others")
NZ = 138                                                                            # three words and a ragged tail under pz = 144


# ---- the references ---------------------------------------------------------------------------------------------------

def shifted(a, axis, d):
    """out[p] = a[p - d e_axis], False where p - d e_axis lies outside."""
    out = numpy.zeros_like(a)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    dst[axis], src[axis] = (slice(d, None), slice(None, -d)) if d > 0 else (slice(None, d), slice(-d, None))
    out[tuple(dst)] = a[tuple(src)]
    return out


def layers(shape, axis, up):
    """int64[nx, ny, nz]: h(p)."""
    along = numpy.indices(shape)[axis]
    return along if up else shape[axis] - 1 - along


def seeds(empty, axis, up):
    """E in layer 0 or with a lateral index of 0 or n - 1."""
    at = numpy.indices(empty.shape)
    out = layers(empty.shape, axis, up) == 0
    for a in range(3):
        if a != axis:
            out = out | (at[a] == 0) | (at[a] == empty.shape[a] - 1)
    return empty & out


def escape_set(empty, axis, up):
    """X from the definition: grown by shifted arrays to the fixed point."""
    sign = 1 if up else -1
    x = seeds(empty, axis, up)
    while True:
        grown = shifted(x, axis, sign)                                              # the sample below is in X
        for a in range(3):
            if a != axis:
                grown = grown | shifted(x, a, 1) | shifted(x, a, -1)
        grown = x | (empty & grown)
        if numpy.array_equal(grown, x):
            return x
        x = grown


def layer_labels(empty, axis):
    """uint32[nx, ny, nz]: the least linear index of the 4-connected component of E a sample lies in WITHIN ITS LAYER of `axis`,
    NONE outside E -- the flood fill of assembly_components_scenes over the volume with a wall between every two layers."""
    shape = empty.shape
    wide = list(shape)
    wide[axis] = 2 * shape[axis]
    apart = numpy.zeros(wide, dtype=bool)
    even = [slice(None)] * 3
    even[axis] = slice(0, None, 2)
    apart[tuple(even)] = empty
    found = comp.flood_labels(apart)[tuple(even)]
    at = list(numpy.unravel_index(numpy.where(found == NONE, 0, found).astype(numpy.int64), wide))
    at[axis] = at[axis] // 2                                                        # (the order of the indices is kept: the least stays the least)
    return numpy.where(found == NONE, NONE, numpy.ravel_multi_index(tuple(at), shape)).astype(numpy.uint32)


def layered_escape(empty, axis, up, labels=None):
    """X the second way: the layers from 0 up, in each the components that hold a seed or a sample over an escaping one."""
    labels = layer_labels(empty, axis) if labels is None else labels
    first = seeds(empty, axis, up)
    x = numpy.zeros(empty.shape, dtype=bool)
    na = empty.shape[axis]
    for h in range(na):
        here = [slice(None)] * 3
        here[axis] = h if up else na - 1 - h
        here = tuple(here)
        start = first[here].copy()
        if h > 0:
            under = [slice(None)] * 3
            under[axis] = h - 1 if up else na - h
            start |= empty[here] & x[tuple(under)]
        x[here] = empty[here] & numpy.isin(labels[here], numpy.unique(labels[here][start]))
    return x


def synchronous(empty, axis, up, k, labels=None):
    """The samples under a flagged component after the seeds and k synchronous steps: a step flags the component of every p of E
    whose sample below lay under a flagged component before the step."""
    labels = layer_labels(empty, axis) if labels is None else labels
    sign = 1 if up else -1
    first = seeds(empty, axis, up)
    x = empty & numpy.isin(labels, numpy.unique(labels[first]))
    for _ in range(k):
        over = empty & shifted(x, axis, sign) & ~x
        if not over.any():
            break
        x = x | (empty & numpy.isin(labels, numpy.unique(labels[over])))
    return x


def floors(ids, axis, up):
    """uint8[nx, ny, nz]: the id of the nearest solid sample below on the line, 255 with none: a walk from layer 0 up."""
    out = numpy.full(ids.shape, EMPTY, dtype=numpy.uint8)
    na = ids.shape[axis]
    last = None
    for h in range(na):
        here = [slice(None)] * 3
        here[axis] = h if up else na - 1 - h
        here = tuple(here)
        if last is None:
            last = numpy.full(ids[here].shape, EMPTY, dtype=numpy.uint8)
        out[here] = last
        last = numpy.where(ids[here] != EMPTY, ids[here], last)
    return out


def reference_of(ids, n, axis, up):
    empty = ids == EMPTY
    x = escape_set(empty, axis, up)
    trapped = empty & ~x
    trapped_ids = numpy.where(trapped, floors(ids, axis, up), EMPTY).astype(numpy.uint8)
    found = comp.reference_components(trapped_ids, SOLID)
    for a in (x, trapped, trapped_ids):
        a.setflags(write=False)
    return Reference(ids, [int((ids == k).sum()) for k in range(n)], x, trapped, trapped_ids,
                     [int((trapped_ids == k).sum()) for k in range(n)], found.components, found.labels)


def level_of(pool, shape, axis, up):
    """The highest layer of a pool's box."""
    return pool.box[1][axis] if up else shape[axis] - 1 - pool.box[0][axis]


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _box(lo, hi):
    return {(x, y, z) for x in range(lo[0], hi[0]) for y in range(lo[1], hi[1]) for z in range(lo[2], hi[2])}


def _mine(name, frame, solids, trapped, others="nothing"):
    return Scene(_scene(name, frame, solids, {}).build, frame, trapped, others)


def _cup_boxes(frame, floor):
    """A floor of `floor` samples and walls two samples thick up to the top layer: the rim is the lattice's top."""
    nx, ny, nz = frame
    base = [((0, 0, 0), (nx, ny, floor))]
    walls = [((0, 0, floor), (2, ny, nz)), ((nx - 2, 0, floor), (nx, ny, nz)), ((2, 0, floor), (nx - 2, 2, nz)),
             ((2, ny - 2, floor), (nx - 2, ny, nz))]
    return base, walls


CUP = (10, 9, 12)
BELL = (10, 9, 14)
UBEND = (14, 5, 12)
STEPPED = (12, 6, 10)
LEVELS = (15, 5, 70)
LEVEL_RIMS = (63, 64, 65)
SHAFT = (5, 5, NZ)
CORRIDOR = (18, 10, 70)


def _bell(gap):
    """Part 0 a slab, part 1 a bell over it: a roof and walls that stand on the slab, or end one layer above it."""
    nx, ny, nz = BELL
    low = 3 if gap else 2
    walls = [((0, 0, low), (1, ny, 11)), ((nx - 1, 0, low), (nx, ny, 11)), ((1, 0, low), (nx - 1, 1, 11)), ((1, ny - 1, low), (nx - 1, ny, 11))]
    return [[((0, 0, 0), (nx, ny, 2))], [((0, 0, 11), (nx, ny, nz))] + walls]


def _block_but(frame, holes):
    """One part: a block of `frame` samples with the boxes `holes` [lo, hi) cut out (assembly_components_scenes._cut)."""
    return comp.cc.assembly("block", [comp._cut(frame, holes).make_part("block")])


def _scenes():
    out = {}
    # a cup: it holds its inside with `up` along its opening, and nothing in the other five directions
    base, walls = _cup_boxes(CUP, 3)
    inside = _box((2, 2, 3), (8, 7, 12))
    out["cup"] = _mine("cup", CUP, [base + walls], {(2, True): inside})
    # the same cup of two parts: the floor is part 0, the walls are part 1; the pool stands on 0 alone
    out["cup_two_parts"] = _mine("cup2", CUP, [base, walls], {(2, True): inside})
    # a bell over a slab with a gap of one layer: nothing is trapped (upside down it is a cup, filled up to the gap); standing on
    # the slab: sealed, trapped every way up
    room = _box((1, 1, 2), (9, 8, 11))
    out["bell_gap"] = _mine("bellgap", BELL, _bell(True), {(2, False): _box((1, 1, 3), (9, 8, 11))})
    out["bell_sealed"] = _mine("bellsealed", BELL, _bell(False), {d: room for d in DIRECTIONS})
    # a U-bend: a channel one sample wide, a leg up to the top face (no exit), a run along x and a leg that leaves sideways at
    # z = 6.  Upwards the whole closed leg, the run and the other leg below the exit are trapped; downwards everything runs out
    # of the leg that reaches the top face, now layer 0
    bend = [((2, 2, 2), (3, 3, 12)), ((2, 2, 2), (12, 3, 3)), ((11, 2, 2), (12, 3, 7)), ((11, 2, 6), (14, 3, 7))]
    held = _box((2, 2, 2), (3, 3, 12)) | _box((2, 2, 2), (12, 3, 3)) | _box((11, 2, 2), (12, 3, 6))
    out["u_bend"] = Scene(functools.partial(_block_but, UBEND, bend), UBEND, {(2, True): held, (2, False): set()}, "any")
    # a stepped pocket: the deep half stands on part 0, the step is part 1's
    ring = [((0, 0, 3), (1, 6, 10)), ((11, 0, 3), (12, 6, 10)), ((1, 0, 3), (11, 1, 10)), ((1, 5, 3), (11, 6, 10))]
    out["stepped"] = _mine("stepped", STEPPED, [[((0, 0, 0), (12, 6, 3))], ring + [((6, 1, 3), (11, 5, 6))]],
                           {(2, True): _box((1, 1, 3), (6, 5, 10)) | _box((6, 1, 6), (11, 5, 10))})
    # three cups along x whose walls end at z = 63, 64 and 65: the surfaces lie in the last layer of word 0 and the first two of word 1
    cups, pools = [((0, 0, 0), (15, 5, 2)), ((0, 0, 0), (1, 1, 70))], set()
    for k, rim in enumerate(LEVEL_RIMS):
        x0 = 5 * k
        cups += [((x0, 0, 2), (x0 + 1, 5, rim + 1)), ((x0 + 4, 0, 2), (x0 + 5, 5, rim + 1)), ((x0 + 1, 0, 2), (x0 + 4, 1, rim + 1)),
                 ((x0 + 1, 4, 2), (x0 + 4, 5, rim + 1))]
        pools |= _box((x0 + 1, 1, 2), (x0 + 4, 4, rim + 1))
    out["levels"] = _mine("levels", LEVELS, [cups], {(2, True): pools, (2, False): set()}, "any")
    # a blind shaft of 135 samples along z: the line (2, 2) holds no solid in words 1 and 2
    shaft = [((2, 2, 3), (3, 3, NZ))]
    out["shaft"] = Scene(functools.partial(_block_but, SHAFT, shaft), SHAFT, {(2, True): _box(*shaft[0]), (2, False): set()}, "any")
    # a chamber x 2..6, y 2..7, z 60..66 and a corridor of one sample at z = 64, the first layer of word 1, from x = 7 across the tile
    # faces 7 | 8 and 15 | 16 to the border x = 17: upwards the layers under the corridor are trapped, downwards those over it,
    # along +x the corridor is a dead end under the top face and everything is trapped, along -x nothing
    chamber, way = ((2, 2, 60), (7, 8, 67)), ((7, 4, 64), (18, 5, 65))
    out["corridor"] = Scene(functools.partial(_block_but, CORRIDOR, [chamber, way]), CORRIDOR,
                            {(2, True): _box((2, 2, 60), (7, 8, 64)), (2, False): _box((2, 2, 65), (7, 8, 67)),
                             (0, True): _box(*chamber) | _box(*way), (0, False): set()}, "any")
    return out


MINE = _scenes()
SCENES = dict(MINE)
SCENES["hollow_ball"] = Scene(comp.SCENES["shell"].build, None, {}, "any")           # its cavity is trapped every way up
SCENES["serpentine"] = Scene(comp.SCENES["serpentine_open"].build, None, {}, "any")   # escape needs several handovers
SCENES["ball_over_slab"] = Scene(dis_scenes.SCENES["ownership"].build, None, {}, "any")     # three owners
SCENES["nothing"] = Scene(dis_scenes.SCENES["single"].build, None, {d: set() for d in DIRECTIONS}, "nothing")
NAMES = list(SCENES)
CASES = [(name, axis, up) for name in NAMES for axis, up in DIRECTIONS]
_OTHER = {"hollow_ball": (comp, "shell"), "serpentine": (comp, "serpentine_open"), "ball_over_slab": (dis_scenes, "ownership"),
          "nothing": (dis_scenes, "single")}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scene."""
    if name in _OTHER:
        module, theirs = _OTHER[name]
        return module.scene(theirs)
    asm = SCENES[name].build()
    instances = dis_scenes._instance_cells.visible(asm, dis_scenes.STEP)
    corner, step, dims = dis_scenes._instance_cells.checked_lattice(instances, dis_scenes.STEP)
    return asm, dis_scenes.STEP, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def part_ids(name):
    """The dense part ids of a scene, every instance evaluated at every sample, once."""
    if name in _OTHER:
        module, theirs = _OTHER[name]
        return module.part_ids(theirs)
    asm, resolution, instances, corner, step, dims = scene(name)
    ids, counts = dis_scenes.voxels.dense_ids([w < 0 for w in dis_scenes.mass.dense_fields(instances, corner, step, dims)])
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def labels_of(name, axis):
    """The layer labels of a scene along an axis, computed once."""
    out = layer_labels(part_ids(name) == EMPTY, axis)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, axis, up):
    """The Reference of a case, computed once and shared; nobody changes it."""
    return reference_of(part_ids(name), len(scene(name)[2]), axis, up)


# ---- raw id volumes, for the entry points alone -----------------------------------------------------------------------

RAW_PARTS = 64


def _random(shape, seed, solid=0.55):
    rng = numpy.random.default_rng(seed)
    ids = rng.integers(0, RAW_PARTS, size=shape).astype(numpy.uint8)
    return numpy.where(rng.random(shape) < solid, ids, EMPTY).astype(numpy.uint8)


RAW = {
    "19x21x70": lambda: _random((19, 21, 70), 31),             # three tiles a lateral axis, ragged on all; a word and six samples
    "9x8x130": lambda: _random((9, 8, 130), 32),               # two words and two samples; one tile and one sample along x
    "line_z": lambda: _random((1, 1, 130), 33),
    "line_y": lambda: _random((1, 21, 1), 34),
    "line_x": lambda: _random((19, 1, 1), 35),
    "sample_empty": lambda: numpy.full((1, 1, 1), EMPTY, dtype=numpy.uint8),
    "sample_solid": lambda: numpy.zeros((1, 1, 1), dtype=numpy.uint8),
    "dense": lambda: _random((17, 9, 66), 36, solid=0.65),     # narrower ways: smaller components, other handovers
}
RAW_NAMES = list(RAW)
RAW_CASES = [(name, axis, up) for name in RAW_NAMES for axis, up in DIRECTIONS]


@functools.lru_cache(maxsize=None)
def raw_ids(name):
    ids = numpy.ascontiguousarray(RAW[name]())
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def raw_labels(name, axis):
    out = layer_labels(raw_ids(name) == EMPTY, axis)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def raw_reference(name, axis, up):
    return reference_of(raw_ids(name), RAW_PARTS, axis, up)
