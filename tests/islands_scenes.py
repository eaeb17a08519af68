"""The scenarios and the CPU references of the islands tests (test_islands_host.py proves on the CPU that each scenario holds what
it is there for; test_gpu_islands.py runs them on the device).

`grounded_set(s, axis, up)` is written from the definition in codecad_amd/islands.py alone: the seeds -- S in layer h0 -- and
then G grown by shifted arrays, "the sample below or a lateral neighbour is in G", to its fixed point.  `layered_grounded` is
the second way: every layer's 4-connected components by flood fill (drainage_scenes.layer_labels), a layer component grounded
when one of its samples has a grounded sample below, upwards once.  `synchronous(s, axis, up, k)` is what the seeds and k
synchronous steps over all (sample, below) pairs leave flagged when whole layer components carry the flags, as on the device.
A, J, the counts, the islands (the flood fill of assembly_components_scenes on the floating ids) and their four host fields
follow from F by shifted slices.

The scenes are boxes on the lattice in SAMPLE units at step 1/16, built with disassembly_scenes' helpers; the ball over a slab
and the single block are that module's own.  RAW volumes are id arrays that no assembly gives, for the entry points alone.
"""
import collections
import functools

import numpy

import assembly_components_scenes as comp
import disassembly_scenes as dis_scenes
import overhangs_scenes as over
from disassembly_scenes import _scene, DIRECTIONS
from drainage_scenes import shifted, layers, layer_labels, _box
from assembly_components_scenes import SOLID, NONE, EMPTY

Reference = collections.namedtuple("Reference", "ids s first_layer grounded floating floating_ids start_ids join_ids floating_counts "
                                                "start_counts join_counts islands labels")
# an island of the reference: the Expected of assembly_components_scenes and the four fields the host adds, `owners` as indices
RefIsland = collections.namedtuple("RefIsland", "expected first_layer starts loose")
# `frame`: the lattice the parts span, or None for a scene of another module; `runs`: the (axis, up, of) the device runs;
# `floating`: {(axis, up, of): the floating samples} written by hand
Scene = collections.namedtuple("Scene", "build frame runs floating")
NZ = 138                                                                            # two words and a ragged tail under pz = 144


# ---- the references ---------------------------------------------------------------------------------------------------

def in_set_of(ids, of):
    return over.in_set_of(ids, of)


def first_layer(s, axis, up):
    """h0: the least layer that holds a sample of S, n_a when S is empty."""
    return int(layers(s.shape, axis, up)[s].min()) if s.any() else s.shape[axis]


def seeds(s, axis, up):
    return s & (layers(s.shape, axis, up) == first_layer(s, axis, up))


def grounded_set(s, axis, up):
    """G from the definition: grown by shifted arrays to the fixed point."""
    sign = 1 if up else -1
    g = seeds(s, axis, up)
    while True:
        grown = shifted(g, axis, sign)                                              # the sample below is in G
        for a in range(3):
            if a != axis:
                grown = grown | shifted(g, a, 1) | shifted(g, a, -1)
        grown = g | (s & grown)
        if numpy.array_equal(grown, g):
            return g
        g = grown


def layered_grounded(s, axis, up, labels=None):
    """G the second way: the layers from h0 up, in each the components that hold a seed or a sample over a grounded one."""
    labels = layer_labels(s, axis) if labels is None else labels
    first = seeds(s, axis, up)
    g = numpy.zeros(s.shape, dtype=bool)
    na = s.shape[axis]
    for h in range(na):
        here = [slice(None)] * 3
        here[axis] = h if up else na - 1 - h
        here = tuple(here)
        start = first[here].copy()
        if h > 0:
            under = [slice(None)] * 3
            under[axis] = h - 1 if up else na - h
            start |= s[here] & g[tuple(under)]
        g[here] = s[here] & numpy.isin(labels[here], numpy.unique(labels[here][start]))
    return g


def synchronous(s, axis, up, k, labels=None):
    """The samples under a flagged component after the seeds and k synchronous steps: a step flags the component of every p of S
    whose sample below lay under a flagged component before the step."""
    labels = layer_labels(s, axis) if labels is None else labels
    sign = 1 if up else -1
    g = s & numpy.isin(labels, numpy.unique(labels[seeds(s, axis, up)]))
    for _ in range(k):
        above = s & shifted(g, axis, sign) & ~g
        if not above.any():
            break
        g = g | (s & numpy.isin(labels, numpy.unique(labels[above])))
    return g


def reference_of(ids, n, axis, up, of=SOLID):
    s = in_set_of(ids, of)
    sign = 1 if up else -1
    g = grounded_set(s, axis, up)
    f = s & ~g
    a = f & ~shifted(s, axis, sign)                                                 # the sample below is not in S
    j = f & shifted(g, axis, -sign)                                                 # the sample above is in G
    volumes = [numpy.where(m, ids, EMPTY).astype(numpy.uint8) for m in (f, a, j)]
    found = comp.reference_components(volumes[0], SOLID)
    h = layers(ids.shape, axis, up)
    islands = [RefIsland(e, int(h[found.labels == e.label].min()), int((a & (found.labels == e.label)).sum()),
                         not bool((j & (found.labels == e.label)).any())) for e in found.components]
    for m in [s, g, f] + volumes:
        m.setflags(write=False)
    return Reference(ids, s, first_layer(s, axis, up), g, f, volumes[0], volumes[1], volumes[2],
                     *([int((v == k).sum()) for k in range(n)] for v in volumes), islands, found.labels)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _mine(name, frame, solids, runs, floating):
    return Scene(_scene(name, frame, solids, {}).build, frame, runs, floating)


ALL = [(axis, up, SOLID) for axis, up in DIRECTIONS]
Z = [(2, True, SOLID), (2, False, SOLID)]
ZX = Z + [(0, True, SOLID)]
TABLE = (12, 10, 14)
PEG = (14, 10, NZ)
ARCH = (12, 4, 20)
CAGE = (10, 10, 10)
EDGE = (8, 8, 6)
ZIGZAG = (13, 3, 13)
FIRSTS = (15, 5, 70)
FIRST_LAYERS = (63, 64, 65)
JOIN = (10, 4, 70)
PLATE = (20, 20, 6)
RAISED = (10, 6, 8)
FEET = (10, 4, 8)


def _cage(ball):
    n = CAGE[0]
    walls = [((0, 0, 0), (n, n, 1)), ((0, 0, n - 1), (n, n, n)), ((0, 0, 1), (1, n, n - 1)), ((n - 1, 0, 1), (n, n, n - 1)),
             ((1, 0, 1), (n - 1, 1, n - 1)), ((1, n - 1, 1), (n - 1, n, n - 1))]
    return [walls, [ball]]


def _scenes():
    out = {}
    # a table: four legs and a top; grounded upwards from its feet and downwards from its top
    legs = [((x, y, 0), (x + 2, y + 2, 10)) for x in (0, 10) for y in (0, 8)]
    out["table"] = _mine("table", TABLE, [legs + [((0, 0, 10), (12, 10, 14))]], ZX, {(2, True, SOLID): set(), (2, False, SOLID): set()})
    # a frame -- floor, two walls, ceiling -- with a peg hanging from its ceiling: upwards the peg floats, with starts on its
    # underside and joins in its top layer; downwards everything hangs from the ceiling, which is layer 0
    frame = [((0, 0, 0), (14, 10, 2)), ((0, 0, 2), (2, 10, 134)), ((12, 0, 2), (14, 10, 134)), ((0, 0, 134), (14, 10, NZ))]
    peg = ((6, 4, 100), (8, 6, 134))
    out["peg"] = _mine("peg", PEG, [frame, [peg]], ZX, {(2, True, SOLID): _box(*peg), (2, False, SOLID): set()})
    # an inverted U with unequal legs: the short leg floats until the bridge is laid over it
    short = ((10, 0, 6), (12, 4, 16))
    out["arch"] = _mine("arch", ARCH, [[((0, 0, 0), (2, 4, 20)), ((0, 0, 16), (12, 4, 20)), short]], ALL,
                        {(2, True, SOLID): _box(*short), (2, False, SOLID): set()})
    # a captive ball in a closed cage: loose in every direction; resting on the cage's floor by a face it is grounded upwards
    ball = ((4, 4, 4), (6, 6, 6))
    out["ball_captive"] = _mine("captive", CAGE, _cage(ball), ALL, {(axis, up, SOLID): _box(*ball) for axis, up in DIRECTIONS})
    resting = ((4, 4, 1), (6, 6, 3))
    out["ball_resting"] = _mine("resting", CAGE, _cage(resting), Z, {(2, True, SOLID): set(), (2, False, SOLID): _box(*resting)})
    # two boxes that meet only along the edge x = 4, z = 3, the second in the layer after the first's last: the 6-neighbourhood
    low, high = ((0, 0, 0), (4, 8, 3)), ((4, 0, 3), (8, 8, 6))
    out["edge"] = _mine("edge", EDGE, [[low], [high]], ALL + [(2, True, 1), (0, False, 0)],
                        {(2, True, SOLID): _box(*high), (2, False, SOLID): _box(*low), (0, True, SOLID): _box(*high),
                         (0, False, SOLID): _box(*low), (1, True, SOLID): set(), (1, False, SOLID): set(), (2, True, 1): set(),
                         (0, False, 0): set()})
    # a zigzag wall: bars along x at z = 0, 4, 8, 12 joined by posts at alternating ends; ground goes up, sideways and up again
    bars = [((0, 0, z), (13, 3, z + 1)) for z in (0, 4, 8, 12)]
    posts = [((12, 0, 1), (13, 3, 4)), ((0, 0, 5), (1, 3, 8)), ((12, 0, 9), (13, 3, 12))]
    out["zigzag"] = _mine("zigzag", ZIGZAG, [bars + posts], ALL, {(axis, up, SOLID): set() for axis, up in DIRECTIONS})
    # three loose blocks whose first layers are z = 63, 64 and 65: the last layer of word 0 and the first two of word 1
    blocks = [((1 + 5 * k, 1, z), (4 + 5 * k, 4, z + 3)) for k, z in enumerate(FIRST_LAYERS)]
    out["firsts"] = _mine("firsts", FIRSTS, [[((0, 0, 0), (15, 5, 2)), ((0, 0, 2), (1, 1, 70))], blocks], ZX,
                          {(2, True, SOLID): set().union(*(_box(*b) for b in blocks)), (2, False, SOLID): set().union(*(_box(*b) for b in blocks))})
    # joins across the word edge: upwards a short leg whose top, z = 63, lies under the bridge's z = 64 ...
    leg = ((8, 0, 40), (10, 4, 64))
    out["join_up"] = _mine("joinup", JOIN, [[((0, 0, 0), (2, 4, 70)), ((0, 0, 64), (10, 4, 68)), leg]], Z,
                           {(2, True, SOLID): _box(*leg), (2, False, SOLID): set()})
    # ... and mirrored for up=False: a stub on top of the bridge, laid before it, whose z = 64 lies over the bridge's z = 63
    stub = ((8, 0, 64), (10, 4, 68))
    out["join_down"] = _mine("joindown", JOIN, [[((0, 0, 0), (2, 4, 70)), ((0, 0, 60), (10, 4, 64)), stub]], Z,
                             {(2, True, SOLID): set(), (2, False, SOLID): _box(*stub)})
    # a plate on one small pillar: its layer component crosses tile faces on both lateral axes, and a loose block over it
    out["plate"] = _mine("plate", PLATE, [[((0, 0, 0), (2, 2, 3)), ((0, 0, 3), (20, 20, 4))], [((15, 15, 5), (18, 18, 6))]], ALL,
                         {(2, True, SOLID): _box((15, 15, 5), (18, 18, 6))})
    # part 1 alone starts at layer 3, above empty layers, and has a second body that starts at layer 5
    second = ((6, 0, 5), (10, 6, 8))
    out["raised"] = _mine("raised", RAISED, [[((0, 0, 0), (10, 6, 3))], [((0, 0, 3), (4, 6, 8)), second]], [(2, True, 1), (2, True, SOLID), (0, True, 1)],
                          {(2, True, 1): _box(*second), (2, True, SOLID): _box(*second)})
    # a part with two feet at different heights on a stepped base: grounded as one solid; alone, the higher foot floats
    base = [((0, 0, 0), (5, 4, 2)), ((5, 0, 0), (10, 4, 4))]
    foot = ((7, 0, 4), (9, 4, 6))
    out["feet"] = _mine("feet", FEET, [base, [((0, 0, 6), (10, 4, 8)), ((1, 0, 2), (3, 4, 6)), foot]], [(2, True, SOLID), (2, True, 1), (2, False, 1)],
                        {(2, True, SOLID): set(), (2, True, 1): _box(*foot)})
    return out


MINE = _scenes()
SCENES = dict(MINE)
SCENES["ball_over_slab"] = Scene(dis_scenes.SCENES["ownership"].build, None, Z + [(2, True, 1)], {})     # three owners
SCENES["nothing"] = Scene(dis_scenes.SCENES["single"].build, None, ALL, {(axis, up, SOLID): set() for axis, up in DIRECTIONS})
NAMES = list(SCENES)
CASES = [(name,) + run for name in NAMES for run in SCENES[name].runs]
_OTHER = {"ball_over_slab": "ownership", "nothing": "single"}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scene."""
    if name in _OTHER:
        return dis_scenes.scene(_OTHER[name])
    asm = SCENES[name].build()
    instances = dis_scenes._instance_cells.visible(asm, dis_scenes.STEP)
    corner, step, dims = dis_scenes._instance_cells.checked_lattice(instances, dis_scenes.STEP)
    return asm, dis_scenes.STEP, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def part_ids(name):
    """The dense part ids of a scene, every instance evaluated at every sample, once."""
    if name in _OTHER:
        return dis_scenes.part_ids(_OTHER[name])
    asm, resolution, instances, corner, step, dims = scene(name)
    ids, counts = dis_scenes.voxels.dense_ids([w < 0 for w in dis_scenes.mass.dense_fields(instances, corner, step, dims)])
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def labels_of(name, axis, of=SOLID):
    """The layer labels of a scene's S along an axis, computed once."""
    out = layer_labels(in_set_of(part_ids(name), of), axis)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, axis, up, of=SOLID):
    """The Reference of a case, computed once and shared; nobody changes it."""
    return reference_of(part_ids(name), len(scene(name)[2]), axis, up, of)


# ---- raw id volumes, for the entry points alone -----------------------------------------------------------------------

RAW_PARTS = 64


def _random(shape, seed, solid, parts=RAW_PARTS):
    rng = numpy.random.default_rng(seed)
    ids = rng.integers(0, parts, size=shape).astype(numpy.uint8)
    return numpy.where(rng.random(shape) < solid, ids, EMPTY).astype(numpy.uint8)


def _raised(shape, seed, solid):
    """Nothing in the first three layers of z and the first two of x, from either end."""
    ids = _random(shape, seed, solid)
    ids[:, :, :3] = ids[:, :, -3:] = EMPTY
    ids[:2] = ids[-2:] = EMPTY
    return ids


# the densities leave both F and G non-empty in the directions test_islands_host.py names
RAW = {
    "19x21x70": lambda: _random((19, 21, 70), 41, 0.5),        # three tiles a lateral axis, ragged on all; a word and six samples
    "9x8x130": lambda: _random((9, 8, 130), 42, 0.5),          # two words and two samples; one tile and one sample along x
    "raised": lambda: _raised((12, 9, 70), 43, 0.5),           # h0 = 3 along z, 2 along x, 0 along y
    "two_ids": lambda: _random((17, 9, 66), 44, 0.9, parts=2),     # of = 1: the samples of id 0 stand right under it and beside it
    "line_z": lambda: _random((1, 1, 130), 45, 0.7),
    "line_y": lambda: _random((1, 21, 1), 46, 0.7),
    "line_x": lambda: _random((19, 1, 1), 47, 0.7),
    "sample_empty": lambda: numpy.full((1, 1, 1), EMPTY, dtype=numpy.uint8),
    "sample_solid": lambda: numpy.zeros((1, 1, 1), dtype=numpy.uint8),
}
RAW_OF = {"two_ids": 1}
RAW_NAMES = list(RAW)
RAW_CASES = [(name, axis, up, RAW_OF.get(name, SOLID)) for name in RAW_NAMES for axis, up in DIRECTIONS]
BOTH_SETS = ["19x21x70", "9x8x130", "raised", "two_ids"]                            # F and G are non-empty in all six directions


@functools.lru_cache(maxsize=None)
def raw_ids(name):
    ids = numpy.ascontiguousarray(RAW[name]())
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def raw_labels(name, axis, of=SOLID):
    out = layer_labels(in_set_of(raw_ids(name), of), axis)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def raw_reference(name, axis, up, of=SOLID):
    return reference_of(raw_ids(name), RAW_PARTS, axis, up, of)
