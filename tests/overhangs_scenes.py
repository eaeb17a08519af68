"""The scenarios and the CPU reference of the overhang tests (test_overhangs_host.py proves on the CPU that each scenario holds
the edge it is there for; test_gpu_overhangs.py runs them on the device).

`reference_overhangs(ids, axis, up, reach_sq, of, n)` (n instances) is written from the definitions in codecad_amd/overhangs.py
alone.  It starts from the dense part ids of assembly_voxels_scenes.reference_voxels and
  * O is S above h0 AND, over the offsets of N, "S shifted by the offset is empty" (outside the lattice nothing is in S),
  * P and L come from a search along every line: for a sample p, t = 1, 2, ... until p + t s e is in S or leaves the lattice,
  * the support structures come from assembly_components_scenes.reference_components' flood fill on the support ids.
`accumulated_overhangs` is the second way: the nearest sample of S above every sample by numpy.maximum.accumulate along the
axis.  `canonical_overhangs` is the third: every direction stated as the +z rule on the transposed and flipped ids.

The scenarios are blocks in SAMPLE units at step 1/16, built with assembly_components_scenes._cut and _box.  Every one is a few
tens of samples across and NZ = 138 samples high (136 for the ball): a line along z spans three 64-sample words of the device
buffer and its padding, pz = 144, lies next to data.
"""
import collections
import functools

import numpy

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_components_scenes as comp
import assembly_voxels_scenes as voxels
from assembly_components_scenes import _cut, _box, STEP, SOLID, NONE, EMPTY

NZ = 138
MAX_REACH = 2                   # |u|, |v| <= 2 for every reach_sq <= 8

Reference = collections.namedtuple("Reference", "ids in_set first_layer overhang_ids support_ids landing_ids overhang_counts "
                                                "support_counts landing_counts plate_landings supports labels")
Case = collections.namedtuple("Case", "name scene axis up reach_sq of nonempty")


# ---- the reference ----------------------------------------------------------------------------------------------------

def in_set_of(ids, of):
    return (ids != EMPTY) if of == SOLID else (ids == of)


def offsets(reach_sq):
    """The lateral offsets (u, v) of N."""
    return [(u, v) for u in range(-MAX_REACH, MAX_REACH + 1) for v in range(-MAX_REACH, MAX_REACH + 1) if u * u + v * v <= reach_sq]


def layers(shape, axis, up):
    """int64[nx, ny, nz]: h(p)."""
    along = numpy.indices(shape)[axis]
    return along if up else shape[axis] - 1 - along


def overhang_set(s, axis, up, reach_sq):
    """(h0, O) of the set S."""
    shape, sign = s.shape, 1 if up else -1
    h = layers(shape, axis, up)
    h0 = int(h[s].min()) if s.any() else shape[axis]
    pad = MAX_REACH + 1
    padded = numpy.pad(s, pad)                                                    # nothing outside the lattice is in S
    lateral = [a for a in range(3) if a != axis]
    o = s & (h > h0)
    for u, v in offsets(reach_sq):
        off = [0, 0, 0]
        off[axis], off[lateral[0]], off[lateral[1]] = -sign, u, v
        o &= ~padded[tuple(slice(pad + off[a], pad + off[a] + shape[a]) for a in range(3))]
    return h0, o


def searched_columns(ids, s, o, h0, axis, up):
    """(support_ids, landing_ids) by a search along every line: every line at once, one step t at a time."""
    shape, sign = s.shape, 1 if up else -1
    h = layers(shape, axis, up)
    at = numpy.indices(shape)
    support = numpy.full(shape, EMPTY, dtype=numpy.uint8)
    searching = ~s & (h >= h0)                                                    # the samples whose holder is still unknown
    for t in range(1, shape[axis]):
        q = [a.copy() for a in at]
        q[axis] = q[axis] + t * sign
        inside = (q[axis] >= 0) & (q[axis] < shape[axis])
        searching &= inside                                                       # the line left the lattice: no holder
        if not searching.any():
            break
        q[axis] = numpy.clip(q[axis], 0, shape[axis] - 1)
        found = searching & s[tuple(q)]                                           # the least t: the nearest sample of S above
        held = found & o[tuple(q)]
        support[held] = ids[tuple(q)][held]
        searching &= ~found
    above = [a.copy() for a in at]
    above[axis] = numpy.clip(above[axis] + sign, 0, shape[axis] - 1)
    has_above = h < shape[axis] - 1
    lands = s & has_above & (support[tuple(above)] != EMPTY)
    return support, numpy.where(lands, ids, EMPTY).astype(numpy.uint8)


def _finish(ids, s, h0, o, support, landing, axis, up, n):
    h = layers(ids.shape, axis, up)
    over = numpy.where(o, ids, EMPTY).astype(numpy.uint8)
    found = comp.reference_components(support, SOLID)
    for a in (over, support, landing):
        a.setflags(write=False)
    return Reference(ids, s, h0, over, support, landing, [int((over == k).sum()) for k in range(n)],
                     [int((support == k).sum()) for k in range(n)], [int((landing == k).sum()) for k in range(n)],
                     int(((support != EMPTY) & (h == h0)).sum()), found.components, found.labels)


def reference_overhangs(ids, axis, up, reach_sq, of, n):
    s = in_set_of(ids, of)
    h0, o = overhang_set(s, axis, up, reach_sq)
    support, landing = searched_columns(ids, s, o, h0, axis, up)
    return _finish(ids, s, h0, o, support, landing, axis, up, n)


def accumulated_overhangs(ids, axis, up, reach_sq, of):
    """(h0, overhang_ids, support_ids, landing_ids) the second way: the position of the nearest sample of S above, per line, by
    a running maximum from the top of the build direction."""
    s = in_set_of(ids, of)
    h0, o = overhang_set(s, axis, up, reach_sq)
    # lines as rows, the TOP layer first: r = n_a - 1 - h
    rows = lambda a: numpy.moveaxis(a if not up else numpy.flip(a, axis), axis, -1)   # noqa: E731
    rs, ro, rid = rows(s), rows(o), rows(ids)
    na = rs.shape[-1]
    r = numpy.arange(na)
    last = numpy.maximum.accumulate(numpy.where(rs, r, -1), axis=-1)              # the nearest sample of S at or above r
    nearest = numpy.concatenate([numpy.full(rs.shape[:-1] + (1,), -1), last[..., :-1]], axis=-1)   # ... strictly above
    have = nearest >= 0
    q = numpy.clip(nearest, 0, na - 1)
    held = ~rs & have & numpy.take_along_axis(ro, q, axis=-1) & ((na - 1 - r) >= h0)
    support = numpy.where(held, numpy.take_along_axis(rid, q, axis=-1), EMPTY).astype(numpy.uint8)
    above_held = numpy.concatenate([numpy.zeros(rs.shape[:-1] + (1,), bool), held[..., :-1]], axis=-1)
    landing = numpy.where(rs & above_held, rid, EMPTY).astype(numpy.uint8)
    back = lambda a: (lambda m: m if not up else numpy.flip(m, axis))(numpy.moveaxis(a, -1, axis))   # noqa: E731
    return h0, numpy.where(o, ids, EMPTY).astype(numpy.uint8), back(support), back(landing)


def canonical_overhangs(ids, axis, up, reach_sq, of, n):
    """(h0, overhang_ids, support_ids, landing_ids) the third way: the axis moved to z and flipped to point up, the +z rule
    there, and the answer moved back.  N is symmetric, so the order of the other two axes does not matter."""
    to = lambda a: (lambda m: m if up else numpy.flip(m, 2))(numpy.moveaxis(a, axis, 2))          # noqa: E731
    back = lambda a: numpy.moveaxis(a if up else numpy.flip(a, 2), 2, axis)                       # noqa: E731
    ref = reference_overhangs(numpy.ascontiguousarray(to(ids)), 2, True, reach_sq, of, n)
    return ref.first_layer, back(ref.overhang_ids), back(ref.support_ids), back(ref.landing_ids)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _solid(n, boxes, swap=False):
    """The union of the boxes [lo, hi) of a frame of `n` samples; `swap` exchanges x and y."""
    flip = (lambda p: (p[1], p[0], p[2])) if swap else (lambda p: tuple(p))
    return shapes.union([_box(flip(n), flip(lo), flip(hi)) for lo, hi in boxes])


def _one(name, shape):
    return cc.assembly(name, [shape.make_part(name)])


CUBOID = (12, 10, NZ)


def _cuboid():
    return _one("cuboid", _box(CUBOID, (0, 0, 0), CUBOID))


STAIR_SIDE, STAIR_BASE, STAIR_LAYERS = 4, 58, 12        # layers z = 58..69: across the word edge 63 | 64
STAIRS = {"stairs_x": (1, 0), "stairs_diagonal": (1, 1), "stairs_run2": (2, 0), "stairs_2_1": (2, 1), "stairs_2_2": (2, 2)}
#          scene: (empty from this reach_sq on, not at this one)
STAIR_THRESHOLDS = {"stairs_x": (1, 0), "stairs_diagonal": (2, 1), "stairs_run2": (4, 2), "stairs_2_1": (5, 4), "stairs_2_2": (8, 5)}


def _stairs(rx, ry):
    """A pillar, a staircase of twelve layers of 4 x 4 samples, each moved by (rx, ry) against the one below, and a pillar on
    its last layer up to the top of the lattice: the far corner of a layer finds the layer below at (-rx, -ry) and no nearer."""
    t, zb, k = STAIR_SIDE, STAIR_BASE, STAIR_LAYERS
    n = ((k - 1) * rx + t, (k - 1) * ry + t, NZ)
    boxes = [((0, 0, 0), (t, t, zb))]
    boxes += [((j * rx, j * ry, zb + j), (j * rx + t, j * ry + t, zb + j + 1)) for j in range(k)]
    boxes += [(((k - 1) * rx, (k - 1) * ry, zb + k), n)]
    return _one("stairs", _solid(n, boxes))


TEE = (16, 8, NZ)


def _tee():
    """A stem of 130 samples and a bar of 8 on it: the bar's underside hangs, its supports go down to the plate through all
    three words, and their lines hold no solid in the two lower ones."""
    return _one("tee", _solid(TEE, [((6, 2, 0), (10, 6, 130)), ((0, 0, 130), (16, 8, NZ))]))


BRIDGE = (16, 8, NZ)


def _bridge():
    """Two piers, a deck across them and a block of 20 samples on the plate under the deck: the supports over the block start
    in the top word, cross the middle word, which holds no solid on their lines, and land in the bottom word."""
    return _one("bridge", _solid(BRIDGE, [((0, 0, 0), (3, 8, 132)), ((13, 0, 0), (16, 8, 132)), ((0, 0, 132), (16, 8, NZ)),
                                          ((6, 2, 0), (9, 6, 20))]))


BALL = (24, 24, 136)
BALL_RADIUS, BALL_CENTRE = 10, (12, 12, 126)


def _ball():
    """Part 0, a cap: a block that holds the lowest samples of the ball and so owns them.  Part 1: the ball, and a pad on the
    plate that puts its own first layer at 0.  Part 2: a slab between them.  The ball's underside hangs; its supports land on
    the slab; under the cap they are held for part 0; alone (of=1) the ball's supports pass through the slab to the plate."""
    centre = [(c - m / 2) * STEP for c, m in zip(BALL_CENTRE, BALL)]
    ball = shapes.union([shapes.sphere(r=BALL_RADIUS * STEP).translated(*centre), _box(BALL, (0, 0, 0), (3, 3, 2))])
    cap = _box(BALL, (10, 10, 114), (14, 14, 118))
    slab = _box(BALL, (0, 0, 10), (24, 24, 16))
    return cc.assembly("ball", [cap.make_part("cap"), ball.make_part("ball"), slab.make_part("slab")])


WORDS = (16, 8, NZ)
WORD_EDGES = (63, 64, 127, 128)


def _words():
    """A floor and a roof of two samples, a pillar between them (lines whose three words are wholly solid), and ledges one
    sample thick, y in [2, 5), on lines two apart in x:
      x = 0: at z = 63 and 127, the last samples of a word;  x = 2: at z = 64 and 128, the first;
      x = 4: at z = 130: its column starts in the top word, crosses the middle one and ends on the floor;
      x = 6: at z = 50, 40, 30 and 20, and x = 7: at z = 39, which holds (6, y, 40) at reach_sq >= 1: on (6, y) the column of 50
             lands on 40, the line is CLOSED from 39 to 31, reopens under 30, lands on 20 and reopens once more, all in word 0;
      x = 8: a block z in [60, 70) across the word edge;  x = 10: at z = 3 (a column of one sample) and at z = 135, under the roof.
    Upwards the roof hangs over every line, downwards the floor does."""
    boxes = [((0, 0, 0), (16, 8, 2)), ((0, 0, 136), (16, 8, NZ)), ((14, 0, 2), (16, 8, 136))]
    ledge = lambda x, z0, z1=None: ((x, 2, z0), (x + 1, 5, z0 + 1 if z1 is None else z1))          # noqa: E731
    boxes += [ledge(0, 63), ledge(0, 127), ledge(2, 64), ledge(2, 128), ledge(4, 130)]
    boxes += [ledge(6, z) for z in (50, 40, 30, 20)] + [ledge(7, 39), ledge(8, 60, 70), ledge(10, 3), ledge(10, 135)]
    return _one("words", _solid(WORDS, boxes))


RAISED = (12, 8, NZ)
RAISED_FIRST = 5


def _raised():
    """A block whose five lowest layers are cut away -- h0 = 5 upwards, with empty layers beneath -- and which touches the top
    of the lattice; a pocket x < 4 under z = 100 leaves an overhang whose supports must stop at h0, and a pocket x >= 8 over
    z = 60 leaves one for the way down."""
    return _one("raised", _cut(RAISED, [((0, 0, 0), (12, 8, RAISED_FIRST)), ((0, 0, RAISED_FIRST), (4, 8, 100)), ((8, 0, 60), (12, 8, NZ))]))


LATERAL = (10, 12, NZ)


def _lateral(swap=False):
    """For a print along x (along y with `swap`): a plate x in [0, 2); a staircase of eight layers along x that moves two
    samples along +z a layer, from z = 56 across 63 | 64; and two ledges that float at x = 6, at z = 0..2 and at z = 135..137:
    their lateral taps leave the lattice at both ends of z."""
    boxes = [((0, 0, 0), (2, 12, NZ))]
    boxes += [((2 + k, 2, 56 + 2 * k), (3 + k, 5, 62 + 2 * k)) for k in range(8)]
    boxes += [((6, 7, 0), (8, 10, 3)), ((6, 7, 135), (8, 10, NZ))]
    return _one("lateral", _solid(LATERAL, boxes, swap))


SIX = (14, 18, NZ)


def _six():
    """Two parts, no symmetry: part 0 a base, a column and an arm; part 1 a block that floats over the base and a post through
    the arm's end up to the top of the lattice (the arm owns what both contain)."""
    first = _solid(SIX, [((0, 0, 0), (14, 18, 3)), ((0, 0, 3), (4, 5, 134)), ((0, 0, 120), (11, 5, 126))])
    second = _solid(SIX, [((6, 8, 60), (12, 16, 70)), ((8, 2, 124), (11, 7, NZ))])
    return cc.assembly("six", [first.make_part("frame"), second.make_part("rider")])


SCENES = {"cuboid": _cuboid, "tee": _tee, "bridge": _bridge, "ball": _ball, "words": _words, "raised": _raised,
          "lateral_x": _lateral, "lateral_y": functools.partial(_lateral, True), "six": _six}
for _name, (_rx, _ry) in STAIRS.items():
    SCENES[_name] = functools.partial(_stairs, _rx, _ry)

DIRECTIONS = [(axis, up) for axis in range(3) for up in (True, False)]


def _case(scene, axis, up, reach_sq, of, nonempty):
    name = "%s_%s%s_r%d%s" % (scene, "xyz"[axis], "+" if up else "-", reach_sq, "" if of == SOLID else "_of%d" % of)
    return Case(name, scene, axis, up, reach_sq, of, nonempty)


# `nonempty`: the sets the case must leave non-empty, of O, P, L and G (the plate landings); a case that does not name O has
# no overhang at all
CASES = [
    _case("cuboid", 2, True, 1, SOLID, ""), _case("cuboid", 0, True, 0, SOLID, ""), _case("cuboid", 1, False, 8, SOLID, ""),
    _case("tee", 2, True, 1, SOLID, "OPG"), _case("tee", 2, False, 1, SOLID, ""), _case("tee", 0, True, 1, SOLID, "OPG"),
    _case("bridge", 2, True, 1, SOLID, "OPLG"), _case("bridge", 2, False, 1, SOLID, "OPL"), _case("bridge", 1, True, 2, SOLID, "OPG"),
    _case("ball", 2, True, 1, SOLID, "OPL"), _case("ball", 2, True, 1, 1, "OPG"), _case("ball", 2, True, 1, 0, ""),
    _case("ball", 2, False, 2, SOLID, "OPLG"), _case("ball", 0, True, 1, SOLID, "OPG"),
    _case("words", 2, True, 1, SOLID, "OPL"), _case("words", 2, False, 1, SOLID, "OPL"), _case("words", 2, True, 0, SOLID, "OPL"),
    _case("words", 2, False, 8, SOLID, "OPL"), _case("words", 1, True, 1, SOLID, "OPG"),
    _case("raised", 2, True, 1, SOLID, "OPG"), _case("raised", 2, False, 1, SOLID, "OPG"), _case("raised", 0, False, 1, SOLID, "OPG"),
    _case("lateral_x", 0, True, 1, SOLID, "OPL"), _case("lateral_x", 0, False, 1, SOLID, "OPLG"), _case("lateral_x", 0, True, 4, SOLID, "OPL"),
    _case("lateral_x", 0, True, 0, SOLID, "OPL"), _case("lateral_y", 1, True, 1, SOLID, "OPL"), _case("lateral_y", 1, False, 1, SOLID, "OPLG"),
    _case("lateral_y", 1, True, 5, SOLID, "OPL"),
]
for _name, (_clean, _not) in STAIR_THRESHOLDS.items():
    CASES += [_case(_name, 2, True, _clean, SOLID, ""), _case(_name, 2, True, _not, SOLID, "OPG")]
CASES += [_case("stairs_2_1", 2, False, 5, SOLID, ""), _case("stairs_2_1", 2, False, 4, SOLID, "OPG")]
SIX_NONEMPTY = {(0, True): "OPLG", (0, False): "OPLG", (1, True): "OPG", (1, False): "OPG", (2, True): "OPL", (2, False): "OPLG"}
SIX_CASES = [_case("six", axis, up, 1, SOLID, SIX_NONEMPTY[axis, up]) for axis, up in DIRECTIONS]
CASES += SIX_CASES + [_case("six", 2, True, 8, SOLID, "OPL"), _case("six", 2, True, 1, 1, "OPG"), _case("six", 0, False, 1, 0, "OPG")]
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
    return reference_overhangs(part_ids(c.scene), c.axis, c.up, c.reach_sq, c.of, len(scene(c.scene)[2]))
