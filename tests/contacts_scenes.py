"""The scenarios and the CPU reference of the contact tests (test_contacts_host.py proves on the CPU that each scenario holds
the entries it is there for; test_gpu_contacts.py runs them on the device).

`reference_faces(ids, n)` is written from the definitions in codecad_amd/contacts.py alone, over a `part_ids` array: per axis the
ids and the ids shifted by one sample (two slices), and per ordered pair the `argwhere` of "i here, j right above" -- its
length, its sums, its extremes and its first row, which is the lexicographically first p.  The exposed counts compare against
the ids padded with 255 on every side (nothing outside the lattice is inside any part), the interface samples take the six
shifted comparisons, and the patches come from assembly_components_scenes.reference_components' flood fill on the contact ids.
`running_faces` is the second way: a walk up every line of an axis that records where a run of one id ends and the next begins.

The scenes are every SMALL scene of disassembly_scenes.py, untouched, and boxes on the lattice in SAMPLE units at step 1/16
built with that module's helpers.  RAW volumes are id arrays that no assembly gives, for the kernel alone.
"""
import collections
import functools

import numpy

import assembly_components_scenes as comp
import disassembly_scenes as dis_scenes
from disassembly_scenes import _scene, NZ, NEVER
from assembly_components_scenes import SOLID, NONE, EMPTY

Reference = collections.namedtuple("Reference", "ids counts faces index_sums box witness exposed contact_ids contact_counts patches labels")
# `by_hand`: {(axis, i, j): (faces, (lowest p, highest p), witness)} written by hand; `exposed`: {(axis, side, i): count} by hand;
# `patches`: [parts of each patch, ordered by label] by hand, or None; `groups`, `loose`: what the report's methods must give
Scene = collections.namedtuple("Scene", "scene by_hand exposed patches groups loose")


# ---- the reference ----------------------------------------------------------------------------------------------------

def _along(axis, sl):
    out = [slice(None)] * 3
    out[axis] = sl
    return tuple(out)


def reference_faces(ids, n):
    """(faces, index_sums, box, witness, exposed, contact_ids, contact_counts) from the definitions."""
    faces = numpy.zeros((3, n, n), dtype=numpy.uint64)
    sums = numpy.zeros((3, n, n, 3), dtype=numpy.uint64)
    box = numpy.full((3, n, n, 2, 3), -1, dtype=numpy.int32)
    witness = numpy.full((3, n, n, 3), -1, dtype=numpy.int32)
    exposed = numpy.zeros((3, 2, n), dtype=numpy.uint64)
    padded = numpy.pad(ids, 1, constant_values=EMPTY)
    inner = tuple(slice(1, -1) for _ in range(3))
    meets = numpy.zeros(ids.shape, dtype=bool)
    for axis in range(3):
        here, above = ids[_along(axis, slice(None, -1))], ids[_along(axis, slice(1, None))]          # p and p + e_a, both inside
        touch = (here != EMPTY) & (above != EMPTY) & (here != above)
        for i, j in sorted(set(zip(here[touch].tolist(), above[touch].tolist()))):
            at = numpy.argwhere((here == i) & (above == j))                                         # C order: the first is the witness
            faces[axis, i, j] = len(at)
            sums[axis, i, j] = at.sum(axis=0)
            box[axis, i, j] = [at.min(axis=0), at.max(axis=0)]
            witness[axis, i, j] = at[0]
        for side, shift in ((0, 1), (1, -1)):
            beyond = numpy.roll(padded, -shift, axis=axis)[inner]                                   # ids[p + shift e_a], 255 outside
            exposed[axis, side] = [int(((ids == i) & (beyond == EMPTY)).sum()) for i in range(n)]
            meets |= (ids != EMPTY) & (beyond != EMPTY) & (beyond != ids)
    contact_ids = numpy.where(meets, ids, EMPTY).astype(numpy.uint8)
    return faces, sums, box, witness, exposed, contact_ids, [int((contact_ids == i).sum()) for i in range(n)]


def running_faces(ids, n):
    """(faces, index_sums, box, witness, exposed) the second way: up every line of an axis, sample after sample, and at each
    step the lines on which the id changes: a run ends there (into another part: a face; into nothing: an exposed face of the
    upper side) and one begins (out of nothing: an exposed face of the lower side)."""
    faces = numpy.zeros((3, n, n), dtype=numpy.uint64)
    sums = numpy.zeros((3, n, n, 3), dtype=numpy.uint64)
    lo = numpy.full((3, n, n, 3), numpy.iinfo(numpy.int64).max, dtype=numpy.int64)
    hi = numpy.full((3, n, n, 3), -1, dtype=numpy.int64)
    key = numpy.full((3, n, n), numpy.iinfo(numpy.int64).max, dtype=numpy.int64)
    exposed = numpy.zeros((3, 2, n), dtype=numpy.uint64)
    for axis in range(3):
        lines = numpy.moveaxis(ids, axis, 0)
        others = [a for a in range(3) if a != axis]
        prev = numpy.full(lines.shape[1:], EMPTY, dtype=numpy.uint8)
        for t in range(lines.shape[0] + 1):
            now = lines[t] if t < lines.shape[0] else numpy.full(lines.shape[1:], EMPTY, dtype=numpy.uint8)
            ended, started = (now != prev) & (prev != EMPTY), (now != prev) & (now != EMPTY)
            numpy.add.at(exposed[axis, 0], prev[ended & (now == EMPTY)], 1)
            numpy.add.at(exposed[axis, 1], now[started & (prev == EMPTY)], 1)
            u, v = numpy.nonzero(ended & started)
            if len(u):
                p = numpy.zeros((len(u), 3), dtype=numpy.int64)
                p[:, axis], p[:, others[0]], p[:, others[1]] = t - 1, u, v
                i, j = prev[u, v], now[u, v]
                numpy.add.at(faces[axis], (i, j), 1)
                numpy.add.at(sums[axis], (i, j), p.astype(numpy.uint64))
                numpy.minimum.at(lo[axis], (i, j), p)
                numpy.maximum.at(hi[axis], (i, j), p)
                numpy.minimum.at(key[axis], (i, j), (p[:, 0] << 32) | (p[:, 1] << 16) | p[:, 2])
            prev = now
    empty = faces == 0
    box = numpy.where(empty[..., None, None], -1, numpy.stack([lo, hi], axis=-2)).astype(numpy.int32)
    fields = numpy.stack([(key >> 32) & 0xffff, (key >> 16) & 0xffff, key & 0xffff], axis=-1)
    return faces, sums, box, numpy.where(empty[..., None], -1, fields).astype(numpy.int32), exposed


def reference_of(ids, n):
    """The Reference over an id array."""
    faces, sums, box, witness, exposed, contact_ids, contact_counts = reference_faces(ids, n)
    found = comp.reference_components(contact_ids, SOLID)
    for a in (faces, sums, box, witness, exposed, contact_ids):
        a.setflags(write=False)
    return Reference(ids, [int((ids == k).sum()) for k in range(n)], faces, sums, box, witness, exposed, contact_ids, contact_counts,
                     found.components, found.labels)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _mine(name, frame, solids, by_hand, exposed=None, patches=None, groups=None, loose=None):
    return Scene(_scene(name, frame, solids, {}), by_hand, exposed or {}, patches, groups, loose)


def _scenes():
    out = {}
    # two boxes face to face, normal to each axis; along y the upper box comes first
    out["face_x"] = _mine("face_x", (8, 5, 6), [[((0, 0, 0), (4, 5, 6))], [((4, 0, 0), (8, 5, 6))]],
                          {(0, 0, 1): (30, ((3, 0, 0), (3, 4, 5)), (3, 0, 0))},
                          {(0, 0, 0): 0, (0, 1, 0): 30, (0, 0, 1): 30, (0, 1, 1): 0, (1, 0, 0): 24, (2, 1, 1): 20},
                          [(0, 1)], [[0, 1]], [])
    out["face_y"] = _mine("face_y", (5, 8, 6), [[((0, 4, 0), (5, 8, 6))], [((0, 0, 0), (5, 4, 6))]],
                          {(1, 1, 0): (30, ((0, 3, 0), (4, 3, 5)), (0, 3, 0))},
                          {(1, 0, 0): 30, (1, 1, 0): 0, (1, 0, 1): 0, (1, 1, 1): 30}, [(0, 1)], [[0, 1]], [])
    out["face_z"] = _mine("face_z", (5, 4, 8), [[((0, 0, 0), (5, 4, 4))], [((0, 0, 4), (5, 4, 8))]],
                          {(2, 0, 1): (20, ((0, 0, 3), (4, 3, 3)), (0, 0, 3))},
                          {(2, 0, 0): 0, (2, 1, 0): 20, (2, 0, 1): 20, (2, 1, 1): 0, (0, 0, 0): 16}, [(0, 1)], [[0, 1]], [])
    # interfaces normal to z at the word edges 63 | 64 and 127 | 128 and at nz - 2 | nz - 1, nz = 138 under pz = 144
    out["stack_z"] = _mine("stack_z", (3, 3, NZ), [[((0, 0, 0), (3, 3, 64))], [((0, 0, 64), (3, 3, 128))], [((0, 0, 128), (3, 3, NZ - 1))],
                                                  [((0, 0, NZ - 1), (3, 3, NZ))]],
                           {(2, 0, 1): (9, ((0, 0, 63), (2, 2, 63)), (0, 0, 63)), (2, 1, 2): (9, ((0, 0, 127), (2, 2, 127)), (0, 0, 127)),
                            (2, 2, 3): (9, ((0, 0, NZ - 2), (2, 2, NZ - 2)), (0, 0, NZ - 2))},
                           {(2, 0, 3): 9, (2, 1, 0): 9, (2, 0, 0): 0, (2, 1, 3): 0, (0, 0, 3): 3, (0, 0, 1): 3 * 64},
                           [(0, 1), (1, 2), (2, 3)], [[0, 1, 2, 3]], [])
    # part 1 reaches the border of the lattice on all six sides; part 0 is a core inside it (the lower index owns what both hold)
    out["border"] = _mine("border", (4, 4, 20), [[((1, 1, 5), (3, 3, 10))], [((0, 0, 0), (4, 4, 20))]],
                          {(0, 1, 0): (10, ((0, 1, 5), (0, 2, 9)), (0, 1, 5)), (0, 0, 1): (10, ((2, 1, 5), (2, 2, 9)), (2, 1, 5)),
                           (2, 1, 0): (4, ((1, 1, 4), (2, 2, 4)), (1, 1, 4)), (2, 0, 1): (4, ((1, 1, 9), (2, 2, 9)), (1, 1, 9))},
                          {(0, 0, 1): 80, (0, 1, 1): 80, (1, 0, 1): 80, (1, 1, 1): 80, (2, 0, 1): 16, (2, 1, 1): 16,
                           (0, 0, 0): 0, (0, 1, 0): 0, (1, 0, 0): 0, (1, 1, 0): 0, (2, 0, 0): 0, (2, 1, 0): 0}, [(0, 1)], [[0, 1]], [])
    # three parts that meet along the edge x = 3 | 4, y = 3 | 4: one patch with three parts
    out["three"] = _mine("three", (8, 8, 6), [[((0, 0, 0), (4, 8, 6))], [((4, 0, 0), (8, 4, 6))], [((4, 4, 0), (8, 8, 6))]],
                         {(0, 0, 1): (24, ((3, 0, 0), (3, 3, 5)), (3, 0, 0)), (0, 0, 2): (24, ((3, 4, 0), (3, 7, 5)), (3, 4, 0)),
                          (1, 1, 2): (24, ((4, 3, 0), (7, 3, 5)), (4, 3, 0))}, {}, [(0, 1, 2)], [[0, 1, 2]], [])
    # one pair, two patches: part 1 is two feet on a slab, six samples apart
    out["two_patches"] = _mine("two_patches", (4, 10, 5), [[((0, 0, 0), (2, 10, 5))], [((2, 0, 0), (4, 3, 5)), ((2, 7, 0), (4, 10, 5))]],
                               {(0, 0, 1): (30, ((1, 0, 0), (1, 9, 4)), (1, 0, 0))}, {(0, 0, 0): 20}, [(0, 1), (0, 1)], [[0, 1]], [])
    # two parts in contact and a third that hangs in the air, two samples off
    out["loose"] = _mine("loose", (10, 4, 5), [[((0, 0, 0), (3, 4, 5))], [((3, 0, 0), (6, 4, 5))], [((8, 0, 0), (10, 4, 5))]],
                         {(0, 0, 1): (20, ((2, 0, 0), (2, 3, 4)), (2, 0, 0))}, {(0, 0, 1): 20, (0, 1, 2): 20, (0, 0, 2): 20},
                         [(0, 1)], [[0, 1], [2]], [2])
    return out


MINE = _scenes()
SCENES = {name: Scene(dis_scenes.SCENES[name], {}, {}, None, None, None) for name in dis_scenes.SMALL}
SCENES.update(MINE)
NAMES = list(SCENES)
FROM_DISASSEMBLY = list(dis_scenes.SMALL)
assert len(NAMES) == len(FROM_DISASSEMBLY) + len(MINE)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scene."""
    if name in dis_scenes.SCENES:
        return dis_scenes.scene(name)
    asm = SCENES[name].scene.build()
    instances = dis_scenes._instance_cells.visible(asm, dis_scenes.STEP)
    corner, step, dims = dis_scenes._instance_cells.checked_lattice(instances, dis_scenes.STEP)
    return asm, dis_scenes.STEP, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def part_ids(name):
    """The dense part ids of a scene, every instance evaluated at every sample, once."""
    if name in dis_scenes.SCENES:
        return dis_scenes.part_ids(name)
    asm, resolution, instances, corner, step, dims = scene(name)
    ids, counts = dis_scenes.voxels.dense_ids([w < 0 for w in dis_scenes.mass.dense_fields(instances, corner, step, dims)])
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def reference(name):
    """The Reference of a scene, computed once and shared; nobody changes it."""
    return reference_of(part_ids(name), len(scene(name)[2]))


# ---- raw id volumes, for the kernel alone -------------------------------------------------------------------------------

# EVERY_PAIR: line (x, y) holds, in each of its halves z in [0, 64) and [64, 128), the zigzag path 0, 1, -1, 2, -2, ..., 32 through
# all 64 ids, shifted by _SHIFTS[x][y][half] mod 64.  The 32 paths with shifts 0..31 hold every unordered pair once as
# neighbours; the shifts below were searched once so that every unordered pair also occurs across x and across y.  The ids
# are then renamed by a seeded permutation and the last two samples of a line are random ids or 255.  (The ordered pairs,
# 64 * 63 = 4032, outnumber the 4 * 7 * 130 = 3640 faces of x: unordered it is.)
_ZIGZAG = [0] + [(t + 1) // 2 if t % 2 else -(t // 2) for t in range(1, 64)]
_SHIFTS = [[[30, 32], [48, 60], [42, 50], [52, 60], [15, 19], [38, 24], [17, 48]], [[41, 32], [35, 35], [5, 34], [55, 4], [51, 34], [52, 21], [28, 50]],
           [[54, 16], [7, 29], [62, 8], [24, 32], [57, 13], [32, 16], [1, 52]], [[24, 17], [31, 25], [7, 37], [47, 61], [5, 46], [18, 12], [2, 56]],
           [[43, 10], [13, 63], [26, 41], [18, 7], [27, 39], [29, 12], [34, 9]]]
RAW_SHAPE = (5, 7, 130)


def _every_pair():
    rng = numpy.random.default_rng(20)
    t = numpy.arange(128)
    ids = (numpy.array(_ZIGZAG)[t % 64][None, None, :] + numpy.array(_SHIFTS)[:, :, t // 64]) % 64
    ids = rng.permutation(64)[ids]
    tail = rng.choice(numpy.array(list(range(64)) + [EMPTY] * 16), size=RAW_SHAPE[:2] + (2,))
    return numpy.concatenate([ids, tail], axis=2).astype(numpy.uint8)


def _random():
    """Ids drawn from {0..63, 255}, 255 a quarter of the time: exposed faces and interface samples everywhere."""
    rng = numpy.random.default_rng(21)
    return rng.choice(numpy.array(list(range(64)) + [EMPTY] * 21), size=RAW_SHAPE).astype(numpy.uint8)


def _few(shape, seed):
    rng = numpy.random.default_rng(seed)
    return rng.choice(numpy.array([0, 1, 2, EMPTY]), size=shape).astype(numpy.uint8)


RAW = {
    "every_pair": _every_pair,
    "random": _random,
    "one_sample": lambda: numpy.zeros((1, 1, 1), dtype=numpy.uint8),
    "one_line_65": lambda: _few((1, 1, 65), 22),                # a word and one sample: lane 63 fetches across the edge
    "3x1x16": lambda: _few((3, 1, 16), 23),                     # no padding at all
    "1x3x17": lambda: _few((1, 3, 17), 24),
    "one_id": lambda: numpy.full((4, 3, 70), 7, dtype=numpy.uint8),
}
RAW_NAMES = list(RAW)
RAW_PARTS = 64


@functools.lru_cache(maxsize=None)
def raw_ids(name):
    ids = numpy.ascontiguousarray(RAW[name]())
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def raw_reference(name):
    return reference_of(raw_ids(name), RAW_PARTS)


def unordered_pairs(faces):
    """bool[3, n, n]: the pairs with a face in either order, per axis."""
    return (faces > 0) | (numpy.swapaxes(faces, 1, 2) > 0)
