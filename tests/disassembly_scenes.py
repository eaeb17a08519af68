"""The scenarios and the CPU reference of the disassembly tests (test_disassembly_host.py proves on the CPU that each scenario
holds the entries it is there for; test_gpu_disassembly.py runs them on the device).

`reference_blocking(ids, n)` is written from the definition in codecad_amd/disassembly.py alone: for each axis and ordered
pair, t = 1, 2, ... and the first t with any(M_i[..., :-t] & M_j[..., t:]) (the slices taken along the axis) is D; the witness
is the lexicographically first p of that intersection.  Two things shorten the search and change nothing: only the lines that
hold both parts are kept, and t starts at (the least index of j) - (the greatest index of i) on them, below which no q - p lies.
`running_blocking` is the second way: a walk up every line with a running last index per part, evaluated where a run starts.
`reference_order` restates the ORDER rule in plain Python over the matrices.

The scenarios are boxes on the lattice in SAMPLE units at step 1/16, in the manner of overhangs_scenes._solid.  Unless stated a
scene is NZ = 138 samples high: a column spans three 64-sample words and a ragged tail of ten under pz = 144.
"""
import collections
import functools

import numpy

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_mass_scenes as mass
import assembly_voxels_scenes as voxels
import overhangs_scenes
from overhangs_scenes import _solid, NZ
from assembly_components_scenes import STEP, EMPTY

NEVER = 0xffffffff
DIRECTIONS = [(axis, up) for axis in range(3) for up in (True, False)]              # +x, -x, +y, -y, +z, -z

Reference = collections.namedtuple("Reference", "ids counts distance witness")
# `frame`: the lattice the parts span; `by_hand`: {(axis, i, j): (D, witness)} written by hand; `never`: [(axis, i, j)] that must be
# NEVER; `order`: what order() must return, or None where the scene is not about it
Scene = collections.namedtuple("Scene", "build frame by_hand never order")


# ---- the reference ----------------------------------------------------------------------------------------------------

def _along(axis, sl):
    out = [slice(None)] * 3
    out[axis] = sl
    return tuple(out)


def reference_blocking(ids, n):
    """(distance uint32[3, n, n], witness int32[3, n, n, 3]) from the definition."""
    distance = numpy.full((3, n, n), NEVER, dtype=numpy.uint32)
    witness = numpy.full((3, n, n, 3), -1, dtype=numpy.int32)
    masks = [ids == k for k in range(n)]
    for axis in range(3):
        others = tuple(a for a in range(3) if a != axis)
        on_line = [m.any(axis=axis, keepdims=True) for m in masks]
        for i in range(n):
            for j in range(n):
                both = on_line[i] & on_line[j]
                if i == j or not both.any():
                    continue
                mi, mj = masks[i] & both, masks[j] & both                           # the lines that hold both
                at_i, at_j = numpy.flatnonzero(mi.any(axis=others)), numpy.flatnonzero(mj.any(axis=others))
                for t in range(max(1, int(at_j.min()) - int(at_i.max())), int(at_j.max()) - int(at_i.min()) + 1):
                    meet = mi[_along(axis, slice(None, -t))] & mj[_along(axis, slice(t, None))]
                    if meet.any():
                        distance[axis, i, j] = t
                        witness[axis, i, j] = numpy.argwhere(meet)[0]               # C order: the lexicographically first
                        break
    return distance, witness


def running_blocking(ids, n):
    """The same the second way: up every line of an axis at once, the last index of every part whose run has ended, and at
    every run start the key (D, x, y, z) against every part seen so far; the least key per pair."""
    ones = numpy.uint64(0xffffffffffffffff)
    keys = numpy.full((3, n, n), ones, dtype=numpy.uint64)
    for axis in range(3):
        lines = numpy.moveaxis(ids, axis, 0)
        others = [a for a in range(3) if a != axis]
        last = numpy.full((n,) + lines.shape[1:], -1, dtype=numpy.int64)
        prev = numpy.full(lines.shape[1:], EMPTY, dtype=numpy.uint8)
        for t in range(lines.shape[0]):
            now = lines[t]
            changed = now != prev
            if not changed.any():
                continue
            ended = changed & (prev != EMPTY)
            u, v = numpy.nonzero(ended)
            last[prev[u, v], u, v] = t - 1
            started = changed & (now != EMPTY)
            for i in range(n):
                u, v = numpy.nonzero(started & (last[i] >= 0) & (now != i))
                if len(u) == 0:
                    continue
                p = numpy.zeros((3, len(u)), dtype=numpy.uint64)
                p[axis], p[others[0]], p[others[1]] = last[i, u, v], u, v
                key = (numpy.uint64(t) - p[axis]) << numpy.uint64(48) | p[0] << numpy.uint64(32) | p[1] << numpy.uint64(16) | p[2]
                numpy.minimum.at(keys[axis, i], now[u, v], key)
            prev = now
    never = keys == ones
    field = lambda s: ((keys >> numpy.uint64(s)) & numpy.uint64(0xffff)).astype(numpy.int64)     # noqa: E731
    return (numpy.where(never, NEVER, field(48)).astype(numpy.uint32),
            numpy.where(never[..., None], -1, numpy.stack([field(32), field(16), field(0)], axis=-1)).astype(numpy.int32))


def reference_steps(distance, i, j, axis, up):
    return int(distance[axis, i, j] if up else distance[axis, j, i])


def reference_order(distance):
    """([(k, axis, up)], stuck) by the ORDER rule, over the matrices alone."""
    rest, sequence = list(range(distance.shape[1])), []
    progress = True
    while rest and progress:
        progress = False
        for k in rest:
            free = [(axis, up) for axis, up in DIRECTIONS if all(reference_steps(distance, k, j, axis, up) == NEVER for j in rest if j != k)]
            if free:
                sequence.append((k,) + free[0])
                rest.remove(k)
                progress = True
                break
    return sequence, rest


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _parts(name, frame, solids):
    """An assembly of one part per list of boxes [lo, hi) of `frame`."""
    return cc.assembly(name, [_solid(frame, boxes).make_part("%s%d" % (name, k)) for k, boxes in enumerate(solids)])


def _scene(name, frame, solids, by_hand, never=(), order=None):
    return Scene(functools.partial(_parts, name, frame, solids), frame, by_hand, list(never), order)


def _column(x, z0, z1):
    """Samples z in [z0, z1) of the two lines (x, 0) and (x, 1)."""
    return [((x, 0, z0), (x + 1, 2, z1))]


def _words():
    """Axis 2, one case a column x, each with parts of its own, so that no case hides behind another's minimum:
      x = 0: a run that ends at z = 63 and another part's that starts at 64 (a start at lane 0 whose predecessor has another owner);
      x = 1: the same at 127 | 128;
      x = 2: a run [60, 70) across the word edge between a run below and a run above: it starts once and ends once;
      x = 3: a run [63, 65), one sample either side of the edge: lane 0 starts nothing, its predecessor has the same owner;
      x = 4: a run that starts at 64 over an empty sample 63;
      x = 5: a part whose last sample, z = 4, lies two words below the other's first, z = 130, an all-empty word between;
      x = 6: a pair whose only q, z = 136, lies in the ragged last word."""
    frame = (7, 2, NZ)
    solids = [_column(0, 50, 64), _column(0, 64, 70),                               # 0, 1
              _column(1, 120, 128), _column(1, 128, 132),                           # 2, 3
              _column(2, 10, 20), _column(2, 60, 70), _column(2, 80, 90),           # 4, 5, 6
              _column(3, 0, 5), _column(3, 63, 65), _column(3, 100, 101),           # 7, 8, 9
              _column(4, 0, 5), _column(4, 64, 70),                                 # 10, 11
              _column(5, 0, 5), _column(5, 130, 135),                               # 12, 13
              _column(6, 128, 130), _column(6, 136, NZ)]                            # 14, 15
    by_hand = {(2, 0, 1): (1, (0, 0, 63)), (2, 2, 3): (1, (1, 0, 127)),
               (2, 4, 5): (41, (2, 0, 19)), (2, 5, 6): (11, (2, 0, 69)), (2, 4, 6): (61, (2, 0, 19)),
               (2, 7, 8): (59, (3, 0, 4)), (2, 8, 9): (36, (3, 0, 64)), (2, 7, 9): (96, (3, 0, 4)),
               (2, 10, 11): (60, (4, 0, 4)), (2, 12, 13): (126, (5, 0, 4)), (2, 14, 15): (7, (6, 0, 129))}
    never = [(2, j, i) for (_, i, j) in by_hand] + [(2, 0, 3), (2, 5, 8)]
    return _scene("words", frame, solids, by_hand, never)


def _slabs(axis):
    """64 parts, slab k the samples 2 k and 2 k + 1 of `axis` over a cross-section of 4 x 4: a line of 128 samples."""
    frame = tuple(128 if a == axis else 4 for a in range(3))
    at = lambda k: tuple(k if a == axis else 0 for a in range(3))                  # noqa: E731
    solids = [[(at(2 * k), tuple(2 * k + 2 if a == axis else 4 for a in range(3)))] for k in range(64)]
    by_hand = {(axis, i, j): (2 * (j - i) - 1, at(2 * i + 1)) for i in range(64) for j in range(i + 1, 64)}
    never = [(a, i, j) for a in range(3) for i in range(64) for j in range(64) if a != axis or j <= i]
    order = ([(k, 0, axis != 0) for k in range(63)] + [(63, 0, True)], [])          # along x: downwards; along z: +x is free
    return _scene("slabs64_" + "xyz"[axis], frame, solids, by_hand, never, order)


def _long(axis):
    """Three small boxes on a lattice 4 wide and 40 010 long: part 0 at its foot, parts 1 and 2 beyond 40 000."""
    n = 40010
    frame = tuple(n if a == axis else 4 for a in range(3))
    span = lambda lo, hi: [(tuple(lo if a == axis else 0 for a in range(3)), tuple(hi if a == axis else 4 for a in range(3)))]   # noqa: E731
    at = lambda k: tuple(k if a == axis else 0 for a in range(3))                  # noqa: E731
    solids = [span(0, 5), span(40000, 40004), span(40006, n)]
    by_hand = {(axis, 0, 1): (39996, at(4)), (axis, 0, 2): (40002, at(4)), (axis, 1, 2): (3, at(40003))}
    never = [(axis, 1, 0), (axis, 2, 0), (axis, 2, 1)] + [(a, i, j) for a in range(3) if a != axis for i in range(3) for j in range(3)]
    return _scene("long_" + "xyz"[axis], frame, solids, by_hand, never, ([(0, 0, axis != 0), (1, 0, axis != 0), (2, 0, True)], []))


def _ball():
    """overhangs_scenes' ball over a slab under three owners: 0 a cap that owns the ball's lowest samples, 1 the ball (and a
    pad on the plate), 2 the slab.  Overlap samples count for the lower index: the cap, not the ball, faces the slab."""
    radius, (cx, cy, cz) = overhangs_scenes.BALL_RADIUS, overhangs_scenes.BALL_CENTRE
    by_hand = {(2, 2, 0): (114 - 15, (10, 10, 15)),                                 # the slab's top layer under the cap's foot
               (2, 0, 1): (1, (10, 10, 117)),                                       # the ball right above the cap
               (2, 1, 2): (10 - 1, (0, 0, 1))}                                      # the ball's pad on the plate, under the slab
    assert cz - radius > 114                                                        # the ball's lowest sample is the cap's
    return Scene(overhangs_scenes._ball, overhangs_scenes.BALL, by_hand, [(2, 0, 2)], None)


HOOK_Z = 56                                                                         # the links cross the word edge 63 | 64


def _hooks():
    """Two links of a chain, each a square ring of bars 2 samples thick: part 0 in the plane y in [4, 6), part 1 in the plane
    x in [4, 6), each with a bar through the other's hole -- on every axis some line meets 0, 1, 0 and another 1, 0, 1 --, and a
    loose pillar, part 2, beside them."""
    frame, z = (14, 10, NZ), HOOK_Z
    ring0 = [((0, 4, z), (10, 6, z + 2)), ((0, 4, z + 8), (10, 6, z + 10)), ((0, 4, z), (2, 6, z + 10)), ((8, 4, z), (10, 6, z + 10))]
    ring1 = [((4, 0, z + 4), (6, 10, z + 6)), ((4, 0, z + 12), (6, 10, z + 14)), ((4, 0, z + 4), (6, 2, z + 14)), ((4, 8, z + 4), (6, 10, z + 14))]
    pillar = [((12, 0, 0), (14, 2, NZ))]
    by_hand = {(0, 0, 1): (3, (1, 4, z + 4)), (0, 1, 0): (3, (5, 4, z + 4)), (1, 1, 0): (3, (4, 1, z + 8)), (1, 0, 1): (3, (4, 5, z + 8)),
               (2, 0, 1): (3, (4, 4, z + 1)), (2, 1, 0): (3, (4, 4, z + 5)), (0, 1, 2): (7, (5, 0, z + 4))}
    never = [(a, 2, k) for a in range(3) for k in (0, 1)] + [(0, 0, 2), (1, 0, 2), (1, 1, 2), (2, 0, 2), (2, 1, 2)]
    return _scene("hooks", frame, [ring0, ring1, pillar], by_hand, never, ([(2, 0, True)], [0, 1]))


def _scenes():
    out = {}
    # two boxes apart along one axis and on no common line of the other two
    out["apart_x"] = _scene("apart_x", (12, 5, NZ), [[((0, 0, 0), (3, 3, NZ))], [((8, 2, 60), (12, 5, 70))]],
                            {(0, 0, 1): (6, (2, 2, 60))}, [(0, 1, 0), (1, 0, 1), (1, 1, 0), (2, 0, 1), (2, 1, 0)],
                            ([(0, 0, False), (1, 0, True)], []))
    out["apart_y"] = _scene("apart_y", (5, 12, NZ), [[((2, 8, 60), (5, 12, 70))], [((0, 0, 0), (3, 3, NZ))]],      # the upper one first
                            {(1, 1, 0): (6, (2, 2, 60))}, [(1, 0, 1), (0, 0, 1), (0, 1, 0), (2, 0, 1), (2, 1, 0)],
                            ([(0, 0, True), (1, 0, True)], []))
    out["apart_z"] = _scene("apart_z", (5, 5, NZ), [[((0, 0, 0), (3, 3, 40))], [((2, 2, 100), (5, 5, NZ))]],
                            {(2, 0, 1): (61, (2, 2, 39))}, [(2, 1, 0), (0, 0, 1), (0, 1, 0), (1, 0, 1), (1, 1, 0)],
                            ([(0, 0, True), (1, 0, True)], []))
    # a peg, part 0, in a blind hole of a block (the peg owns what both contain): free upwards, in contact sideways and downwards
    out["peg"] = _scene("peg", (16, 16, NZ), [[((6, 6, 40), (10, 10, NZ))], [((0, 0, 0), (16, 16, NZ))]],
                        {(2, 1, 0): (1, (6, 6, 39)), (0, 0, 1): (1, (9, 6, 40)), (0, 1, 0): (1, (5, 6, 40)),
                         (1, 0, 1): (1, (6, 9, 40)), (1, 1, 0): (1, (6, 5, 40))}, [(2, 0, 1)], ([(0, 2, True), (1, 0, True)], []))
    # i, k, j on one line: D[i][j] counts across k
    out["between_x"] = _scene("between_x", (16, 4, NZ), [[((0, 0, 0), (3, 4, NZ))], [((5, 0, 0), (8, 4, NZ))], [((12, 0, 0), (16, 4, NZ))]],
                              {(0, 0, 1): (3, (2, 0, 0)), (0, 1, 2): (5, (7, 0, 0)), (0, 0, 2): (10, (2, 0, 0))},
                              [(0, 1, 0), (0, 2, 0), (0, 2, 1)], ([(0, 0, False), (1, 0, False), (2, 0, True)], []))
    out["between_z"] = _scene("between_z", (4, 4, NZ), [[((0, 0, 0), (4, 4, 10))], [((0, 0, 60), (4, 4, 70))], [((0, 0, 130), (4, 4, NZ))]],
                              {(2, 0, 1): (51, (0, 0, 9)), (2, 1, 2): (61, (0, 0, 69)), (2, 0, 2): (121, (0, 0, 9))},
                              [(2, 1, 0), (2, 2, 0), (2, 2, 1)], ([(0, 0, True), (1, 0, True), (2, 0, True)], []))
    # i, gap, i, j on the lines y < 2 (x < 2) and j, i, j on the others: the later sample of i counts, both ways finite
    out["again_x"] = _scene("again_x", (12, 4, NZ), [[((0, 0, 0), (2, 2, NZ)), ((5, 0, 0), (7, 4, NZ))], [((9, 0, 0), (12, 4, NZ)), ((0, 2, 0), (2, 4, NZ))]],
                            {(0, 0, 1): (3, (6, 0, 0)), (0, 1, 0): (4, (1, 2, 0))}, [])
    out["again_z"] = _scene("again_z", (4, 4, NZ), [[((0, 0, 0), (2, 4, 20)), ((0, 0, 50), (4, 4, 70))], [((0, 0, 100), (4, 4, NZ)), ((2, 0, 0), (4, 4, 10))]],
                            {(2, 0, 1): (31, (0, 0, 69)), (2, 1, 0): (41, (2, 0, 9))}, [])
    out["words"] = _words()
    out["slabs64_x"], out["slabs64_z"] = _slabs(0), _slabs(2)
    out["ownership"] = _ball()
    out["hooks"] = _hooks()
    out["long_x"], out["long_z"] = _long(0), _long(2)
    out["single"] = _scene("single", (5, 5, NZ), [[((0, 0, 0), (5, 5, NZ))]], {}, [(a, 0, 0) for a in range(3)], ([(0, 0, True)], []))
    return out


SCENES = _scenes()
NAMES = list(SCENES)
SMALL = [name for name in NAMES if not name.startswith("long_")]


def empty_assembly():
    return cc.assembly("nothing", [shapes.box(1).make_part("ghost").hidden()])


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scene."""
    asm = SCENES[name].build()
    instances = _instance_cells.visible(asm, STEP)
    corner, step, dims = _instance_cells.checked_lattice(instances, STEP)
    return asm, STEP, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def part_ids(name):
    """The dense part ids of a scene, every instance evaluated at every sample (assembly_voxels_scenes.dense_ids), once."""
    asm, resolution, instances, corner, step, dims = scene(name)
    ids, counts = voxels.dense_ids([w < 0 for w in mass.dense_fields(instances, corner, step, dims)])
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def reference(name):
    """The Reference of a scene, computed once and shared; nobody changes it."""
    ids = part_ids(name)
    n = len(scene(name)[2])
    distance, witness = reference_blocking(ids, n)
    for a in (distance, witness):
        a.setflags(write=False)
    return Reference(ids, [int((ids == k).sum()) for k in range(n)], distance, witness)
