"""The scenarios and the CPU reference of the component tests (test_assembly_components_host.py proves on the CPU that each
scenario holds the edge it is there for; test_gpu_assembly_components.py runs them on the device).

`reference_components(ids, of)` is written from the definitions in codecad_amd/assembly_components.py.  It starts from the
part ids of assembly_voxels_scenes.reference_voxels (the dense definition), labels S by ONE algorithm -- a flood fill seeded
in ascending linear index, so a component's label is its seed -- and derives every Component field per label with plain
array operations on the mask `labels == label`.

The new scenarios are boxes with faces on multiples of the dyadic step 1/16 and samples half-way between them, given in
SAMPLE units: `_cut(n, [(lo, hi), ...])` is a block of n samples with the listed boxes [lo, hi) taken out.
"""
import collections
import functools

import numpy

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_mass_scenes as mass
import assembly_voxels_scenes as voxels

components = __import__("sys").modules["codecad_amd.assembly_components"]
EMPTY_SPACE, SOLID, NONE, TILE = components.EMPTY_SPACE, components.SOLID, components.NONE, components.TILE
EMPTY = 255
STEP = 0.0625

Reference = collections.namedtuple("Reference", "ids labels components")
Expected = collections.namedtuple("Expected", "label count box index_sums touches_border parts")
Scene = collections.namedtuple("Scene", "build resolution side ofs")


# ---- the reference ----------------------------------------------------------------------------------------------------

def neighbours(flat, shape):
    """The flat indices of the in-lattice 6-neighbours of the samples `flat` (with repetitions)."""
    at = numpy.stack(numpy.unravel_index(flat, shape), axis=-1)
    out = []
    for axis in range(3):
        for d in (-1, 1):
            moved = at.copy()
            moved[:, axis] += d
            ok = (moved[:, axis] >= 0) & (moved[:, axis] < shape[axis])
            out.append(numpy.ravel_multi_index(tuple(moved[ok].T), shape))
    return numpy.concatenate(out) if out else flat[:0]


def flood_labels(in_set):
    """uint32 labels of bool[nx, ny, nz] `in_set`: seeds in ascending linear index, each filled by its frontier."""
    shape = in_set.shape
    labels = numpy.full(in_set.size, NONE, dtype=numpy.uint32)
    todo = in_set.ravel().copy()
    for seed in numpy.flatnonzero(todo):
        if not todo[seed]:
            continue
        frontier = numpy.array([seed])
        todo[seed] = False
        while len(frontier):
            labels[frontier] = seed
            near = numpy.unique(neighbours(frontier, shape))
            frontier = near[todo[near]]
            todo[frontier] = False
    return labels.reshape(shape)


def propagated_labels(in_set):
    """The same labels by a second way: every sample of S takes the least index among itself and its 6-neighbours of S,
    again and again, until nothing changes."""
    big = numpy.iinfo(numpy.int64).max
    labels = numpy.where(in_set, numpy.arange(in_set.size, dtype=numpy.int64).reshape(in_set.shape), big)
    while True:
        least = labels.copy()
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            least[lo] = numpy.minimum(least[lo], labels[hi])
            least[hi] = numpy.minimum(least[hi], labels[lo])
        least = numpy.where(in_set, least, big)
        if numpy.array_equal(least, labels):
            return numpy.where(in_set, labels, NONE).astype(numpy.uint32)
        labels = least


def reference_components(ids, of):
    in_set = (ids == EMPTY) if of == EMPTY_SPACE else (ids != EMPTY)
    labels = flood_labels(in_set)
    shape = ids.shape
    out = []
    for label in numpy.unique(labels[in_set]).tolist():
        mask = labels == label
        at = numpy.argwhere(mask)
        lo, hi = tuple(int(v) for v in at.min(axis=0)), tuple(int(v) for v in at.max(axis=0))
        border = bool(((at == 0) | (at == numpy.array(shape) - 1)).any())
        if of == SOLID:
            owners = ids[mask]
        else:
            owners = ids.ravel()[neighbours(numpy.flatnonzero(mask.ravel()), shape)]
        parts = tuple(sorted(set(owners[owners != EMPTY].tolist())))
        out.append(Expected(label, int(mask.sum()), (lo, hi), tuple(int(v) for v in at.sum(axis=0)), border, parts))
    labels.setflags(write=False)
    return Reference(ids, labels, out)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _box(n, lo, hi):
    """The box of the samples [lo, hi) of a block of `n` samples centred at the origin."""
    size = [(b - a) * STEP for a, b in zip(lo, hi)]
    centre = [((a + b) / 2 - m / 2) * STEP for a, b, m in zip(lo, hi, n)]
    return shapes.box(*size).translated(*centre)


def _cut(n, holes):
    return _box(n, (0, 0, 0), n) - shapes.union([_box(n, lo, hi) for lo, hi in holes])


SHELL_SAMPLES = 36


def _shell():
    """A hollow ball, 36 samples across: three tiles or more on every axis, no dimension a multiple of the tile's."""
    r = SHELL_SAMPLES * STEP / 2
    return cc.assembly("shell", [(shapes.sphere(r=r) - shapes.sphere(r=0.7)).make_part("shell")])


CUP = (16, 16, 8)


def _cup(flip):
    pocket = ((4, 4, 0), (12, 12, 4)) if flip else ((4, 4, 4), (12, 12, 8))
    return _cut(CUP, [pocket]).make_part("upper" if flip else "lower").translated_z((0.25 if flip else -0.25))


def _two_cups(hide=False):
    """Two cups mouth to mouth: an 8 x 8 x 8 void that only both together enclose."""
    upper = _cup(True)
    return cc.assembly("cups", [_cup(False), upper.hidden() if hide else upper])


SERPENTINE = (36, 12, 44)
RUNS = 7


def serpentine_holes(opened=False):
    """Seven runs along z, 2 x 2 samples wide, 4 samples apart in x, joined at alternating ends: six turns.  The least
    linear index is the free end of run 0."""
    holes = [((4 + 4 * k, 5, 4), (6 + 4 * k, 7, 40)) for k in range(RUNS)]
    holes += [((4 + 4 * k, 5, 4 if k % 2 else 38), (10 + 4 * k, 7, 6 if k % 2 else 40)) for k in range(RUNS - 1)]
    if opened:
        holes.append(((28, 5, 38), (30, 7, 44)))
    return holes


def _serpentine(opened=False):
    return cc.assembly("serpentine", [_cut(SERPENTINE, serpentine_holes(opened)).make_part("block")])


DIAGONAL = (20, 20, 20)
DIAGONAL_VOIDS = [((4, 4, 4), (8, 8, 8)), ((8, 8, 4), (12, 12, 8)),               # share the edge x = y = 8 only
                  ((12, 2, 12), (16, 6, 16)), ((16, 6, 16), (19, 10, 19))]         # share the corner (16, 6, 16) only


def _diagonal():
    return cc.assembly("diagonal", [_cut(DIAGONAL, DIAGONAL_VOIDS).make_part("block")])


def _diagonal_solid():
    """Two blocks of 8^3 samples that touch along one edge only."""
    n = (16, 16, 8)
    return cc.assembly("edge", [_box(n, (0, 0, 0), (8, 8, 8)).make_part("a"), _box(n, (8, 8, 0), (16, 16, 8)).make_part("b")])


BUBBLES = (47, 47, 47)
BUBBLE_AT = [7 + 8 * i for i in range(5)]                  # 2 samples each: they straddle every x and y face, z = 15|16, 31|32


def _bubbles():
    holes = [((x, y, z), (x + 2, y + 2, z + 2)) for x in BUBBLE_AT for y in BUBBLE_AT for z in BUBBLE_AT]
    return cc.assembly("bubbles", [_cut(BUBBLES, holes).make_part("block")])


BOTH = (EMPTY_SPACE, SOLID)
SCENES = {
    "shell": Scene(_shell, STEP, None, BOTH),
    "two_cups": Scene(_two_cups, STEP, None, BOTH),
    "one_cup": Scene(functools.partial(_two_cups, True), STEP, None, (EMPTY_SPACE,)),
    "serpentine": Scene(_serpentine, STEP, None, (EMPTY_SPACE,)),
    "serpentine_open": Scene(functools.partial(_serpentine, True), STEP, None, (EMPTY_SPACE,)),
    "diagonal": Scene(_diagonal, STEP, None, (EMPTY_SPACE,)),
    "diagonal_solid": Scene(_diagonal_solid, STEP, None, (SOLID,)),
    "bubbles": Scene(_bubbles, STEP, None, (EMPTY_SPACE,)),
}
MASS_SCENES = {"rims": BOTH, "coarse_64": (SOLID,), "solids64": (SOLID,), "heavy_pair25": (EMPTY_SPACE,)}
for _name, _ofs in MASS_SCENES.items():
    SCENES[_name] = Scene(mass.SCENES[_name].build, mass.SCENES[_name].resolution, mass.SCENES[_name].side, _ofs)
CASES = [(name, of) for name in sorted(SCENES) for of in SCENES[name].ofs]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scenario."""
    if name in MASS_SCENES:
        return mass.scene(name)
    sc = SCENES[name]
    asm = sc.build()
    instances = _instance_cells.visible(asm, sc.resolution)
    corner, step, dims = _instance_cells.checked_lattice(instances, sc.resolution)
    return asm, sc.resolution, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def part_ids(name):
    """The dense part ids of a scenario: assembly_voxels_scenes.reference_voxels', computed once."""
    if name in MASS_SCENES:
        return voxels.reference(name).ids
    asm, resolution, instances, corner, step, dims = scene(name)
    ids = voxels.reference_voxels(instances, corner, step, dims, True).ids
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def reference(name, of=EMPTY_SPACE):
    """The Reference of a scenario, computed once and shared; nobody changes it."""
    return reference_components(part_ids(name), of)


def face_pairs(mask, tile=TILE):
    """How many 6-adjacent pairs of samples of `mask` lie across a face between two tiles."""
    total = 0
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(tile[axis] - 1, -1, tile[axis]), slice(tile[axis], None, tile[axis])
        total += int((mask[tuple(lo)] & mask[tuple(hi)]).sum())
    return total
