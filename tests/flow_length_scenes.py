"""The references and the scenarios of the flow-length tests (test_flow_length_host.py proves on the CPU that the two references
agree and that each scenario holds what it is there for; test_gpu_geodesic_raw.py runs the entry points of
csrc/instance_geodesic.hip alone on raw volumes, test_gpu_flow_length.py the scenarios through flow_length() on the device).

`reference_steps(s, seeds)` is REFERENCE A, from the definition: the reached set grown by shifted arrays, frontier by frontier;
the frontier that is k steps from the seeds reads k.
`reference_rounds(s, seeds)` is REFERENCE B, the device's way emulated in NumPy: rounds of `sweep` along z, then y, then x, each
a forward and then a backward walk of every whole line with a carry, until a round lowers nothing -> the field after every
round, and how many rounds ran (the last, which changed nothing, included).
`stats` restates the per-part fields with plain array operations; `raw_stats` what hu_geodesic_stats leaves in its buffers.

The scenarios are boxes in SAMPLE units at step 1/16, built like those of assembly_components_scenes."""
import collections
import functools

import numpy

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_components_scenes as comp
import assembly_voxels_scenes as voxels
import raw_volume_scenes as raw
from assembly_components_scenes import SOLID, EMPTY_SPACE, EMPTY, STEP

fl = __import__("sys").modules["codecad_amd.flow_length"]
NONE = 0xffffffff
SLOTS = 65
VOID_CODE = 254                 # include/hip_util.h HU_GEODESIC_EMPTY
MODE_BORDER, MODE_LAYER, MODE_LIST = 0, 1, 2

Stats = collections.namedtuple("Stats", "reached_counts unreached_counts sum_steps farthest")
Case = collections.namedtuple("Case", "name scene of source")


# ---- the references ---------------------------------------------------------------------------------------------------

def in_set_of(ids, of):
    if of == SOLID:
        return ids != EMPTY
    return ids == (EMPTY if of == EMPTY_SPACE else of)


def code(of):
    return VOID_CODE if of == EMPTY_SPACE else raw.code(of)


def shifted(mask, axis, by):
    """`mask` moved by `by` (+1 or -1) along `axis`, False moving in."""
    out = numpy.zeros_like(mask)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[axis], dst[axis] = (slice(None, -1), slice(1, None)) if by > 0 else (slice(1, None), slice(None, -1))
    out[tuple(dst)] = mask[tuple(src)]
    return out


def reference_steps(s, seeds):
    """REFERENCE A: uint32 d, NONE outside S and where no seed reaches."""
    d = numpy.full(s.shape, NONE, dtype=numpy.uint32)
    frontier = seeds & s
    reached = frontier.copy()
    k = 0
    while frontier.any():
        d[frontier] = k
        grown = numpy.zeros_like(frontier)
        for axis in range(3):
            grown |= shifted(frontier, axis, 1) | shifted(frontier, axis, -1)
        frontier = grown & s & ~reached
        reached |= frontier
        k += 1
    return d


def sweep(dist, s, axis):
    """One sweep of hu_geodesic_sweep in place on the int64 field `dist`: along every line of `axis` a forward and then a backward
    walk; the carry is NONE at the start and after a sample outside S, v = min(dist, carry + 1 saturating at NONE) on a sample of
    S.  Entries outside S are neither read nor written -> whether an entry was lowered."""
    d, m = numpy.moveaxis(dist, axis, 0), numpy.moveaxis(s, axis, 0)              # views
    n = d.shape[0]
    lowered = False
    for order in (range(n), range(n - 1, -1, -1)):
        c = numpy.full(d.shape[1:], NONE, dtype=numpy.int64)
        for t in order:
            v = numpy.minimum(d[t], numpy.minimum(c + 1, NONE))                   # (NONE + 1 saturates back to NONE)
            low = m[t] & (v < d[t])
            lowered = lowered or bool(low.any())
            d[t][low] = v[low]
            c = numpy.where(m[t], v, NONE)
    return lowered


def swept(dist, s, axis):
    """(the field after one sweep along `axis`, whether it lowered an entry), `dist` left as it is."""
    out = dist.astype(numpy.int64)
    lowered = sweep(out, s, axis)
    return out.astype(numpy.uint32), lowered


def seeded(s, seeds):
    return numpy.where(s & seeds, 0, NONE).astype(numpy.uint32)


def reference_rounds(s, seeds):
    """REFERENCE B: ([the uint32 field after round 1, 2, ...], rounds)."""
    d = seeded(s, seeds).astype(numpy.int64)
    fields = []
    while True:
        lowered = False
        for axis in (2, 1, 0):
            lowered |= sweep(d, s, axis)
        fields.append(d.astype(numpy.uint32))
        if not lowered:
            return fields, len(fields)


def border_of(shape):
    rim = numpy.zeros(shape, dtype=bool)
    rim[[0, -1], :, :] = rim[:, [0, -1], :] = rim[:, :, [0, -1]] = True
    return rim


def layer_of(shape, axis, layer):
    at = numpy.zeros(shape, dtype=bool)
    index = [slice(None)] * 3
    index[axis] = layer
    at[tuple(index)] = True
    return at


def listed(shape, samples):
    at = numpy.zeros(shape, dtype=bool)
    for p in samples:
        at[tuple(int(v) for v in p)] = True
    return at


def plate_of(s, axis, up):
    """The seeds of Plate(axis, up): S in the least layer that holds a sample of it."""
    held = numpy.flatnonzero(s.any(axis=tuple(a for a in range(3) if a != axis)))
    if len(held) == 0:
        return numpy.zeros(s.shape, dtype=bool)
    return s & layer_of(s.shape, axis, int(held[0] if up else held[-1]))


def seeds_of(source, s, corner=None, step=None):
    """bool: the seeds of a `source` of flow_length() on the set `s` (Gates through the module's own mapping, which the host
    test checks by hand)."""
    if isinstance(source, fl.Plate):
        return plate_of(s, source.axis, source.up)
    if isinstance(source, fl.Samples):
        return listed(s.shape, source.indices)
    if isinstance(source, fl.Gates):
        return listed(s.shape, fl.nearest_samples(source.points, corner, step, s.shape))
    assert source == fl.BORDER
    return s & border_of(s.shape)


def farthest_of(d, own):
    """(the greatest finite d over the bool `own`, the lexicographically first sample that has it), or None."""
    got = own & (d != NONE)
    if not got.any():
        return None
    far = int(d[got].max())
    return far, tuple(int(v) for v in numpy.argwhere(got & (d == far))[0])        # (argwhere: in C order, x slowest)


def stats(ids, of, d, n):
    """The per-part fields of a FlowLengthReport from the field `d`: lists over the n parts, single values under EMPTY_SPACE."""
    s = in_set_of(ids, of)
    owners = [s] if of == EMPTY_SPACE else [s & (ids == k) for k in range(n)]
    fields = [[int((own & (d != NONE)).sum()) for own in owners], [int((own & (d == NONE)).sum()) for own in owners],
              [int(d[own & (d != NONE)].astype(numpy.int64).sum()) for own in owners], [farthest_of(d, own) for own in owners]]
    return Stats(*([f[0] for f in fields] if of == EMPTY_SPACE else fields))


def raw_stats(ids, of, d, pitch):
    """(uint64[65] keys, uint64[3][65] counts) as hu_geodesic_stats leaves them over zeros."""
    s = in_set_of(ids, of)
    keys, counts = numpy.zeros(SLOTS, dtype=numpy.uint64), numpy.zeros((3, SLOTS), dtype=numpy.uint64)
    for slot in ([64] if of == EMPTY_SPACE else range(64)):
        own = s if slot == 64 else s & (ids == slot)
        got = own & (d != NONE)
        counts[0, slot], counts[1, slot] = int(got.sum()), int((own & ~got).sum())
        counts[2, slot] = int(d[got].astype(numpy.int64).sum())
        far = farthest_of(d, own)
        if far is not None:
            x, y, z = far[1]
            keys[slot] = (far[0] + 1) << 32 | (0xffffffff - ((x * ids.shape[1] + y) * pitch + z))
    return keys, counts


def padded32(values, fill, pitch=None):
    """raw_volume_scenes.padded for a uint32 volume."""
    return raw._fill(numpy.uint32, values, fill, pitch)


# ---- raw volumes ------------------------------------------------------------------------------------------------------

def some_ids(rng, shape, empty=0.3):
    """Ids from 0..63, about a third of them 3 (so that of = 3 has runs) and `empty` of the samples empty."""
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.35] = 3
    ids[rng.random(shape) < empty] = EMPTY
    return ids


def some_field(rng, shape, s):
    """No distance field: small values, NONE, and values near 2^31 and near NONE; outside S arbitrary values of their own."""
    field = rng.integers(0, 40, size=shape).astype(numpy.uint32)
    pick = rng.random(shape)
    field[pick < 0.45] = NONE
    field[(pick >= 0.45) & (pick < 0.5)] = rng.integers(2 ** 31 - 2, 2 ** 31 + 2, size=int(((pick >= 0.45) & (pick < 0.5)).sum()))
    field[(pick >= 0.5) & (pick < 0.53)] = NONE - 1
    outside = rng.integers(0, 2 ** 32, size=shape, dtype=numpy.uint64).astype(numpy.uint32)
    outside[rng.random(shape) < 0.3] = 0                                              # zeros outside S: they would seed
    return numpy.where(s, field, outside)


SERPENTINE = (21, 3, 70)


@functools.lru_cache(maxsize=None)
def serpentine():
    """(ids, seeds): a block of one part with walls of empty samples at odd x, each open at alternating ends z = 69 and z = 0,
    seeded along (0, :, 0): ten turns, 779 steps to the far end."""
    ids = numpy.zeros(SERPENTINE, dtype=numpy.uint8)
    for k, x in enumerate(range(1, SERPENTINE[0], 2)):
        ids[x, :, :] = EMPTY
        ids[x, :, SERPENTINE[2] - 1 if k % 2 == 0 else 0] = 0
    seeds = numpy.zeros(SERPENTINE, dtype=bool)
    seeds[0, :, 0] = True
    ids.setflags(write=False), seeds.setflags(write=False)
    return ids, seeds


def random_volume(seed, shape=None, density=None, parts=3):
    """(ids, of, seeds): a seeded volume of `parts` parts, a set and seeds on it (a plane, the border, or a few samples)."""
    rng = numpy.random.default_rng(5200 + seed)
    if shape is None:
        shape = tuple(int(v) for v in rng.integers(1, 12, size=3))
    ids = rng.integers(0, parts, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) >= (float(rng.uniform(0.4, 0.9)) if density is None else density)] = EMPTY
    of = (SOLID, EMPTY_SPACE, int(rng.integers(0, parts)))[seed % 3]
    s = in_set_of(ids, of)
    kind = seed % 4
    if kind == 0:
        seeds = layer_of(shape, 0, 0)
    elif kind == 1:
        seeds = border_of(shape)
    elif kind == 2:
        seeds = plate_of(s, int(rng.integers(0, 3)), bool(rng.integers(0, 2)))
    else:
        seeds = numpy.zeros(shape, dtype=bool)
        seeds.ravel()[rng.integers(0, seeds.size, size=3)] = True
    return ids, of, seeds & s


# ---- the scenarios of flow_length() -------------------------------------------------------------------------------------

def _part(n, boxes, name):
    return shapes.union([comp._box(n, lo, hi) for lo, hi in boxes]).make_part(name)


UBEND = (14, 6, 20)


def _ubend():
    """Two legs along z, 4 x 6 samples across, joined at the top: from the foot of one leg the way leads over the bridge."""
    n = UBEND
    return cc.assembly("ubend", [_part(n, [((0, 0, 0), (4, 6, 20)), ((10, 0, 0), (14, 6, 20)), ((4, 0, 16), (10, 6, 20))], "bend")])


PAIR = (16, 6, 6)


def _pair():
    """Two blocks end to end along x: as one solid the way passes through, as its own part each ends at the other."""
    n = PAIR
    return cc.assembly("pair", [_part(n, [((0, 0, 0), (8, 6, 6))], "left"), _part(n, [((8, 0, 0), (16, 6, 6))], "right")])


TABLE = (16, 8, 12)


def _table():
    """A top of 3 samples on two feet that end at different heights: upwards the plate is under the long foot alone, downwards
    it is the whole top."""
    n = TABLE
    return cc.assembly("table", [_part(n, [((0, 0, 9), (16, 8, 12)), ((0, 0, 0), (3, 8, 9)), ((13, 0, 4), (16, 8, 9))], "table")])


TOWER = (5, 4, 70)


def _tower():
    """70 samples along z: two words of a column; a notch leaves a neck at z = 63 | 64."""
    n = TOWER
    return cc.assembly("tower", [_part(n, [((0, 0, 0), (5, 4, 62)), ((0, 0, 62), (2, 4, 66)), ((0, 0, 66), (5, 4, 70))], "tower")])


def _nothing():
    return cc.assembly("nothing", [shapes.box(1).make_part("ghost").hidden()])


SCENES = {"ubend": _ubend, "pair": _pair, "table": _table, "tower": _tower, "shell": comp.SCENES["shell"].build, "nothing": _nothing}


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
    if not instances:
        return numpy.full(tuple(int(d) for d in dims), EMPTY, dtype=numpy.uint8)
    ids = voxels.reference_voxels(instances, corner, step, dims, True).ids
    ids.setflags(write=False)
    return ids


def position(name, index):
    """The world point of the sample `index` of a scene, in float64."""
    corner, step = scene(name)[3:5]
    return [float(numpy.float32(corner[a]) + numpy.float32(step) * numpy.float32(index[a])) for a in range(3)]


def first_of(name, of=SOLID):
    """The lexicographically first sample of the set of a scene."""
    return tuple(int(v) for v in numpy.argwhere(in_set_of(part_ids(name), of))[0])


def last_of(name, of=SOLID):
    return tuple(int(v) for v in numpy.argwhere(in_set_of(part_ids(name), of))[-1])


def _cases():
    return [
        Case("ubend_gate", "ubend", SOLID, lambda: fl.Gates([position("ubend", first_of("ubend"))])),
        Case("pair_solid", "pair", SOLID, lambda: fl.Gates([position("pair", first_of("pair", 0))])),
        Case("pair_left", "pair", 0, lambda: fl.Gates([position("pair", first_of("pair", 0))])),
        Case("pair_right_unseeded_side", "pair", 1, lambda: fl.Samples([last_of("pair", 1)])),
        Case("shell_void", "shell", EMPTY_SPACE, lambda: fl.BORDER),
        Case("shell_solid_border", "shell", SOLID, lambda: fl.BORDER),
        Case("table_up", "table", SOLID, lambda: fl.Plate(2, True)),
        Case("table_down", "table", SOLID, lambda: fl.Plate(2, False)),
        Case("table_x", "table", SOLID, lambda: fl.Plate(0, True)),
        Case("tower_two_seeds", "tower", SOLID, lambda: fl.Samples([first_of("tower"), last_of("tower")])),
        Case("tower_plate", "tower", SOLID, lambda: fl.Plate(2, False)),
        Case("nothing_void", "nothing", EMPTY_SPACE, lambda: fl.BORDER),         # every sample is empty: it runs on the device
    ]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

Reference = collections.namedtuple("Reference", "ids in_set seeds steps rounds stats")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The Reference of a case (by name): reference A on the reference part ids, the rounds of reference B; computed once and
    shared; nobody changes it."""
    c = BY_NAME[name]
    asm, resolution, instances, corner, step, dims = scene(c.scene)
    ids = part_ids(c.scene)
    s = in_set_of(ids, c.of)
    seeds = seeds_of(c.source(), s, corner, step)
    d = reference_steps(s, seeds)
    d.setflags(write=False)
    fields, rounds = reference_rounds(s, seeds)
    assert numpy.array_equal(fields[-1], d)
    return Reference(ids, s, seeds, d, rounds, stats(ids, c.of, d, len(instances)))
