"""How far it is through the material: the shortest paths inside a set of the part-id volume from gates, from the plate or from
the lattice's rim -- the geodesic distance in 6-steps --, by a min-plus relaxation along the lattice lines that is repeated on
the device until it changes nothing.  `wall_thickness()` says how thick a wall is; this says how long the way through it is:
the flow length from a gate (divided by the thickness, the L/t ratio that decides whether a cavity fills; the last sample to
fill is where the vent goes), the conduction path down to the plate, the way out of a channel.

`flow_length(asm, resolution, source, of=SOLID) -> FlowLengthReport`.  Everything is defined on the index space Z^3 of the
lattice of `assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `thin_walls()`, through the same helpers: the same ValueErrors, the same
    `retire=True` traversal, the same bytes.
  * THE SET S.  `of=SOLID`: the samples with part_ids != 255; `of=k`: those with part_ids == k; `of=EMPTY_SPACE` (the constant
    of `assembly_components`): those with part_ids == 255.  Nothing outside the lattice is in S.  A STEP joins two 6-neighbours
    that are both in S.
  * SEEDS.  `source` is `Gates(points)`: world points, each mapped to the sample whose position -- corner + step * (float)index
    per axis in float32, as AssemblyVoxels defines it -- is nearest, compared in float64, a tie going to the lower index; a
    gate more than half a step outside the lattice's positions on some axis is OUTSIDE THE LATTICE.  `Samples(indices)`: integer
    (x, y, z) triples.  For both: 1 to 65536 (MAX_SEEDS) of them, ValueError for one outside the lattice or not in S, checked
    on the host against `part_ids`.  `Plate(axis=2, up=True)`: the samples of S in layer h0, the least layer along the axis
    that holds a sample of S, counted from index 0 when `up` and from the far end otherwise.  `BORDER`: the samples of S with
    an index of 0 or dims - 1 on some axis.  `seed_count`: how many samples that is.
  * STEPS.  d(p) = the least number of steps of a path inside S from a seed to p; 0 exactly on the seeds; NONE = 0xffffffff for a
    sample of S that no seed reaches and for every sample outside S.  `steps`, uint32[nx, ny, nz].
  * PER PART, accumulated on the device.  `reached_counts[k]`: the samples of S that instance k owns with d != NONE;
    `unreached_counts[k]`: those with d == NONE; `sum_steps[k]`: the sum of d over the former; `farthest[k]` = (d, (x, y, z)):
    the greatest finite d among them and the lexicographically first sample that has it, None when nothing of k is reached.
    Under `of=EMPTY_SPACE` each of the four is a single value.  `rounds`: how many rounds the device ran, the last one, which
    changed nothing, included.
No visible instance (or no top row) launches nothing: `steps` is all NONE, the counts are zeros, every `farthest[k]` None,
`rounds` 0 -- but under `of=EMPTY_SPACE`, where every sample of the lattice is in S: that runs on the device like any other,
over a volume of 255s.

ON THE DEVICE (csrc/instance_geodesic.hip).  `hu_geodesic_seed` writes every entry: 0 on the seeds, NONE elsewhere.  A ROUND is a
memset of one word, `hu_geodesic_sweep` along z, then y, then x, and a read of that word: a sweep walks every line of its axis
forwards and then backwards with a carry, v = min(d, carry + 1) on a sample of S, no carry after a sample outside it, and sets
the word when it lowered an entry.  Values only fall and the fixed point of d(p) = min(d(p), d(q) + 1) with the seeds at 0 is
the distance, so the rounds end after the first that leaves the word zero, the result is the same bytes whatever ran when,
and `rounds` is a number of the volume and the seeds alone: a straight way costs one round, every turn against the order
z, y, x about one more.  `hu_geodesic_stats` then gathers the per-part fields and everything is read back once.
DEVICE MEMORY.  The ids (1 byte a sample of the device buffer nx * ny * pz) and one uint32 volume: 5 bytes a sample.
ValueError when 5 * nx * ny * pz > max_bytes or nx * ny * pz > 2^31 (a key carries a 32-bit buffer index), before anything
is launched.
OUT OF SCOPE here: 18- or 26-neighbour and Euclidean geodesic metrics, a set restricted by a ball ("passable by a sphere of
diameter d": it needs the transform of empty space), weld lines and fill times, more than 64 instances, several devices,
pictures of the map.
"""
import collections

import numpy

from . import _instance_cells as cells
from . import hip_util
from .assembly_voxels import _device_volume, _of_code, _axis, _dims, _cropped, _whole, volume_shape, EMPTY
from .assembly_components import SOLID, EMPTY_SPACE
from .hip_util import manager as hip_manager, check

NONE = 0xffffffff               # include/hip_util.h HU_GEODESIC_NONE: d of a sample no seed reaches, and outside S
MAX_SEEDS = 65536               # HU_GEODESIC_MAX_SAMPLES
SAMPLE_BYTES = 5                # the ids and one uint32 volume
BORDER = "border"               # source: the samples of S on the lattice's rim
_EMPTY_CODE = 254               # HU_GEODESIC_EMPTY: `of` as the entry points take EMPTY_SPACE
_MODE_BORDER, _MODE_LAYER, _MODE_LIST = 0, 1, 2
_SLOTS = 65                     # HU_GEODESIC_SLOTS: 64 parts, and slot 64 for empty space

Gates = collections.namedtuple("Gates", "points")
Gates.__doc__ = "source: world points (x, y, z), each seeding the sample nearest to it."
Samples = collections.namedtuple("Samples", "indices")
Samples.__doc__ = "source: integer index triples (x, y, z) of the lattice."


class Plate(collections.namedtuple("Plate", "axis up", defaults=(2, True))):
    """source: the samples of S in the least layer along `axis` that holds one, counted from index 0 (`up`) or from the far end."""
    __slots__ = ()


class FlowLengthReport(collections.namedtuple("FlowLengthReport", "instances corner step dims of source part_ids steps counts "
                                              "reached_counts unreached_counts sum_steps farthest seed_count rounds "
                                              "samples_evaluated traversals")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    every other field: the module's docstring."""
    __slots__ = ()

    def in_set(self):
        """bool[nx, ny, nz]: S."""
        return in_set_of(self.part_ids, self.of)

    def unreached(self):
        """bool[nx, ny, nz]: the samples of S that no seed reaches."""
        return self.in_set() & (self.steps == NONE)

    def lengths(self):
        """float64[nx, ny, nz]: d * step, infinity where a sample of S is unreached, nan outside S."""
        out = self.steps.astype(numpy.float64) * float(self.step)
        out[self.steps == NONE] = numpy.inf
        out[~self.in_set()] = numpy.nan
        return out

    def last_to_fill(self, k=None):
        """(d, (x, y, z)) of the sample that is reached last: `farthest[k]`, or without `k` the greatest of them over all parts
        (among equal d the lexicographically first sample); None when nothing is reached."""
        if self.of == EMPTY_SPACE or k is not None:
            return self.farthest if k is None else self.farthest[k]
        found = [f for f in self.farthest if f is not None]
        return min(found, key=lambda f: (-f[0], f[1])) if found else None

    def path(self, p):
        """The samples from `p` back to a seed, [(x, y, z), ...] of length d(p) + 1: from a sample with d > 0 the first neighbour
        in the order -x, +x, -y, +y, -z, +z that is in S and has d - 1.  ValueError for a `p` outside S or unreached."""
        try:
            at = tuple(int(v) for v in p)
            inside = len(at) == 3 and all(_whole(v, 0, int(n) - 1) for v, n in zip(p, self.steps.shape))
        except TypeError:
            at, inside = None, False
        if not inside or int(self.steps[at]) == NONE or not self.in_set()[at]:
            raise ValueError("%r is no sample of the set that a seed reaches" % (p,))
        s, out = self.in_set(), [at]
        while int(self.steps[at]) > 0:
            d = int(self.steps[at])
            for axis in range(3):
                for side in (-1, 1):
                    q = at[:axis] + (at[axis] + side,) + at[axis + 1:]
                    if 0 <= q[axis] < self.steps.shape[axis] and s[q] and int(self.steps[q]) == d - 1:
                        break
                else:
                    continue
                break
            else:
                raise ValueError("steps is no distance field at %r" % (at,))
            at = q
            out.append(at)
        return out

    def ratio(self, thickness_sq):
        """float64[nx, ny, nz]: d / (2 * sqrt(L)), the flow length over the wall thickness (L/t) per sample, L the
        `thickness_sq` of a WallThicknessReport on the same lattice and set; infinity where unreached, nan where L is 0."""
        L = numpy.asarray(thickness_sq)
        if L.shape != self.steps.shape:
            raise ValueError("thickness_sq has the shape %s, the lattice %s" % (L.shape, self.steps.shape))
        with numpy.errstate(divide="ignore", invalid="ignore"):
            out = self.steps.astype(numpy.float64) / (2.0 * numpy.sqrt(L.astype(numpy.float64)))
        out[(self.steps == NONE) & (L != 0)] = numpy.inf
        out[L == 0] = numpy.nan
        return out


def in_set_of(part_ids, of):
    """bool like `part_ids`: S."""
    if of == SOLID:
        return part_ids != EMPTY
    return part_ids == (EMPTY if of == EMPTY_SPACE else of)


def positions(corner, step, n, axis):
    """float64[n]: the positions of the samples along `axis`, computed in float32 as the kernels compute them."""
    at = numpy.float32(corner[axis]) + numpy.float32(step) * numpy.arange(int(n), dtype=numpy.float32)
    return at.astype(numpy.float64)


def nearest_samples(points, corner, step, dims):
    """int64[n, 3]: the sample nearest to every world point of `points` (float64, a tie to the lower index), or a ValueError
    for a point more than half a step outside the lattice's positions."""
    points = numpy.asarray(points, dtype=numpy.float64)
    if points.ndim != 2 or points.shape[1] != 3 or not numpy.isfinite(points).all():
        raise ValueError("gates must be finite world points (x, y, z), not an array of shape %s" % (points.shape,))
    out = numpy.empty(points.shape, dtype=numpy.int64)
    half = float(step) / 2
    for axis in range(3):
        at = positions(corner, step, dims[axis], axis)
        g = points[:, axis]
        bad = (g < at[0] - half) | (g > at[-1] + half)
        if bad.any():
            raise ValueError("gate %s lies outside the lattice" % (points[int(numpy.flatnonzero(bad)[0])].tolist(),))
        out[:, axis] = numpy.abs(at[None, :] - g[:, None]).argmin(axis=1)          # (argmin: the first of equals)
    return out


def first_layer(in_set, axis, up):
    """The index along `axis` of layer h0, the least layer that holds a sample of S, or None while S is empty."""
    held = numpy.flatnonzero(in_set.any(axis=tuple(a for a in range(3) if a != axis)))
    if len(held) == 0:
        return None
    return int(held[0] if up else held[-1])


def seeds_of(source, part_ids, of, corner, step):
    """(mode, axis, layer, uint32[n, 3] or None, seed_count) as hu_geodesic_seed takes the seeds of `source`, or a ValueError."""
    s = in_set_of(part_ids, of)
    shape = s.shape
    if isinstance(source, str) and source == BORDER:
        rim = numpy.zeros(shape, dtype=bool)
        rim[[0, -1], :, :] = rim[:, [0, -1], :] = rim[:, :, [0, -1]] = True
        return _MODE_BORDER, 0, 0, None, int((s & rim).sum())
    if isinstance(source, Plate):
        axis, up = _axis(source.axis), bool(source.up)
        layer = first_layer(s, axis, up)
        if layer is None:
            return _MODE_LAYER, axis, 0, None, 0                                  # S is empty: the layer seeds nothing
        return _MODE_LAYER, axis, layer, None, int(numpy.take(s, layer, axis=axis).sum())
    if isinstance(source, Gates):
        listed = nearest_samples(source.points, corner, step, shape)
    elif isinstance(source, Samples):
        listed = numpy.asarray(source.indices)
        if listed.ndim != 2 or listed.shape[1] != 3 or listed.dtype.kind not in "iu":
            raise ValueError("samples must be integer index triples (x, y, z), not %s of shape %s" % (listed.dtype, listed.shape))
        listed = listed.astype(numpy.int64)
        bad = ((listed < 0) | (listed >= numpy.array(shape))).any(axis=1)
        if bad.any():
            raise ValueError("sample %s lies outside the lattice of %s samples" % (listed[int(numpy.flatnonzero(bad)[0])].tolist(), list(shape)))
    else:
        raise ValueError("source must be Gates(points), Samples(indices), Plate(axis, up) or BORDER, not %r" % (source,))
    if not 1 <= len(listed) <= MAX_SEEDS:
        raise ValueError("%d seeds: there must be 1 to %d" % (len(listed), MAX_SEEDS))
    outside = ~s[tuple(listed.T)]
    if outside.any():
        raise ValueError("seed %s is not in the set %r" % (listed[int(numpy.flatnonzero(outside)[0])].tolist(), of))
    return _MODE_LIST, 0, 0, numpy.ascontiguousarray(listed, dtype=numpy.uint32), len(numpy.unique(listed, axis=0))


def _check_entries(dims):
    nx, ny, pz = volume_shape(dims, 2 ** 62)
    if nx * ny * pz > 2 ** 31:
        raise ValueError("a lattice of %s samples has more than 2^31 distance entries; use a coarser resolution" % [int(d) for d in dims])


def flow_length(asm, resolution, source, of=SOLID, initial_capacity=None, max_bytes=2 ** 32):
    """The shortest paths inside the solid (or one part, or the empty space) of the visible instances of the 3D assembly `asm`
    on the lattice of `interference(asm, resolution)` from the seeds of `source`, in 6-steps (the module's docstring defines
    them) -> FlowLengthReport.

    `source`: Gates(points), Samples(indices), Plate(axis, up) or BORDER.  `of`: SOLID, the index of a visible instance or
    EMPTY_SPACE.  `initial_capacity` caps the first guess of every cell list of the voxel traversal.  Raises ValueError for what
    assembly_voxels() refuses, for a bad `of`, a bad source, a seed outside the lattice or the set, more than 2^31 entries and
    for volumes of more than `max_bytes` bytes together."""
    n = len(cells.visible(asm, resolution))
    void = isinstance(of, str) and of == EMPTY_SPACE
    code = _EMPTY_CODE if void else _of_code(of, n)
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES, check_dims=_check_entries)
    shape = tuple(int(d) for d in voxels.dims)

    def report(steps, totals, keys, seed_count, rounds):
        def farthest(slot):
            key = int(keys[slot])
            if key == 0:
                return None
            q = 0xffffffff - (key & 0xffffffff)
            row, z = divmod(q, pz)
            return (key >> 32) - 1, divmod(row, shape[1]) + (z,)
        slots = [64] if void else range(n)
        fields = [[int(totals[j][slot]) for slot in slots] for j in range(3)] + [[farthest(slot) for slot in slots]]
        if void:
            fields = [f[0] for f in fields]
        return FlowLengthReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, source, voxels.part_ids, steps, voxels.counts,
                                *fields, seed_count, rounds, voxels.samples_evaluated, voxels.traversals)

    pz = volume_shape(shape, 2 ** 62)[2]
    try:
        mode, axis, layer, listed, seed_count = seeds_of(source, voxels.part_ids, of, voxels.corner, voxels.step)
    except ValueError:
        if volume is not None:
            volume.release()
        raise
    if volume is None and not void:
        return report(numpy.full(shape, NONE, numpy.uint32), numpy.zeros((3, _SLOTS), numpy.uint64), numpy.zeros(_SLOTS, numpy.uint64),
                      seed_count, 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    if volume is None:
        volume = hip_util.Buffer(numpy.uint8, (shape[0], shape[1], pz), queue=queue)      # every sample is empty: a volume of 255s
        check(lib.hu_memset(volume.device_ptr, EMPTY, volume.size, queue.handle), "hu_memset")
    dims = _dims(shape)
    dist = hip_util.Buffer(numpy.uint32, volume.shape, queue=queue)
    keys = hip_util.Buffer(numpy.uint64, (_SLOTS,), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (3, _SLOTS), queue=queue)                    # reached, unreached, the sum of d
    word = hip_util.Buffer(numpy.uint32, (1,), queue=queue)
    buffers = [volume, dist, keys, acc, word]
    check(lib.hu_memset(keys.device_ptr, 0, keys.size, queue.handle), "hu_memset")
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    samples = None
    if listed is not None:
        samples = hip_util.Buffer(numpy.uint32, listed.shape, queue=queue)
        samples.enqueue_write(listed)
        buffers.append(samples)
    check(lib.hu_geodesic_seed(volume.device_ptr, dist.device_ptr, dims, pz, code, mode, axis, layer,
                               None if samples is None else samples.device_ptr, 0 if listed is None else len(listed), queue.handle),
          "hu_geodesic_seed")
    rounds = relax(hip_manager, volume.device_ptr, dist.device_ptr, word, dims, pz, code)
    check(lib.hu_geodesic_stats(volume.device_ptr, dist.device_ptr, keys.device_ptr, acc.device_ptr, dims, pz, code, queue.handle),
          "hu_geodesic_stats")
    steps = _cropped(dist, shape[2])
    greatest, totals = keys.read(), acc.read()
    for b in buffers:
        b.release()
    return report(steps, totals, greatest, seed_count, rounds)


def relax(manager, ids_ptr, dist_ptr, word, dims, pz, code):
    """Rounds of `hu_geodesic_sweep` along z, y and x over the seeded distances at `dist_ptr` until one leaves the Buffer `word`
    zero -> how many ran.  Between the launches the host waits only for the word of a round."""
    lib, queue = manager.lib, manager.queue
    rounds = 0
    while True:
        check(lib.hu_memset(word.device_ptr, 0, word.size, queue.handle), "hu_memset")
        for axis in (2, 1, 0):
            check(lib.hu_geodesic_sweep(ids_ptr, dist_ptr, word.device_ptr, dims, pz, axis, code, queue.handle), "hu_geodesic_sweep")
        rounds += 1
        if int(word.read()[0]) == 0:
            return rounds
