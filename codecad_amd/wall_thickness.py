"""How thick an assembly is at every sample: the local thickness of the part-id volume -- over every sample the greatest ball
inside the solid that contains it -- by an exact capped distance transform and one dense gather on the device.  `thin_walls()`
says yes or no for one threshold chosen beforehand; this is the map to colour a part by, and per part the thinnest spot and
where it is.

`wall_thickness(asm, resolution, max_thickness=None, of=SOLID, radius_sq=None) -> WallThicknessReport`.  Everything is defined
on the index space Z^3 of the lattice of `assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in
which anything ran.

  * INSTANCES, LATTICE, PART_IDS, THE SET S, BACKGROUND B.  Exactly those of `thin_walls()`, through the same helpers: the same
    ValueErrors, the same `retire=True` traversal, the same bytes.  `of=SOLID`: the samples with part_ids != 255; `of=k`: those
    with part_ids == k.  Every point outside the lattice is background, and the padding z in [nz, pz) of the device buffers is
    never read as data.  (The thickness of EMPTY space is not offered, for the reason thin_walls.py gives: it needs a margin
    around the lattice.)
  * RADIUS.  R2 = `radius_sq`, or floor((max_thickness / (2 * float(step)))^2) in float64 as `thin_walls.radii` computes it: an
    integer 0..1024 (MAX_RADIUS_SQ); K = isqrt(R2) <= 32; CAP = R2 + 1.  ValueError outside that range.
  * DEPTH.  D(p) = min(D1(p), CAP) for p in S, D1 the squared distance to B, and 0 elsewhere: `depth_sq` of `thin_walls()` with
    the same R2, uint16[nx, ny, nz].
  * THICKNESS.  For p in S, L(p) = the greatest D(q) over the q with |p - q|^2 < D(q): the (capped) squared radius of the
    greatest ball inside S that contains p.  q = p always qualifies, so L >= D >= 1; L = 0 outside S.  `thickness_sq`,
    uint16[nx, ny, nz].
  * WHAT IT MEANS.  L(p) - 1 is the greatest v in 0..R2 for which the opening of S by the digital ball of squared radius v keeps
    p -- the greatest v for which `thin_walls(radius_sq=v, cover_sq=v)` does not flag p: that opening keeps p exactly when some q
    has |p - q|^2 <= v < D1(q), and over the q with |p - q|^2 < D(q) the greatest such v is D(q) - 1.  In particular {L <= R2} is
    exactly the thin set of `thin_walls(radius_sq=R2, cover_sq=R2)`, and L == CAP means "at least the cap".
    tests/test_wall_thickness_host.py proves it.
  * SLABS.  An isolated slab of w samples reads ceil(w / 2)^2 throughout while that is <= R2, and CAP otherwise -- on a slab
    that ends, throughout the samples at least ceil(w / 2) samples from its rim; nearer to it the balls are the rim's.
  * THE CAP.  Digital openings are not nested, so L is NOT min(uncapped L, CAP): where the uncapped value is <= R2 the two agree
    (the test holds it on random volumes), but where the capped value is <= R2 the uncapped one can be larger -- a ball of a
    squared radius above R2 can contain a sample that no ball up to R2 inside S contains.
  * PER PART, accumulated on the device.  `min_sq[k]`: the least L over the samples instance k owns (within S), None when it
    owns none; `thinnest[k]`: the lexicographically first (x, y, z) among those samples, None likewise; `capped_counts[k]`: the
    samples of k with L == CAP; `core_counts[k]`: those with D == CAP; `counts[k]`: as in AssemblyVoxels.
No visible instance (or no top row) launches nothing: all fields zeros, every `min_sq[k]` and `thinnest[k]` None.

ON THE DEVICE.  Transform 1 exactly as `thin_walls()` runs it (csrc/instance_thickness.hip: z, y, x with K, cap = R2 + 1, the x
pass counting the core), then `hu_thickness_local` (csrc/instance_local.hip) on the same stream, no host wait in between, and
one read-back.  That kernel is the step that is not separable: a workgroup takes a tile of 8 x 8 x 16 samples, stages it and a
halo as uint16 in LDS (zeros outside the lattice, outside S and in the padding) while the halo is at most LDS_K = 16 -- the halo
of K up to K = 16, above that the halo that the greatest value around the tile can reach, found by reading first --, and
every lane looks over the ball around its sample, nearest offsets first: one read, one compare, one max per tap.  The saving is
in not searching: a lane is finished when it holds the greatest value it can meet and a wavefront leaves when a ballot says all
its lanes are; while staging, the workgroup reduces the greatest value M around its tile, no ball reaches further than
isqrt(M - 1), and the search shrinks to that -- a sheet costs what its thickness costs, not what K costs; a tile with M = 0
writes zeros and leaves.  `lds=False` reads every tap from global memory: the comparison arm, the same bytes.
DEVICE MEMORY.  The ids (1 byte a sample of the device buffer nx * ny * pz), two uint16 volumes for the passes and the result
are held together: 7 bytes a sample.  ValueError when 7 * nx * ny * pz > max_bytes, before anything is launched.
OUT OF SCOPE here: regions and labels of the thin samples (`thin_walls()` has them), empty space, more than 64 instances,
several devices, pictures of the map.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from . import hip_util
from .assembly_voxels import _device_volume, _of_code, _dims, _cropped, _whole
from .assembly_components import SOLID
from .hip_util import manager as hip_manager, check
from .thin_walls import axis_tile

MAX_RADIUS_SQ = 1024            # include/hip_util.h HU_LOCAL_MAX_RADIUS_SQ
LDS_K = 16                      # HU_LOCAL_LDS_K: the widest halo a workgroup stages
SAMPLE_BYTES = 7                # the ids, two uint16 volumes of the passes and the result
_NO_KEY = 0xffffffffffffffff    # a part that owns no sample of S leaves its key as it was


class WallThicknessReport(collections.namedtuple("WallThicknessReport", "instances corner step dims of radius_sq part_ids depth_sq "
                                                 "thickness_sq counts core_counts capped_counts min_sq thinnest "
                                                 "samples_evaluated traversals")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    every other field: the module's docstring."""
    __slots__ = ()

    @property
    def cap(self):
        """CAP = radius_sq + 1: what `thickness_sq` reads where the wall is at least as thick as was asked."""
        return self.radius_sq + 1

    def below(self, v):
        """bool[nx, ny, nz]: the samples of S with L <= v.  `below(radius_sq)` is the thin set of
        `thin_walls(radius_sq=radius_sq, cover_sq=radius_sq)`."""
        return (self.thickness_sq != 0) & (self.thickness_sq <= v)

    def diameters(self):
        """float64[nx, ny, nz]: 2 * sqrt(L) * step, infinity where L is the cap, 0 outside S: the wall's width to within one
        step either way (a slab of w samples reads ceil(w / 2)^2, so 2 * sqrt(L) is w or w + 1, and the wall it samples is
        between w - 1 and w + 1 steps wide)."""
        width = 2.0 * numpy.sqrt(self.thickness_sq.astype(numpy.float64)) * float(self.step)
        width[self.thickness_sq == self.cap] = numpy.inf
        return width

    def thinnest_part(self):
        """The index of the instance with the least `min_sq` (the lowest index among equals), None when no part owns a
        sample of S."""
        owned = [(v, k) for k, v in enumerate(self.min_sq) if v is not None]
        return min(owned)[1] if owned else None


def radius(step, max_thickness=None, radius_sq=None):
    """R2 as the module's docstring defines it, or a ValueError."""
    if radius_sq is not None:
        if not _whole(radius_sq, 0, MAX_RADIUS_SQ):
            raise ValueError("radius_sq must be an integer from 0 to %d, not %r" % (MAX_RADIUS_SQ, radius_sq))
        return int(radius_sq)
    # the rule of thin_walls.radii, which accepts and refuses the same values, with this module's limit in place of its own
    if not (isinstance(max_thickness, (int, float, numpy.floating, numpy.integer)) and math.isfinite(max_thickness)
            and max_thickness >= 0):
        raise ValueError("max_thickness must be a finite number that is not negative, not %r" % (max_thickness,))
    half = float(max_thickness) / (2.0 * float(step))
    if half * half >= MAX_RADIUS_SQ + 1:
        raise ValueError("max_thickness = %g is more than %d steps; use a coarser resolution or a smaller cap"
                         % (max_thickness, 2 * math.isqrt(MAX_RADIUS_SQ)))
    return math.floor(half * half)


def wall_thickness(asm, resolution, max_thickness=None, of=SOLID, radius_sq=None, lds=True, initial_capacity=None, max_bytes=2 ** 32):
    """The local thickness of the visible instances of the 3D assembly `asm` on the lattice of `interference(asm, resolution)`:
    over every sample the squared radius, in steps, of the greatest ball inside the solid that contains it, capped where the
    wall is at least `max_thickness` wide (the module's docstring defines it) -> WallThicknessReport.

    `of`: SOLID, or the index of a visible instance.  `radius_sq`: the cap's squared radius in steps, instead of
    `max_thickness`.  `lds=False` reads every tap from global memory (the same result, the comparison arm).
    `initial_capacity` caps the first guess of every cell list of the voxel traversal.  Raises ValueError for what
    assembly_voxels() refuses, for a bad `of`, a bad radius and for volumes of more than `max_bytes` bytes together."""
    n = len(cells.visible(asm, resolution))
    code = _of_code(of, n)
    r2 = radius(numpy.float32(resolution), max_thickness, radius_sq)
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES)
    shape = tuple(int(d) for d in voxels.dims)

    def report(depth, thickness, core_counts, capped_counts, keys):
        least = [None if k == _NO_KEY else int(k >> 48) for k in keys]
        where = [None if k == _NO_KEY else (int(k >> 32) & 0xffff, int(k >> 16) & 0xffff, int(k) & 0xffff) for k in keys]
        return WallThicknessReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, r2, voxels.part_ids, depth, thickness,
                                   voxels.counts, core_counts, capped_counts, least, where, voxels.samples_evaluated, voxels.traversals)

    if volume is None:
        return report(numpy.zeros(shape, numpy.uint16), numpy.zeros(shape, numpy.uint16), [0] * n, [0] * n, [_NO_KEY] * n)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)
    K, cap = math.isqrt(r2), r2 + 1
    tile, staged = axis_tile(K, lds)
    depth = hip_util.Buffer(numpy.uint16, (nx, ny, pz), queue=queue)
    other = hip_util.Buffer(numpy.uint16, (nx, ny, pz), queue=queue)
    thickness = hip_util.Buffer(numpy.uint16, (nx, ny, pz), queue=queue)
    keys = hip_util.Buffer(numpy.uint64, (64,), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (2, 64), queue=queue)          # the core and the capped samples per part
    check(lib.hu_memset(keys.device_ptr, 0xff, keys.size, queue.handle), "hu_memset")
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    # transform 1 as thin_walls() runs it: the squared distance to the background, capped at R2 + 1
    check(lib.hu_thickness_pass_z(volume.device_ptr, None, depth.device_ptr, dims, pz, code, r2, K, cap, int(bool(lds)), queue.handle),
          "hu_thickness_pass_z")
    check(lib.hu_thickness_pass_axis(depth.device_ptr, other.device_ptr, None, None, None, dims, pz, 1, code, K, cap, 0, 0, tile, staged,
                                     queue.handle), "hu_thickness_pass_axis")
    check(lib.hu_thickness_pass_axis(other.device_ptr, depth.device_ptr, volume.device_ptr, None, acc.device_ptr, dims, pz, 0, code, K, cap,
                                     0, 1, tile, staged, queue.handle), "hu_thickness_pass_axis")
    # the greatest ball over every sample, and per part the least of them, where, and how many read the cap
    check(lib.hu_thickness_local(depth.device_ptr, volume.device_ptr, thickness.device_ptr, keys.device_ptr, acc.device_ptr + 64 * 8, dims,
                                 pz, code, r2, int(bool(lds)), queue.handle), "hu_thickness_local")
    depth_sq, thickness_sq = _cropped(depth, shape[2]), _cropped(thickness, shape[2])
    least, totals = keys.read(), acc.read()
    for b in (volume, depth, other, thickness, keys, acc):
        b.release()
    return report(depth_sq, thickness_sq, [int(v) for v in totals[0, :n]], [int(v) for v in totals[1, :n]], [int(k) for k in least[:n]])
