"""Which walls of an assembly are thinner than a ball: a morphological opening of the part-id volume with two radii, by an
exact Euclidean distance transform on the device.

`thin_walls(asm, resolution, min_thickness, of=SOLID) -> ThinWallReport`.  Everything is defined on the index space Z^3 of
the lattice of `assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)`: the same ValueErrors, the same
    `retire=True` traversal, the same bytes.  No visible instance (or no top row) gives a report with nothing thin (`depth_sq`
    all 0, `thin_ids` all 255, no region) and launches nothing.
  * THE SET S.  `of=SOLID` (the constant of `assembly_components`): the samples with part_ids != 255 -- a wall backed by
    another part is not thin; `of=k`, an int, a visible index: the samples with part_ids == k, the part as the assembly owns
    it.  Anything else, and a k out of range, is a ValueError.  (The thickness of EMPTY space, narrow channels, is not
    offered: it needs a margin around the lattice.)
  * BACKGROUND B.  Every point of Z^3 that is not in S: also every point outside the lattice -- the lattice covers every
    bounding box, outside is empty -- and the padding z in [nz, pz) of the device buffers, whose content is unspecified and
    which no kernel reads as data.
  * RADII.  Two integers, `radius_sq` (R2) and `cover_sq` (C2).  By default R2 = floor((min_thickness / (2 * float(step)))^2)
    in float64 and C2 = 3 * R2; both may be passed instead, R2 <= C2.  K1 = isqrt(R2), K2 = isqrt(C2).  ValueError for a
    `min_thickness` that is negative or not finite, for C2 < R2 and for C2 > 65534: distances are kept in uint16.
  * DEPTH.  D1(p) = min over q in B of |p - q|^2 for p in S.  `depth_sq` = min(D1, R2 + 1), uint16[nx, ny, nz], 0 outside S:
    capped, because nothing needs more.
  * CORE.  E = {p in S : D1(p) > R2}: the centres whose digital ball of squared radius R2 lies in S.
  * COVER.  D2(p) = min over q in E of |p - q|^2, C2 + 1 where there is no q within C2.  O = {p in S : D2(p) <= C2}.
  * THIN.  T = S \\ O.  `thin_ids`, uint8[nx, ny, nz] in the format of `part_ids`: part_ids where p is in T, 255 elsewhere.
  * PER PART.  `thin_counts[k]`, `core_counts[k]`: the samples of T, of E, that instance k owns, counted on the device in
    uint64; `counts[k]`: the samples it owns at all, from the voxel traversal.
  * REGIONS.  The 6-connected components of T as `Component`s of `assembly_components` (label, count, box, index sums, border
    flag, `parts` = the owners of the region's samples, volume, centroid), ordered by label, found by that module's kernels
    over `thin_ids`; `labels`, uint32[nx, ny, nz], holds a region's label at its samples and NONE elsewhere.

WHY TWO RADII.  With C2 = R2 this is the textbook opening by a digital ball, and it flags every sharp convex edge of every
block: the ball does not reach into a corner.  With C2 = 3 * R2 two facts hold (tests/test_thin_walls_host.py proves both):
  1. an axis-aligned cuboid with every side at least 2 * K1 + 1 samples has T empty -- its core is the cuboid shrunk by K1 on
     every side, and the corner sample is 3 * K1^2 <= C2 from the core's corner, every other sample nearer;
  2. an isolated slab of w samples (its other sides at least 2 * K1 + 1) is wholly thin exactly when ceil(w / 2)^2 <= R2, and
     otherwise wholly kept.
Physically: a wall of thickness h holds between h / step - 1 and h / step + 1 samples across, and it is flagged when
ceil(w / 2) <= K1 = floor(min_thickness / (2 step)), that is when w * step is at most min_thickness rounded down to a
multiple of 2 steps: the verdict agrees with h < min_thickness to within one step on either side.

ON THE DEVICE (csrc/instance_thickness.hip).  The transform is separable: each of the two is a pass along z, then y, then x,
a capped min-plus stencil out(i) = min(cap, min over |k| <= K of in(i + k) + k^2) with cap = R2 + 1, K = K1 (transform 1,
outside the lattice counts as 0) and cap = C2 + 1, K = K2 (transform 2, outside counts as the cap).  The z pass of transform
1 reads the ids, that of transform 2 reads depth_sq and takes > R2 ? 0 : cap on the fly -- the core is never stored; the x
pass of transform 1 also counts the core per part, that of transform 2 writes `thin_ids` and counts the thin samples.
`lds=True` stages a workgroup's lines with their halo of K in LDS (along y and x while K <= 96: tile + 2 K rows of 128 bytes
fit the kernel's 32 KiB; above that the taps come from global memory); `lds=False` reads every tap from global memory
everywhere -- the comparison arm: the same bytes.
DEVICE MEMORY.  At the peak the ids (1 byte a sample of the device buffer nx * ny * pz) and three uint16 volumes are held
together: 7 bytes a sample; the labelling afterwards holds the thin ids and the labels, 5.  ValueError when
7 * nx * ny * pz > max_bytes, and when the label volume would have more than 2^31 entries, before anything is launched.
"""
import collections
import math

import numpy

from . import _instance_cells as cells
from . import hip_util
from .assembly_voxels import _device_volume, _of_code, _dims, _cropped, _LabelMask, EMPTY
from .assembly_components import SOLID, NONE, _components, _label_volume, _check_entries
from .hip_util import manager as hip_manager, check

MAX_COVER_SQ = 65534            # C2 + 1 is the largest uint16
SAMPLE_BYTES = 7                # the ids and three uint16 volumes: what is held per sample at the peak
LDS_ROWS = 256                  # include/hip_util.h HU_THICKNESS_LDS_ROWS: rows of 64 uint16 a workgroup may stage
_GLOBAL_TILE = 64               # positions along the axis a workgroup takes when it reads its taps from global memory
_MAX_LDS_K = 96                 # the tile of the LDS path, LDS_ROWS - 2 K, is at least 64 up to here


class ThinWallReport(_LabelMask, collections.namedtuple("ThinWallReport", "instances corner step dims of radius_sq cover_sq part_ids depth_sq "
                                                              "thin_ids counts core_counts thin_counts regions labels "
                                                              "samples_evaluated traversals component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `component_capacity_runs`: as in ComponentsReport; every other field: the module's docstring."""
    __slots__ = ()


def radii(step, min_thickness=None, radius_sq=None, cover_sq=None):
    """(R2, C2) as the module's docstring defines them, or a ValueError."""
    if radius_sq is None:
        if not (isinstance(min_thickness, (int, float, numpy.floating, numpy.integer)) and math.isfinite(min_thickness)
                and min_thickness >= 0):
            raise ValueError("min_thickness must be a finite number that is not negative, not %r" % (min_thickness,))
        half = float(min_thickness) / (2.0 * float(step))
        radius_sq = half * half
        if radius_sq > MAX_COVER_SQ:
            raise ValueError("min_thickness = %g is more than %d steps: distances are kept in uint16; use a coarser resolution"
                             % (min_thickness, 2 * math.isqrt(MAX_COVER_SQ)))
        radius_sq = math.floor(radius_sq)
    r2 = int(radius_sq)
    c2 = 3 * r2 if cover_sq is None else int(cover_sq)
    if r2 < 0 or r2 != radius_sq or (cover_sq is not None and c2 != cover_sq):
        raise ValueError("radius_sq and cover_sq must be integers that are not negative")
    if c2 < r2:
        raise ValueError("cover_sq = %d is below radius_sq = %d" % (c2, r2))
    if c2 > MAX_COVER_SQ:
        raise ValueError("cover_sq = %d is above %d: distances are kept in uint16; use a coarser resolution" % (c2, MAX_COVER_SQ))
    return r2, c2


def axis_tile(K, lds):
    """(positions along the axis a workgroup of a y or x pass takes, whether it stages them in LDS)."""
    return (LDS_ROWS - 2 * K, 1) if lds and K <= _MAX_LDS_K else (_GLOBAL_TILE, 0)


def thin_walls(asm, resolution, min_thickness=None, of=SOLID, radius_sq=None, cover_sq=None, lds=True, initial_components=None,
               initial_capacity=None, max_bytes=2 ** 32):
    """The samples of the visible instances of the 3D assembly `asm`, on the lattice of `interference(asm, resolution)`, that no
    ball of diameter `min_thickness` inside the solid covers (the module's docstring defines them) -> ThinWallReport.

    `of`: SOLID, or the index of a visible instance.  `radius_sq`, `cover_sq`: the two radii in squared steps, instead of
    `min_thickness`.  `lds=False` reads every tap from global memory (the same result, the comparison arm).
    `initial_components` caps the first guess of the region table, `initial_capacity` that of every cell list of the voxel
    traversal.  Raises ValueError for what assembly_voxels() refuses, for a bad `of`, bad radii, more than 2^31 label entries
    and for volumes of more than `max_bytes` bytes together."""
    n = len(cells.visible(asm, resolution))
    code = _of_code(of, n)
    r2, c2 = radii(numpy.float32(resolution), min_thickness, radius_sq, cover_sq)
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES,
                                    check_dims=_check_entries)
    shape = tuple(int(d) for d in voxels.dims)

    def report(depth, thin, core_counts, thin_counts, regions, labels, runs):
        return ThinWallReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, r2, c2, voxels.part_ids, depth, thin,
                              voxels.counts, core_counts, thin_counts, regions, labels, voxels.samples_evaluated, voxels.traversals, runs)

    if volume is None:
        return report(numpy.zeros(shape, numpy.uint16), numpy.full(shape, EMPTY, numpy.uint8), [0] * n, [0] * n, [],
                      numpy.full(shape, NONE, numpy.uint32), 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)
    k1, k2 = math.isqrt(r2), math.isqrt(c2)
    z_lds = int(bool(lds))

    def axis_pass(source, target, axis, K, cap, outside, finish=0, thin=None, counts=0):
        tile, staged = axis_tile(K, lds)
        check(lib.hu_thickness_pass_axis(source.device_ptr, target.device_ptr if target is not None else None, volume.device_ptr if finish else None,
                                         thin.device_ptr if thin is not None else None, counts or None, dims, pz, axis, code, K, cap,
                                         outside, finish, tile, staged, queue.handle), "hu_thickness_pass_axis")

    depth = hip_util.Buffer(numpy.uint16, (nx, ny, pz), queue=queue)
    other = hip_util.Buffer(numpy.uint16, (nx, ny, pz), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (2, 64), queue=queue)          # the core and the thin samples per part
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    # transform 1: the squared distance to the background, capped at R2 + 1; outside the lattice is background
    check(lib.hu_thickness_pass_z(volume.device_ptr, None, depth.device_ptr, dims, pz, code, r2, k1, r2 + 1, z_lds, queue.handle),
          "hu_thickness_pass_z")
    axis_pass(depth, other, 1, k1, r2 + 1, 0)
    axis_pass(other, depth, 0, k1, r2 + 1, 0, finish=1, counts=acc.device_ptr)
    # transform 2: the squared distance to the core, capped at C2 + 1; there is no core outside the lattice
    third = hip_util.Buffer(numpy.uint16, (nx, ny, pz), queue=queue)
    check(lib.hu_thickness_pass_z(None, depth.device_ptr, other.device_ptr, dims, pz, code, r2, k2, c2 + 1, z_lds, queue.handle),
          "hu_thickness_pass_z")
    axis_pass(other, third, 1, k2, c2 + 1, c2 + 1)
    other.release()
    thin = hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue)
    axis_pass(third, None, 0, k2, c2 + 1, c2 + 1, finish=2, thin=thin, counts=acc.device_ptr + 64 * 8)
    depth_sq, thin_ids = _cropped(depth, shape[2]), _cropped(thin, shape[2])
    totals = acc.read()
    for b in (depth, third, volume, acc):
        b.release()
    labels, rows, runs = _label_volume(thin, shape, 1, True, initial_components)
    return report(depth_sq, thin_ids, [int(v) for v in totals[0, :n]], [int(v) for v in totals[1, :n]],
                  _components(rows, voxels.corner, voxels.step), labels, runs)
