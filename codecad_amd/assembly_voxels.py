"""The part-id voxel volume of an assembly: which part owns which sample of the lattice.

`assembly_voxels(asm, resolution) -> AssemblyVoxels`.  The answer is defined on the lattice of `interference()`, densely.

  * INSTANCES AND LATTICE.  Exactly those of `interference(asm, resolution)`: `_instance_cells.visible` and
    `checked_lattice`; sample (x, y, z) sits at `corner + step * (float)index` per axis in float32 (kernels.hpp sample()).
    One visible instance is enough; none (or no top row) gives a volume of all EMPTY with `traversals == 0`.  ValueError
    as there: a 2D assembly, more than 64 visible instances, a bad resolution, more than 65536 samples on an axis.
  * INSIDE.  Sample p is inside instance k when the tape of that instance alone gives w_k(p) < 0, strictly; a NaN is not
    inside.
  * PART_IDS.  uint8[nx, ny, nz] in C order: the lowest visible index k that contains the sample -- the owner rule of
    `section()`'s `part_ids`, of the assembly picture's ids and of the sets O_k of `assembly_mass_properties()` --, or
    EMPTY = 255 for a sample inside no part.  Bit for bit what evaluating every instance at every sample gives.
  * COUNTS.  One Python int per instance, n(O_k), counted on the device in uint64: equal to `(part_ids == k).sum()` and to
    `assembly_mass_properties(...).parts[k].owned_sums[0]`.
  * DEVICE BUFFER.  uint8[nx, ny, pz], pz = nz rounded up to a multiple of 16: every cell's z run starts on an aligned
    dword and every z run of a cell of 16 samples or more on an aligned 16 bytes.  The host returns the view
    [:, :, :nz]; the content of the padding is unspecified.  ValueError when nx * ny * pz > max_bytes.  Byte offsets on
    the device are 64-bit.  The buffer is prefilled with EMPTY once, before the first traversal; a traversal repeated
    after a list overflowed writes the same bytes again (what a cell writes depends on the cell alone, and a list that
    overflowed holds a subset of the cells of the list that did not); the accumulators are reset per run.

It is computed sparsely on the device by the traversal under `interference()` (_instance_cells.py) over its default
16-byte row with one more bit (csrc/instance_voxels.hip):
    {x0 | y0 << 16, z0 | capped << 31, cand lo, cand hi},
capped: the HIGHEST bit of cand is full in this cell -- every sample of the cell is inside that instance.  Candidates
above a full one are never listed, they cannot own a sample of the cell.  The host seeds the top level from the
instances' windows (every cell a window reaches, capped = 0).  A level evaluates the candidates of each child cell of s
samples a side at its centre in ASCENDING index (a capped top bit is inherited) and, with
thr = (s * step * sqrt(3) / 2) * (1 + 2^-10), the threshold of `assembly_mass_properties()`,
    w >= thr  drops the candidate,    w < -thr  makes it full,    anything else (a NaN too) leaves it a boundary candidate;
a lane keeps nothing above its lowest full candidate, and a wavefront stops evaluating once every live child has a full
one.  A child with no candidate is dropped (the prefill stands); a child whose LOWEST candidate is full is RETIRED: its
extent is filled with that index and counted; any other child is listed, capped when its highest bit is full.

THE RETIRE RULE IN TWO LINES.
 1. w(c) < -thr puts every sample of the child inside k: the premise of `assembly_mass_properties()`.
 2. Every lower index was dropped by w >= thr or by its window, so it is inside nowhere in the child.  Hence k owns every
    sample, whatever lies above it -- a stronger rule than the mass properties can use, which need every candidate full.

The finest level (4^3 samples) evaluates every candidate but a capped one at every sample: id = the lowest inside, else
the capped one, else EMPTY.  `retire=False` makes nothing full: the same kernels, every cell descends to the finest
level, the same volume -- the comparison arm.  `samples_evaluated` counts live lanes x candidates a wavefront evaluated.

PREMISE.  That of `assembly_mass_properties()`: on BOTH sides of the surface |w| does not exceed the distance to it, and
the bounding box holds the instance.  Shapes from `shapes.unsafe` break it; then the volume may differ from `retire=False`.
"""
import collections
import ctypes

import numpy

from . import _instance_cells as cells
from . import hip_util
from .hip_util import manager as hip_manager, check
from ._instance_cells import Instance
from .assembly_mass import threshold

EMPTY = 255                 # the id of a sample inside no part
SOLID = "solid"             # the set `of` every sample inside some part, for the checks that take a set (assembly_components.py)
_SOLID_CODE = 255           # ... as their entry points take it: include/hip_util.h HU_THICKNESS_SOLID, HU_OVERHANG_SOLID
_RUN = 16                   # a z run of the device buffer is a multiple of this many bytes
_ACC = numpy.dtype("<u8")   # n counts, then the bytes retired children filled


class AssemblyVoxels(collections.namedtuple("AssemblyVoxels", "instances corner step dims part_ids counts samples_evaluated "
                                                              "traversals")):
    """`instances`, `corner`, `step`, `dims`: as in InterferenceReport; `part_ids`: uint8[nx, ny, nz], the index of the
    visible instance that owns a sample or EMPTY; `counts`: the samples each instance owns; `samples_evaluated`:
    per-instance sample evaluations of the last traversal, on every level; `traversals`: how often it ran (more than once
    when a cell list overflowed; 0 when nothing was launched)."""

    __slots__ = ()

    def mask(self, k):
        """bool[nx, ny, nz]: the samples instance `k` owns."""
        return self.part_ids == k

    def layer(self, z):
        """uint8[nx, ny]: lattice plane `z`."""
        return self.part_ids[:, :, z]

    def volumes(self):
        """float64[n]: counts * step^3."""
        return numpy.array(self.counts, dtype=numpy.float64) * float(self.step) ** 3


def volume_shape(dims, max_bytes, sample_bytes=1):
    """(nx, ny, pz) of the device buffer over a lattice of `dims`; ValueError when it has more than `max_bytes` bytes at
    `sample_bytes` a sample (a caller that keeps further volumes of that shape beside the ids counts them in)."""
    nx, ny, nz = (int(d) for d in dims)
    pz = -(-nz // _RUN) * _RUN
    if nx * ny * pz * sample_bytes > max_bytes:
        raise ValueError("a lattice of %s samples needs a volume of %d bytes, more than max_bytes = %d; use a coarser resolution"
                         % ([nx, ny, nz], nx * ny * pz * sample_bytes, max_bytes))
    return nx, ny, pz


def top_rows(instances, corner, step, dims, side):
    """uint32[n, 4] rows of the top level: every cell of `side` samples that a window reaches, nothing capped."""
    return cells.cell_rows(cells.windows(instances, corner, float(step), dims), dims, side, least=1)


def _voxels(instances, corner, step, dims, part_ids, counts, evaluations, traversals):
    return AssemblyVoxels([Instance(i.name, i) for i in instances], corner, step, dims, part_ids, [int(c) for c in counts],
                          evaluations, traversals)


def _whole(v, least, most):     # what a caller of _device_volume() needs beside it starts here (the device's: csrc/id_volume.hpp)
    return isinstance(v, (int, numpy.integer)) and not isinstance(v, bool) and least <= v <= most


def _of_code(of, n):
    if of != SOLID and not _whole(of, 0, n - 1):
        raise ValueError("of must be SOLID or the index of one of the %d visible instances, not %r" % (n, of))
    return _SOLID_CODE if of == SOLID else int(of)


def _axis(axis):
    if not _whole(axis, 0, 2):
        raise ValueError("axis must be 0, 1 or 2, not %r" % (axis,))
    return int(axis)


def _dims(shape):
    return (ctypes.c_uint32 * 3)(*(int(d) for d in shape))


def _cropped(buffer, nz):
    return numpy.ascontiguousarray(buffer.read()[:, :, :nz])


class _LabelMask:
    __slots__ = ()

    def mask(self, region, /):
        """bool[nx, ny, nz]: the samples of `region` (one of the report's Components or a label)."""
        return self.labels == getattr(region, "label", region)


def assembly_voxels(asm, resolution, initial_capacity=None, retire=True, max_bytes=2 ** 32):
    """The part-id volume of the visible instances of the 3D assembly `asm` on the lattice of `interference(asm,
    resolution)` (the module's docstring defines it and says what the traversal assumes) -> AssemblyVoxels.

    `retire=False` retires no cell: every sample a part may own is evaluated at the finest level (the same volume,
    slower).  `initial_capacity` caps the first guess of every cell list, as in interference().  Raises ValueError for
    what interference() refuses and for a volume of more than `max_bytes` bytes."""
    voxels, volume = _device_volume(asm, resolution, initial_capacity, retire, max_bytes)
    if volume is not None:
        volume.release()
    return voxels


def _device_volume(asm, resolution, initial_capacity, retire, max_bytes, sample_bytes=1, check_dims=None):
    """assembly_voxels() for a caller that goes on with the volume on the device (assembly_components.py) ->
    (AssemblyVoxels, the uint8[nx, ny, pz] Buffer, still the caller's to release -- or None when nothing was launched).
    `sample_bytes`: what the caller keeps per sample of that shape, the ids included, against `max_bytes`;
    `check_dims(dims)`: the caller's own refusals, before anything is launched."""
    instances = cells.visible(asm, resolution)
    corner, step, dims = cells.checked_lattice(instances, resolution)
    nx, ny, pz = volume_shape(dims, max_bytes, sample_bytes)
    if check_dims is not None:
        check_dims(dims)
    n = len(instances)
    side = cells.top_side(dims)
    top = top_rows(instances, corner, step, dims, side) if n else ()
    if len(top) == 0:
        return _voxels(instances, corner, step, dims, numpy.full(tuple(int(d) for d in dims), EMPTY, numpy.uint8), [0] * n, 0, 0), None
    queue = hip_manager.queue
    volume = hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue)
    check(hip_manager.lib.hu_memset(volume.device_ptr, EMPTY, volume.size, queue.handle), "hu_memset")
    where = (volume.device_ptr, pz)
    evaluations, acc, traversals = cells.traverse(
        instances, top, side, corner, step, dims, initial_capacity, pair_dtype=_ACC, pair_init={},
        thr=lambda child: threshold(child, step), cells="hu_assembly_voxels_cells", finest=[("hu_assembly_voxels_leaf", where)],
        cells_extra=(int(bool(retire)),) + where, accumulators=n + 1)
    part_ids = volume.read()[:, :, :int(dims[2])]
    return _voxels(instances, corner, step, dims, part_ids, acc[:n], evaluations, traversals), volume
