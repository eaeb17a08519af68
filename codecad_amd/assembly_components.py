"""How the samples of an assembly's lattice hang together: connected components of empty space or of solid, and the
cavities among them -- the voids that no path joins to the outside.

`assembly_components(asm, resolution, of=EMPTY_SPACE) -> ComponentsReport`, `cavities(asm, resolution) -> CavityReport`.
Everything is defined on the part-id volume of `assembly_voxels(asm, resolution)` and computed on the device from the buffer
that call leaves there; every figure is an integer, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)`: the same ValueErrors, the same
    `retire=True` traversal, the same bytes.  No visible instance (or no top row) gives a report without components, `labels`
    all NONE, and launches nothing.
  * THE SET S.  `of=EMPTY_SPACE`: the samples with part_ids == 255; `of=SOLID`: those with part_ids != 255.  Only samples
    x < nx, y < ny, z < nz exist: the padding z in [nz, pz) of the device buffer is neither in S nor a neighbour of anything.
    Any other `of` is a ValueError.
  * CONNECTIVITY.  Two samples of S are connected when they differ by one step along one axis (6-neighbourhood); diagonal
    contact does not connect.
  * LABELS.  uint32[nx, ny, nz] in C order: the label of a sample of S is the smallest linear index (x * ny + y) * nz + z
    of any sample of its component, NONE = 0xffffffff outside S.  ValueError when the device volume nx * ny * pz (and so
    prod(dims)) exceeds 2^31 entries: the top bit of a label stays free for the device.  The label volume (4 bytes a sample)
    counts towards `max_bytes` together with the part-id volume: ValueError when 5 * nx * ny * pz > max_bytes.
  * COMPONENTS.  One `Component` per component, ordered by label; from the device, in integers: `label`, `count`, `box`
    ((lowest), (highest) index per axis), `index_sums` (the sums of x, of y and of z, uint64), `touches_border` (some sample
    has an index 0 or dims - 1 on some axis) and `parts`, a 64-bit mask given as a tuple of instance indices: for SOLID the
    owners of the component's samples, for EMPTY_SPACE the owners of the in-lattice 6-neighbours of its samples -- the parts
    that bound the void.  The host derives `volume` = count * step^3 and `centroid` = corner + step * index_sums / count in
    float64 (corner and step widened from float32 as `_instance_cells.pair_fields` widens them).
  * CAVITIES.  The EMPTY_SPACE components with touches_border == False.  The lattice of `interference()` has no margin
    around the boxes, so the outside may fall into several border components: all of them are open, none is a cavity.

The device side is csrc/instance_components.hip: a union-find over a uint32[nx, ny, pz] label volume whose entries only ever
decrease.  `local=True` labels tiles of TILE samples in LDS first and merges across the tile faces only; `local=False`
starts from label = own index and merges every pair -- the comparison arm: the same bytes, the same components.  Roots then
take a slot each of a table of `capacity` rows and every sample adds to its component's row; the counter keeps counting
past the capacity while rows beyond it are not touched, and the host then regrows the table to the count and runs the
statistics pass alone again (`component_capacity_runs` says how often it ran: 1 or 2; `initial_components` caps the first
guess).  That changes how often a pass runs, never a result.
"""
import collections

import numpy

from . import util
from . import hip_util
from .assembly_voxels import _device_volume, _dims, _cropped, _LabelMask, SOLID
from .hip_util import manager as hip_manager, check

EMPTY_SPACE = "empty_space"     # (SOLID: assembly_voxels.py)
NONE = 0xffffffff               # the label of a sample outside S
TILE = (8, 8, 16)               # the samples of a tile of the LDS stage (include/hip_util.h HU_COMPONENTS_TILE_*)
_CAPACITY = 4096                # the first guess of the table's rows
_LABEL_BYTES = 4
_ROW = numpy.dtype([("count", "<u8"), ("sums", "<u8", 3), ("parts", "<u8"), ("not_lo", "<u4", 3), ("hi", "<u4", 3),
                    ("label", "<u4"), ("flags", "<u4")])     # csrc/instance_components.hip CompRow; row 0 of a table: the counter
assert _ROW.itemsize == 72


class Component(collections.namedtuple("Component", "label count box index_sums touches_border parts volume centroid")):
    """The module's docstring defines every field."""
    __slots__ = ()


class ComponentsReport(_LabelMask, collections.namedtuple("ComponentsReport", "instances corner step dims of labels components part_ids "
                                                                  "samples_evaluated traversals component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `samples_evaluated`, `traversals`: as in AssemblyVoxels; `of`: the
    set that was labelled; `labels`: uint32[nx, ny, nz]; `components`: [Component] ordered by label;
    `component_capacity_runs`: how often the statistics pass ran (0 when nothing was launched)."""
    __slots__ = ()


class Cavity(collections.namedtuple("Cavity", Component._fields + ("enclosed_by",))):
    """A Component of empty space that does not touch the border; `enclosed_by`: the names of `parts`."""
    __slots__ = ()


class CavityReport(collections.namedtuple("CavityReport", "cavities sealed_volume components_report")):
    """`cavities`: [Cavity] ordered by label; `sealed_volume`: the sum of their volumes; `components_report`: the
    ComponentsReport of EMPTY_SPACE they were taken from."""
    __slots__ = ()


def _bits(mask):
    return tuple(k for k in range(64) if mask >> k & 1)


def _components(rows, corner, step):
    """[Component] of the table's used rows, ordered by label."""
    out = []
    cell = float(step) ** 3
    for r in rows[numpy.argsort(rows["label"], kind="stable")]:
        count = int(r["count"])
        sums = tuple(int(v) for v in r["sums"])
        lo, hi = tuple(int(v) ^ 0xffffffff for v in r["not_lo"]), tuple(int(v) for v in r["hi"])
        centroid = util.Vector(*(float(corner[k]) + float(step) * sums[k] / count for k in range(3)))
        out.append(Component(int(r["label"]), count, (lo, hi), sums, bool(int(r["flags"]) & 1), _bits(int(r["parts"])), count * cell,
                             centroid))
    return out


def _check_entries(dims):
    nx, ny, nz = (int(d) for d in dims)
    pz = -(-nz // 16) * 16
    if nx * ny * pz > 2 ** 31:
        raise ValueError("a lattice of %s samples has more than 2^31 label entries; use a coarser resolution" % [nx, ny, nz])


def assembly_components(asm, resolution, of=EMPTY_SPACE, local=True, initial_components=None, initial_capacity=None,
                        max_bytes=2 ** 32):
    """The connected components of empty space (or, `of=SOLID`, of solid) of the visible instances of the 3D assembly `asm` on
    the lattice of `interference(asm, resolution)` (the module's docstring defines them) -> ComponentsReport.

    `local=False` skips the labelling of tiles in LDS (the same result, the comparison arm).  `initial_components` caps the
    first guess of the component table, `initial_capacity` that of every cell list of the voxel traversal.  Raises
    ValueError for what assembly_voxels() refuses, for a bad `of`, for more than 2^31 label entries and for volumes of more
    than `max_bytes` bytes together."""
    if of not in (EMPTY_SPACE, SOLID):
        raise ValueError("of must be EMPTY_SPACE or SOLID, not %r" % (of,))
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=1 + _LABEL_BYTES,
                                            check_dims=_check_entries)
    shape = tuple(int(d) for d in voxels.dims)

    def report(labels, components, runs):
        return ComponentsReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, labels, components, voxels.part_ids,
                                voxels.samples_evaluated, voxels.traversals, runs)

    if volume is None:
        return report(numpy.full(shape, NONE, numpy.uint32), [], 0)
    labels, rows, runs = _label_volume(volume, shape, int(of == SOLID), local, initial_components)
    return report(labels, _components(rows, voxels.corner, voxels.step), runs)


def _label_volume(volume, shape, solid, local, initial_components):
    """The labelling from a uint8[nx, ny, pz] volume on the device on, for every caller that has one (thin_walls.py labels its
    thin ids with it): S is the samples != 255 (`solid` = 1) or == 255 of the lattice `shape` -> (labels uint32[nx, ny, nz],
    the table's used rows, how often the statistics pass ran).  `volume` is released here, as soon as no kernel reads it."""
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    check(lib.hu_components_local(volume.device_ptr, labels.device_ptr, dims, pz, solid, int(bool(local)), queue.handle),
          "hu_components_local")
    check(lib.hu_components_merge(labels.device_ptr, dims, pz, int(bool(local)), queue.handle), "hu_components_merge")
    check(lib.hu_components_flatten(labels.device_ptr, dims, pz, queue.handle), "hu_components_flatten")
    capacity = max(1, min(_CAPACITY, nx * ny * pz) if initial_components is None else int(initial_components))
    runs, count = 0, None
    while True:
        table = hip_util.Buffer(_ROW, (capacity + 1,), queue=queue)     # row 0: the counter
        check(lib.hu_memset(table.device_ptr, 0, table.size, queue.handle), "hu_memset")
        check(lib.hu_components_stats(volume.device_ptr, labels.device_ptr, dims, pz, solid, int(count is None), table.device_ptr,
                                      table.device_ptr + _ROW.itemsize, capacity, queue.handle), "hu_components_stats")
        rows = table.read()
        table.release()
        runs += 1
        if count is None:
            count = int(rows[:1].view(numpy.uint32)[0])
        if count <= capacity:
            break
        capacity = count                                               # every root was counted: the second table holds them all
    volume.release()
    check(lib.hu_components_finish(labels.device_ptr, dims, pz, queue.handle), "hu_components_finish")
    out = _cropped(labels, shape[2])
    labels.release()
    return out, rows[1:1 + count], runs


def cavities(asm, resolution, **kw):
    """The voids of `asm` that no path joins to the outside, on the lattice of `interference(asm, resolution)` -> CavityReport.
    Keywords as for assembly_components(), but `of`."""
    if "of" in kw:
        raise TypeError("cavities() labels EMPTY_SPACE")
    full = assembly_components(asm, resolution, of=EMPTY_SPACE, **kw)
    names = [i.name for i in full.instances]
    found = [Cavity(*c, enclosed_by=tuple(names[k] for k in c.parts)) for c in full.components if not c.touches_border]
    return CavityReport(found, sum(c.volume for c in found), full)
