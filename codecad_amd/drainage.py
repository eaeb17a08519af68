"""What an assembly holds when it is drained along a lattice axis: the pools of the part-id volume that stay behind when liquid
or powder runs out downwards and sideways -- a cup, a blind hole that faces up, a U-bend, the pocket between two mated parts.
`cavities()` finds the voids that no path joins to the outside; these are open to it, and hold in one orientation and not in
another.

`drainage(asm, resolution, axis=2, up=True) -> DrainageReport`.  Everything is defined on the index space Z^3 of the lattice of
`assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)` with `retire=True`: the same
    ValueErrors, the same bytes, n <= 64 visible instances.  S is the solid, part_ids != 255; E is the empty samples of the
    lattice.  Nothing outside the lattice is solid: THE OUTSIDE IS A SINK.  No visible instance (or no top row) gives the empty
    report and launches nothing.  The padding z in [nz, pz) of the device buffers is never read as data.
  * DIRECTION.  `axis` a is 0, 1 or 2, `up` gives s = +1 or -1, e is the unit index vector of a: as in `overhangs()`.  Up is s e,
    liquid falls along -s e, BELOW p is p - s e.  The LAYER of p is h(p) = p[a] if s > 0, else n_a - 1 - p[a].  The LATERAL axes
    are the other two.
  * ESCAPE.  A sample p of E ESCAPES when a path leads from it out of the lattice through samples of E, each step going to a
    6-neighbour and none of them upwards; it leaves the lattice by a lateral step or a downward one: THE TOP FACE IS NO EXIT.
    Equivalently X, the samples that escape, is the least set such that p in E is in X when it lies in layer 0, when it has a
    lateral index of 0 or n - 1, and when the sample below it or a lateral neighbour of it is in X.
  * TRAPPED.  T = E \\ X: the pools, filled to the level at which they spill.  T and S are disjoint; the sample below a trapped
    sample, and every in-lattice lateral neighbour of it, is solid or trapped; every sample of a cavity of `cavities()` is
    trapped, in all six directions.
  * FLOOR.  The nearest sample of S below a trapped sample on its line.  Every trapped sample has one: with no solid below on
    its line the straight way down leaves the lattice, and the sample escapes.  `trapped_ids`, uint8[nx, ny, nz] in the format
    of `part_ids`: the id of the floor on T, 255 elsewhere.  `trapped_counts[k]`: the trapped samples whose floor is part k,
    counted on the device in uint64, Python ints here; `trapped_volume` = sum(trapped_counts) * step^3.
  * POOLS.  The 6-connected components of trapped_ids != 255 as `Pool`s, `Component`s of `assembly_components` found by that
    module's kernels over `trapped_ids`: their `parts` are the floors the pool stands on.  The host adds `held_by`, the parts'
    names, and `level`, the highest layer of the pool's box: the layer of its surface.  `labels`, uint32[nx, ny, nz]: a pool's
    label at its samples, NONE elsewhere.
  * PASSES.  `passes`: how often the rise ran, 1 <= passes <= n_a + 1 (0 when nothing was launched); it depends on the
    scheduling, no other field does.

`render_assembly_voxel_layers` shows `trapped_ids`: it has the format of `part_ids`.

OUT OF SCOPE.  Directions off the lattice axes; partial fill levels; drain holes sized by a ball (the transform of `thin_walls`
on empty space); the transitive grounded-from-the-plate closure of the SOLID, the dual problem and the next caller of the first
three stages (`islands()`, islands.py, is that caller); whether a pool is a sealed cavity (DESIGN.md section 9.2 says what that would cost; compare `labels` with those
of `cavities()`); more than 64 instances; several devices.

ON THE DEVICE (csrc/instance_reach.hip, driven by _layer_reach.py, both shared with `islands()`), monotone reachability:
connected within a layer, handed on from layer to layer in one direction only.  `hu_drain_layers` labels the layers' components of E, all layers at once, by the union-find of
`assembly_components` with the edges of the two lateral axes alone (`local=True` labels tiles in LDS first, `local=False` is
the comparison arm: the same bytes); `hu_components_flatten` makes every entry its root; `hu_drain_seed` sets bit 31 of a
root's entry, its ESCAPE FLAG, for every sample in layer 0 or at a lateral border; `hu_drain_rise` is one PASS up every line
of the axis that hands the flags on from a layer to the next, and the host repeats it until a pass sets no flag, reading one
word a pass; `hu_drain_floor` walks the lines once more and writes `trapped_ids` -- every in-lattice byte: nothing is preset --
and the counters.  Between the launches the host waits only for that word.
DEVICE MEMORY.  While the kernels run the ids, the labels and the trapped ids are held, 6 bytes a sample of the device buffer
nx * ny * pz: the peak; the labelling of the pools afterwards holds the trapped ids and its labels, 5.  ValueError when
6 * nx * ny * pz > max_bytes, and when the label volume would have more than 2^31 entries, before anything is launched.
"""
import collections

import numpy

from . import hip_util
from .assembly_voxels import _device_volume, _axis, _dims, _cropped, _LabelMask, EMPTY
from .assembly_components import Component, NONE, _components, _label_volume, _check_entries
from .hip_util import manager as hip_manager, check
from ._layer_reach import flagged_layers, box_layers

SAMPLE_BYTES = 6                # the ids, the labels and the trapped ids: what is held per sample at the peak
_COUNTS = (64,)                 # uint64: the trapped samples per floor


class Pool(collections.namedtuple("Pool", Component._fields + ("held_by", "level"))):
    """A Component of the trapped samples; `parts`: the floors it stands on, `held_by`: their names, `level`: the highest layer
    of its box."""
    __slots__ = ()


class DrainageReport(_LabelMask, collections.namedtuple("DrainageReport", "instances corner step dims axis up part_ids trapped_ids "
                                                        "trapped_counts trapped_volume pools labels passes samples_evaluated "
                                                        "traversals component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `component_capacity_runs`: as in ComponentsReport; every other field: the module's docstring."""
    __slots__ = ()

    @property
    def drains(self):
        """Nothing is trapped: this way up the assembly holds nothing."""
        return sum(self.trapped_counts) == 0


def _pools(rows, voxels, axis, up):
    names = [i.name for i in voxels.instances]
    na = int(voxels.dims[axis])
    return [Pool(*c, held_by=tuple(names[k] for k in c.parts), level=box_layers(c.box, na, axis, up)[1])
            for c in _components(rows, voxels.corner, voxels.step)]


def drainage(asm, resolution, axis=2, up=True, local=True, initial_components=None, initial_capacity=None, max_bytes=2 ** 32):
    """What the visible instances of the 3D assembly `asm` hold on the lattice of `interference(asm, resolution)` when they are
    drained with lattice axis `axis` pointing up (or down, with `up=False`): the trapped samples, their floors and the pools
    they form (the module's docstring defines them) -> DrainageReport.

    `local=False` skips the labelling of tiles in LDS, in the layers and in the pools (the same result, the comparison arm).
    `initial_components` caps the first guess of the pool table, `initial_capacity` that of every cell list of the voxel
    traversal.  Raises ValueError for what assembly_voxels() refuses, for a bad `axis`, more than 2^31 label entries and for
    volumes of more than `max_bytes` bytes together."""
    axis, up = _axis(axis), bool(up)
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES,
                                    check_dims=_check_entries)
    n = len(voxels.instances)
    shape = tuple(int(d) for d in voxels.dims)

    def report(trapped_ids, counts, pools, labels, passes, runs):
        return DrainageReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, axis, up, voxels.part_ids, trapped_ids, counts,
                              sum(counts) * float(voxels.step) ** 3, pools, labels, passes, voxels.samples_evaluated,
                              voxels.traversals, runs)

    if volume is None:
        return report(numpy.full(shape, EMPTY, numpy.uint8), [0] * n, [], numpy.full(shape, NONE, numpy.uint32), 0, 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)

    def label(acc, layers):
        check(lib.hu_drain_layers(volume.device_ptr, layers.device_ptr, dims, pz, axis, int(bool(local)), queue.handle), "hu_drain_layers")

    def seed(acc, layers):
        check(lib.hu_drain_seed(layers.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_drain_seed")

    acc, word, layers, passes = flagged_layers(hip_manager, volume, dims, axis, up, _COUNTS, label, seed)
    trapped = hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue)
    check(lib.hu_drain_floor(volume.device_ptr, layers.device_ptr, trapped.device_ptr, acc.device_ptr, dims, pz, axis, int(up),
                             queue.handle), "hu_drain_floor")
    trapped_ids = _cropped(trapped, shape[2])
    totals = acc.read()
    for b in (layers, volume, acc, word):
        b.release()
    labels, rows, runs = _label_volume(trapped, shape, 1, local, initial_components)
    return report(trapped_ids, [int(v) for v in totals[:n]], _pools(rows, voxels, axis, up), labels, passes, runs)
