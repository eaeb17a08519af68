"""What a print starts in mid-air: the material of the part-id volume of an assembly that, at the moment its layer is laid down
along a lattice axis, is joined to the build plate by nothing that was printed before it or in the same layer -- a peg that
hangs from a ceiling, the short leg of an inverted U, a captive ball.  `overhangs()` answers a local question, whether
something lies in the layer below within a reach; a hanging peg has material under almost every one of its samples and is
still an island: its first layer starts in the air.  This is the transitive closure, grounded from the plate.

`islands(asm, resolution, axis=2, up=True, of=SOLID, local=True, initial_components=None, initial_capacity=None,
max_bytes=2**32) -> IslandReport`.  Everything is defined on the index space Z^3 of the lattice of `assembly_voxels(asm,
resolution)`, in integers, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)` with `retire=True`: the same
    ValueErrors, the same bytes, n <= 64 visible instances.  No visible instance (or no top row) gives the empty report and
    launches nothing.  The padding z in [nz, pz) of the device buffers is never read as data.
  * THE SET S.  As in `overhangs()`.  `of=SOLID`: the samples with part_ids != 255, the assembly printed in place as one solid;
    `of=k`, a visible index: the samples with part_ids == k, everything else counting as empty.  Anything else is a ValueError.
  * DIRECTION.  `axis` a is 0, 1 or 2, `up` gives s = +1 or -1, e is the unit index vector of a: as in `overhangs()` and
    `drainage()`.  BELOW p is p - s e, ABOVE p is p + s e.  The LAYER of p is h(p) = p[a] if s > 0, else n_a - 1 - p[a].  The
    LATERAL axes are the other two.  h0, `first_layer`, is the least layer that holds a sample of S, n_a when S is empty: the
    plate lies directly under it, as in `overhangs()`.
  * GROUNDED G.  The least subset of S that holds every p of S with h(p) = h0, and every p of S whose sample below, or one of
    whose in-lattice lateral neighbours, is in G.  Nothing is handed downwards; the lattice's sides and top ground nothing.
  * FLOATING F = S \\ G.  F holds nothing in layer h0; the sample below a floating sample is in F or outside S; a floating
    sample's lateral neighbours are in F or outside S; F and G touch only where a sample of G lies directly ABOVE a sample of F.
  * STARTS A = {p in F : p - s e not in S}: the undersides where a support would have to reach.  A = F & O, with O the
    overhangs of `overhangs(..., reach_sq=0, of=of)`, and every 6-connected component of F holds at least one start.
  * JOINS J = {p in F : p + s e in G}: here an island is finally held, from above.
  * VOLUMES, uint8[nx, ny, nz] in the format of `part_ids`: `floating_ids`, `start_ids`, `join_ids`, each part_ids on its set
    and 255 elsewhere; `render_assembly_voxel_layers` shows them as they are.
  * COUNTS, on the device in uint64, Python ints here: `floating_counts[k]`, `start_counts[k]`, `join_counts[k]`, the samples
    of each set that part k owns; `floating_volume` = sum(floating_counts) * step^3.
  * ISLANDS.  The 6-connected components of floating_ids != 255 as `Island`s, `Component`s of `assembly_components` found by
    that module's kernels over `floating_ids`, as `drainage` finds its pools.  The host adds `owners`, the names of the parts;
    `first_layer`, the lowest layer of its box; `starts`, the number of start samples in it; and `loose`: no sample of J
    carries its label -- such an island is never joined to anything grounded: a separate body, such as a captive ball or a part
    that touches nothing below.  `labels`, uint32[nx, ny, nz]: an island's label at its samples, NONE elsewhere.
  * PASSES.  `passes`: how often the rise ran, 1 <= passes <= n_a + 1 (0 when nothing was launched); it depends on the
    scheduling, no other field does.  `grounded`: nothing floats.

OUT OF SCOPE.  A lateral reach, so handing on across a diagonal: the 6-neighbourhood only, and two boxes that meet only along
an edge do not ground each other; grounding through the supports of `overhangs()`; directions off the lattice axes; more than
64 instances; several devices.

ON THE DEVICE (csrc/instance_reach.hip, driven by _layer_reach.py, both shared with `drainage()`), monotone reachability:
connected within a layer, handed on from layer to layer in one direction only.  `hu_overhang_first_layer` raises a device word
to n_a - h0; `hu_ground_layers` labels the layers' components of S, all layers at once, by the union-find of
`assembly_components` with the edges of the two lateral axes alone (`local=True` labels tiles in LDS first, `local=False` is
the comparison arm: the same bytes); `hu_components_flatten` makes every entry its root; `hu_ground_seed` reads the word on
the device and sets bit 31 of the root's entry for every sample of layer h0; `hu_drain_rise`, unchanged, is one PASS up every
line of the axis that hands the flags on from a layer to the next, and the host repeats it until a pass sets no flag, reading
one word a pass; `hu_ground_mark` walks the lines once more and writes `floating_ids`, `start_ids` and `join_ids` -- every
in-lattice byte once: nothing is preset -- and the counters.  Between the launches the host waits only for that word.
DEVICE MEMORY.  While the kernels run the ids, the labels and the three id volumes are held, 8 bytes a sample of the device
buffer nx * ny * pz: the peak; the labelling of the islands afterwards holds the floating ids and its labels, 5.  ValueError
when 8 * nx * ny * pz > max_bytes, when the label volume would have more than 2^31 entries, and when it has exactly 2^31
with `up=False` (the flag of the last entry would be lost), before anything is launched.
"""
import collections

import numpy

from . import _instance_cells as cells
from . import hip_util
from .assembly_voxels import _device_volume, _of_code, _axis, _dims, _cropped, _LabelMask, EMPTY
from .assembly_components import Component, SOLID, NONE, _components, _label_volume, _check_entries
from .hip_util import manager as hip_manager, check
from ._layer_reach import flagged_layers, box_layers

SAMPLE_BYTES = 8                # the ids, the labels and the three id volumes: what is held per sample at the peak
_ACC = (4, 64)                  # uint64: F, A and J per part, then the depth word of hu_overhang_first_layer
_DEPTH = 8 * 3 * 64             # its byte offset


class Island(collections.namedtuple("Island", Component._fields + ("owners", "first_layer", "starts", "loose"))):
    """A Component of the floating samples; `parts`: the parts that own them, `owners`: their names, `first_layer`: the lowest
    layer of its box, `starts`: its start samples, `loose`: no sample of it lies under a grounded one."""
    __slots__ = ()


class IslandReport(_LabelMask, collections.namedtuple("IslandReport", "instances corner step dims of axis up first_layer part_ids "
                                                      "floating_ids start_ids join_ids floating_counts start_counts join_counts "
                                                      "floating_volume islands labels passes samples_evaluated traversals "
                                                      "component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `component_capacity_runs`: as in ComponentsReport; every other field: the module's docstring."""
    __slots__ = ()

    @property
    def grounded(self):
        """Nothing floats: every layer of the print starts on the plate or on what was printed before."""
        return sum(self.floating_counts) == 0


def _islands(rows, voxels, axis, up, labels, start_ids, join_ids):
    found = _components(rows, voxels.corner, voxels.step)
    names = [i.name for i in voxels.instances]
    na = int(voxels.dims[axis])
    order = numpy.array([c.label for c in found], dtype=numpy.uint32)             # ascending: _components sorts by label
    starts = numpy.bincount(numpy.searchsorted(order, labels[start_ids != EMPTY]), minlength=len(found))
    joined = set(numpy.unique(labels[join_ids != EMPTY]).tolist())
    return [Island(*c, owners=tuple(names[k] for k in c.parts), first_layer=box_layers(c.box, na, axis, up)[0],
                   starts=int(starts[k]), loose=c.label not in joined) for k, c in enumerate(found)]


def _check_flag(dims, up):
    nx, ny, nz = (int(d) for d in dims)
    if not up and nx * ny * (-(-nz // 16) * 16) == 2 ** 31:
        raise ValueError("a lattice of %s samples has exactly 2^31 label entries, which islands() takes with up=True only; use "
                         "another resolution" % [nx, ny, nz])


def islands(asm, resolution, axis=2, up=True, of=SOLID, local=True, initial_components=None, initial_capacity=None,
            max_bytes=2 ** 32):
    """The samples of the visible instances of the 3D assembly `asm`, on the lattice of `interference(asm, resolution)`, that a
    print along lattice axis `axis` (upwards, or downwards with `up=False`) starts in mid-air: the floating samples, where they
    start, where they are finally joined from above and the islands they form (the module's docstring defines them) ->
    IslandReport.

    `of`: SOLID, or the index of a visible instance.  `local=False` skips the labelling of tiles in LDS, in the layers and in the
    islands (the same result, the comparison arm).  `initial_components` caps the first guess of the island table,
    `initial_capacity` that of every cell list of the voxel traversal.  Raises ValueError for what assembly_voxels() refuses,
    for a bad `of` or `axis`, more than 2^31 label entries and for volumes of more than `max_bytes` bytes together."""
    n = len(cells.visible(asm, resolution))
    code, axis, up = _of_code(of, n), _axis(axis), bool(up)

    def check_dims(dims):
        _check_entries(dims)
        _check_flag(dims, up)

    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES,
                                    check_dims=check_dims)
    shape = tuple(int(d) for d in voxels.dims)

    def report(first, floating_ids, start_ids, join_ids, totals, found, labels, passes, runs):
        return IslandReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, axis, up, first, voxels.part_ids,
                            floating_ids, start_ids, join_ids, totals[0], totals[1], totals[2],
                            sum(totals[0]) * float(voxels.step) ** 3, found, labels, passes, voxels.samples_evaluated,
                            voxels.traversals, runs)

    if volume is None:
        return report(shape[axis], *(numpy.full(shape, EMPTY, numpy.uint8) for _ in range(3)), [[0] * n for _ in range(3)], [],
                      numpy.full(shape, NONE, numpy.uint32), 0, 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)

    def label(acc, layers):                                               # the depth word lies behind the counters
        check(lib.hu_overhang_first_layer(volume.device_ptr, acc.device_ptr + _DEPTH, dims, pz, axis, int(up), code, queue.handle),
              "hu_overhang_first_layer")
        check(lib.hu_ground_layers(volume.device_ptr, layers.device_ptr, dims, pz, axis, code, int(bool(local)), queue.handle),
              "hu_ground_layers")

    def seed(acc, layers):
        check(lib.hu_ground_seed(layers.device_ptr, acc.device_ptr + _DEPTH, dims, pz, axis, int(up), queue.handle), "hu_ground_seed")

    acc, word, layers, passes = flagged_layers(hip_manager, volume, dims, axis, up, _ACC, label, seed)
    floating, start, join = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(3))
    check(lib.hu_ground_mark(volume.device_ptr, layers.device_ptr, floating.device_ptr, start.device_ptr, join.device_ptr,
                             acc.device_ptr, dims, pz, axis, int(up), code, queue.handle), "hu_ground_mark")
    floating_ids, start_ids, join_ids = (_cropped(b, shape[2]) for b in (floating, start, join))
    totals = acc.read()
    for b in (layers, volume, start, join, acc, word):
        b.release()
    labels, rows, runs = _label_volume(floating, shape, 1, local, initial_components)
    first = shape[axis] - (int(totals[3, 0]) & 0xffffffff)
    return report(first, floating_ids, start_ids, join_ids, [[int(v) for v in totals[k, :n]] for k in range(3)],
                  _islands(rows, voxels, axis, up, labels, start_ids, join_ids), labels, passes, runs)
