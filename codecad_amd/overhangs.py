"""What a print direction leaves in the air: the overhangs of the part-id volume of an assembly along a lattice axis, the
support columns that hold them up, and where those columns stand -- on the plate, or on a part, where they leave scars.

`overhangs(asm, resolution, axis=2, up=True, reach_sq=1, of=SOLID) -> OverhangReport`.  Everything is defined on the index
space Z^3 of the lattice of `assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in which
anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)`: the same ValueErrors, the same
    `retire=True` traversal, the same bytes.  No visible instance (or no top row) gives the empty report (every id volume all
    255, no support, `first_layer` = n_a) and launches nothing.
  * THE SET S.  `of=SOLID` (the constant of `assembly_components`): the samples with part_ids != 255; `of=k`, an int, a
    visible index: the samples with part_ids == k, every other sample counting as empty -- the part printed alone, as the
    assembly owns it.  Anything else, and a k out of range, is a ValueError.  No point outside the lattice is in S, and the
    padding z in [nz, pz) of the device buffers is never read as data.
  * DIRECTION.  `axis` a is 0, 1 or 2, `up` gives s = +1 or -1, e is the unit index vector of a.  BELOW p is p - s e.  The LAYER
    of p is h(p) = p[a] if s > 0, else n_a - 1 - p[a].  h0, `first_layer`, is the least layer that holds a sample of S, n_a when
    S is empty: the build plate lies directly under it.
  * N.  The lateral offsets (u, v) on the other two axes with u^2 + v^2 <= `reach_sq`, an integer 0..8 (ValueError otherwise):
    0 lets only the sample straight below support, 1 (the default) prints a 45 degree slope along the lattice axes, 2 is the
    3 x 3 square, 4, 5 and 8 tolerate shallower slopes.
  * OVERHANG O.  A sample p of S with h(p) > h0 and p - s e + n not in S for every n in N: what a printer would lay into air.
    `overhang_ids`, uint8[nx, ny, nz] in the format of `part_ids`: part_ids on O, 255 elsewhere.
  * SUPPORT P.  A sample p inside the lattice, not in S, with h(p) >= h0, whose nearest sample of S above it on its line --
    q = p + t s e with the least t >= 1 -- lies in O: q is its HOLDER.  `support_ids` is part_ids(q) on P, 255 elsewhere.  With
    `of=k` a support passes through the samples of other parts: they count as empty.
  * LANDING L.  A sample q of S with q + s e in P: a support column stands on it.  `landing_ids`: part_ids on L, 255 elsewhere.
    `plate_landings` = |{p in P : h(p) = h0}|: the columns that stand on the plate.
  * PER PART, counted on the device in uint64, Python ints here.  `overhang_counts[k]`: the samples of O that k owns;
    `support_counts[k]`: the samples of P held for k; `landing_counts[k]`: the samples of L that k owns; `counts[k]`: as in
    AssemblyVoxels.
  * SUPPORT STRUCTURES.  `supports`: the 6-connected components of P as `Component`s of `assembly_components`, found by that
    module's kernels over `support_ids`; their `parts` are the parts they hold up.  `labels`, uint32[nx, ny, nz]: a structure's
    label at its samples, NONE elsewhere.

ONE INVARIANT.  The sample straight below an overhang o is an offset of N, so it is not in S; it lies in a layer >= h0, so it
is in P with o as its holder: every sample of O heads one COLUMN, the run of P below it, and the columns of two overhangs
are disjoint.  A column ends above a sample of S, which is then a landing and no other column's, or in layer h0, where it is
a plate landing -- never both, no sample of S lies below h0.  So |O| = |L| + plate_landings, and P and S are disjoint.

ON THE DEVICE (csrc/instance_overhang.hip).  `hu_overhang_first_layer` finds h0 into a device word (one ballot and at most
one atomic a wavefront), `hu_overhang_mark` writes `overhang_ids` and counts O (a lane per sample, lanes along z, at most 25
byte taps in the layer below with early exit), `hu_overhang_columns` walks every line of the axis from the top of the build
direction down and writes `support_ids` and `landing_ids` and the other counters: along x or y a wavefront owns 64
consecutive z of a line and carries the holder per lane, along z the line is the wavefront itself, which works on the
ballots of S and O and hands a carry from word to word.  The host does not wait between them.
DEVICE MEMORY.  While the kernels run the ids and the three id volumes are held, 4 bytes a sample of the device buffer
nx * ny * pz; the labelling afterwards holds `support_ids` and the labels, 5: the peak.  ValueError when
5 * nx * ny * pz > max_bytes, and when the label volume would have more than 2^31 entries, before anything is launched.
OUT OF SCOPE here: whether what lies below a sample is itself held, the transitive grounded-from-the-plate closure; that is
`islands()` (islands.py), whose starts are the floating overhangs of `reach_sq=0`.
"""
import collections

import numpy

from . import _instance_cells as cells
from . import hip_util
from .assembly_voxels import _device_volume, _whole, _of_code, _axis, _dims, _cropped, _LabelMask, EMPTY
from .assembly_components import SOLID, NONE, _components, _label_volume, _check_entries
from .hip_util import manager as hip_manager, check

MAX_REACH_SQ = 8                # include/hip_util.h HU_OVERHANG_MAX_REACH_SQ
SAMPLE_BYTES = 5                # support_ids and the labels: what is held per sample at the peak
_ACC = (4, 64)                  # uint64: O, P and L per part, then the plate landings and the depth word
_PLATE, _WORD = 3 * 64, 3 * 64 + 1


class OverhangReport(_LabelMask, collections.namedtuple("OverhangReport", "instances corner step dims of axis up reach_sq first_layer part_ids "
                                                              "overhang_ids support_ids landing_ids counts overhang_counts "
                                                              "support_counts landing_counts plate_landings supports labels "
                                                              "samples_evaluated traversals component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `component_capacity_runs`: as in ComponentsReport; every other field: the module's docstring."""
    __slots__ = ()

    def support_volume(self):
        """|P| * step^3: the material the supports take."""
        return sum(self.support_counts) * float(self.step) ** 3

    def overhang_area(self):
        """|O| * step^2: the area laid into air, seen along the build direction."""
        return sum(self.overhang_counts) * float(self.step) ** 2

    @property
    def self_supporting(self):
        """Nothing is laid into air: the direction prints without supports."""
        return sum(self.overhang_counts) == 0


def overhangs(asm, resolution, axis=2, up=True, reach_sq=1, of=SOLID, initial_components=None, initial_capacity=None,
              max_bytes=2 ** 32):
    """The samples of the visible instances of the 3D assembly `asm`, on the lattice of `interference(asm, resolution)`, that a
    print along lattice axis `axis` (upwards, or downwards with `up=False`) lays into air, the supports under them and where
    those stand (the module's docstring defines them) -> OverhangReport.

    `reach_sq`: the squared lateral reach, 0..8, within which a sample of the layer below supports.  `of`: SOLID, or the index
    of a visible instance.  `initial_components` caps the first guess of the support table, `initial_capacity` that of every
    cell list of the voxel traversal.  Raises ValueError for what assembly_voxels() refuses, for a bad `of`, `axis` or
    `reach_sq`, more than 2^31 label entries and for volumes of more than `max_bytes` bytes together."""
    n = len(cells.visible(asm, resolution))
    code, axis = _of_code(of, n), _axis(axis)
    if not _whole(reach_sq, 0, MAX_REACH_SQ):
        raise ValueError("reach_sq must be an integer from 0 to %d, not %r" % (MAX_REACH_SQ, reach_sq))
    up, reach_sq = bool(up), int(reach_sq)
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=SAMPLE_BYTES,
                                    check_dims=_check_entries)
    shape = tuple(int(d) for d in voxels.dims)

    def report(first, over, support, landing, totals, plate, supports, labels, runs):
        return OverhangReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, of, axis, up, reach_sq, first, voxels.part_ids,
                              over, support, landing, voxels.counts, totals[0], totals[1], totals[2], plate, supports, labels,
                              voxels.samples_evaluated, voxels.traversals, runs)

    if volume is None:
        return report(shape[axis], *(numpy.full(shape, EMPTY, numpy.uint8) for _ in range(3)), [[0] * n for _ in range(3)], 0, [],
                      numpy.full(shape, NONE, numpy.uint32), 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    dims = _dims(shape)
    acc = hip_util.Buffer(numpy.uint64, _ACC, queue=queue)
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    word = acc.device_ptr + 8 * _WORD
    over, support, landing = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(3))
    check(lib.hu_overhang_first_layer(volume.device_ptr, word, dims, pz, axis, int(up), code, queue.handle), "hu_overhang_first_layer")
    check(lib.hu_overhang_mark(volume.device_ptr, over.device_ptr, word, acc.device_ptr, dims, pz, axis, int(up), reach_sq, code,
                               queue.handle), "hu_overhang_mark")
    check(lib.hu_overhang_columns(volume.device_ptr, over.device_ptr, support.device_ptr, landing.device_ptr, word,
                                  acc.device_ptr + 8 * 64, dims, pz, axis, int(up), code, queue.handle), "hu_overhang_columns")
    overhang_ids, support_ids, landing_ids = (_cropped(b, shape[2]) for b in (over, support, landing))
    totals = acc.read()
    for b in (over, landing, volume, acc):
        b.release()
    labels, rows, runs = _label_volume(support, shape, 1, True, initial_components)
    flat = totals.ravel()
    return report(shape[axis] - (int(flat[_WORD]) & 0xffffffff), overhang_ids, support_ids, landing_ids,
                  [[int(v) for v in totals[k, :n]] for k in range(3)], int(flat[_PLATE]), _components(rows, voxels.corner, voxels.step),
                  labels, runs)
