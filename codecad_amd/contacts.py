"""Which parts touch: over how many faces of the part-id volume of an assembly, where, facing which way and in what patches --
where a fastener goes, how much area a glue or weld line has, what a thermal or electrical path crosses, and which part hangs
in the air because a transform was mistyped.

`contacts(asm, resolution, patches=True) -> ContactReport`.  Everything is defined on the index space Z^3 of the lattice of
`assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)` with `retire=True`: the same
    ValueErrors, the same bytes, n <= 64 visible instances, and an overlap sample belongs to the lower index, as everywhere.
    No visible instance (or no top row) gives the empty report and launches nothing.  Nothing outside the lattice is inside any
    part, and the padding z in [nz, pz) of the device buffers is never read as data.
  * FACE.  For axis a in {0, 1, 2} and sample p, the face between p and p + e_a, e_a the unit index vector of a.  It counts for
    a pair only when both samples are in the lattice.
  * CONTACT.  For an ordered pair i != j of parts and axis a,
        C_a[i][j] = { p : ids[p] = i, ids[p + e_a] = j }:
    j lies right above i there.  Per (a, i, j), all from the device: `faces`, uint64[3, n, n], |C_a[i][j]|; `index_sums`,
    uint64[3, n, n, 3], the sums of p; `box`, int32[3, n, n, 2, 3], the lowest and the highest p per axis, -1 where C is empty;
    `witness`, int32[3, n, n, 3], the lexicographically first p, -1 where C is empty -- the witness rule of `disassembly`.  The
    diagonal is empty by definition.
  * EXPOSED.  `exposed`, uint64[3, 2, n]: [a, 0, i] is the number of p with ids[p] = i and p + e_a empty or outside the lattice,
    [a, 1, i] the same with p - e_a: the faces of i that face nothing.
  * INTERFACE SAMPLES.  A sample p with ids[p] = i != 255 and some in-lattice 6-neighbour q with ids[q] not in {i, 255}.
    `contact_ids`, uint8[nx, ny, nz] in the format of `part_ids`: ids[p] on the interface samples, 255 elsewhere;
    `contact_counts[i]`: the interface samples i owns, counted on the device in uint64, Python ints here.
  * PATCHES (`patches=True`).  The 6-connected components of contact_ids != 255 as `Component`s of `assembly_components`, found
    by that module's kernels over `contact_ids`; their `parts` are the parts that meet there.  `labels`, uint32[nx, ny, nz]: a
    patch's label at its samples, NONE elsewhere.  A PATCH IS TWO SAMPLES THICK, one layer of each side, and it may hold more
    than two parts: where three parts meet along an edge, and where two interfaces adjoin, their samples are 6-connected and
    form one patch.  A patch is not split per pair.  With `patches=False` nothing is labelled: `patches` = [], `labels` all NONE,
    `component_capacity_runs` = 0.

ONE INVARIANT.  For every axis a and part i,
    exposed[a, 0, i] + sum_j faces[a, i, j] = exposed[a, 1, i] + sum_j faces[a, j, i]:
both sides count the maximal runs of i along the lines of a, the left one by their upper ends, the right one by their lower.

RELATION TO `disassembly`.  faces[a, i, j] > 0 exactly when `disassembly(...).distance[a, i, j] == 1`, and `witness[a, i, j]` is
then equal in the two reports.

AREAS ARE STAIRCASE AREAS.  A face has the area step^2, and every area here is a number of faces times step^2: exact for an
interface normal to a lattice axis, an overestimate by up to sqrt(3) for an inclined one (a plane with the unit normal n shows
|n_x| + |n_y| + |n_z| times its area in faces).  `normal(i, j)` says how a contact is inclined.

OUT OF SCOPE.  True (non-staircase) areas; contact within a tolerance (that is `clearance`); contact across edges or corners
(26 neighbours); more than 64 instances; 2D assemblies; splitting a patch per pair.

ON THE DEVICE (csrc/instance_contacts.hip).  The ids stay on the device as `assembly_voxels` left them.  A table of 3 x 64 x 64
rows of 64 bytes and a table of 7 x 64 counters are set to zero, one `hu_memset` each, and `hu_contact_faces` is launched
once: one pass in which a lane holds its sample's id and its six neighbours', and a wavefront writes a row out only when the
pair it meets changes.  The host reads the two tables back once, releases the ids and hands the contact volume to the
labelling of `assembly_components`; it does not wait between the launches.
DEVICE MEMORY.  While the kernel runs the ids and the contact ids are held, 2 bytes a sample of the device buffer nx * ny * pz;
the labelling afterwards holds the contact ids and the labels, 5: the peak.  ValueError when 5 * nx * ny * pz > max_bytes (2
with `patches=False`), and with patches when the label volume would have more than 2^31 entries, before anything is launched.
"""
import collections

import numpy

from . import util
from . import hip_util
from .assembly_voxels import _device_volume, _axis, _dims, _cropped, _LabelMask, EMPTY
from .assembly_components import NONE, _components, _label_volume, _check_entries
from .disassembly import _indices
from .hip_util import manager as hip_manager, check

MAX_PARTS = 64                  # include/hip_util.h HU_CONTACT_MAX_PARTS
SAMPLE_BYTES = 5                # the contact ids and the labels: what is held per sample at the peak; without patches:
SAMPLE_BYTES_NO_PATCHES = 2     # the ids and the contact ids
_ROW = numpy.dtype([("count", "<u8"), ("sums", "<u8", 3), ("not_key", "<u8"), ("not_lo", "<u4", 3), ("hi", "<u4", 3)])
assert _ROW.itemsize == 64      # include/hip_util.h hu_contact_row
_ROWS = (3, MAX_PARTS, MAX_PARTS)
_COUNTS = (7, 64)               # uint64: exposed [a][0] and [a][1] per axis a, then the interface samples


class ContactReport(_LabelMask, collections.namedtuple("ContactReport", "instances corner step dims part_ids counts faces index_sums box "
                                                       "witness exposed contact_ids contact_counts patches labels "
                                                       "samples_evaluated traversals component_capacity_runs")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `component_capacity_runs`: as in ComponentsReport; every other field: the module's docstring.  Every area is a staircase
    area (the module's docstring): a number of faces times step^2."""
    __slots__ = ()

    def _pair(self, i, j):
        n = len(self.instances)
        (i,), (j,) = _indices(i, n, "i"), _indices(j, n, "j")
        return i, j

    def _faces(self, i, j, axis):
        return int(self.faces[axis, i, j]) + int(self.faces[axis, j, i])

    def area(self, i, j):
        """The contact area of parts i and j: their faces on every axis and in both orders, times step^2."""
        i, j = self._pair(i, j)
        return sum(self._faces(i, j, axis) for axis in range(3)) * float(self.step) ** 2

    def projected_area(self, i, j, axis):
        """The contact area of the pair on the faces of `axis` alone: what the contact shows seen along that axis."""
        (i, j), axis = self._pair(i, j), _axis(axis)
        return self._faces(i, j, axis) * float(self.step) ** 2

    def normal(self, i, j):
        """The three signed face counts faces[a, i, j] - faces[a, j, i]: positive on axis a where j lies above i."""
        i, j = self._pair(i, j)
        return tuple(int(self.faces[axis, i, j]) - int(self.faces[axis, j, i]) for axis in range(3))

    def centroid(self, i, j):
        """The mean face centre of the pair over both orders and all axes, in model units -- a face of axis a at p has its
        centre at corner + step * (p + e_a / 2) --, or None when the two do not touch."""
        i, j = self._pair(i, j)
        total = sum(self._faces(i, j, axis) for axis in range(3))
        if total == 0:
            return None
        # twice the sum of the centres, in integers: 2 p + e_a per face
        twice = [sum(2 * (int(self.index_sums[axis, i, j, k]) + int(self.index_sums[axis, j, i, k])) for axis in range(3))
                 + self._faces(i, j, k) for k in range(3)]
        return util.Vector(*(float(self.corner[k]) + float(self.step) * twice[k] / (2 * total) for k in range(3)))

    def touching(self, i):
        """The parts that touch part i, ascending."""
        n = len(self.instances)
        (i,) = _indices(i, n, "i")
        return [j for j in range(n) if j != i and any(self._faces(i, j, axis) for axis in range(3))]

    def pairs(self):
        """The pairs (i, j), i < j, with any face, ascending."""
        n = len(self.instances)
        return [(i, j) for i in range(n) for j in self.touching(i) if i < j]

    def groups(self):
        """The connected sets of the graph whose edges are `pairs()`, each sorted, ordered by their least member."""
        n = len(self.instances)
        seen, out = set(), []
        for start in range(n):
            if start in seen:
                continue
            group, todo = {start}, [start]
            while todo:
                for j in self.touching(todo.pop()):
                    if j not in group:
                        group.add(j)
                        todo.append(j)
            seen |= group
            out.append(sorted(group))
        return out

    def loose(self):
        """The parts that touch nothing, ascending."""
        return [i for i in range(len(self.instances)) if not self.touching(i)]

    def _exposed(self, i):
        return sum(int(v) for v in self.exposed[:, :, i].ravel())

    def exposed_area(self, i):
        """The faces of part i that face nothing, times step^2."""
        (i,) = _indices(i, len(self.instances), "i")
        return self._exposed(i) * float(self.step) ** 2

    def surface_area(self, i):
        """The exposed and the contact faces of part i, times step^2."""
        n = len(self.instances)
        (i,) = _indices(i, n, "i")
        touched = sum(self._faces(i, j, axis) for j in range(n) if j != i for axis in range(3))
        return (self._exposed(i) + touched) * float(self.step) ** 2


def _decode(rows, n):
    """(faces, index_sums, box, witness) of the row table."""
    rows = numpy.ascontiguousarray(rows[:, :n, :n])
    faces = rows["count"].astype(numpy.uint64)
    empty = faces == 0
    sums = numpy.ascontiguousarray(rows["sums"]).astype(numpy.uint64)
    lo = (rows["not_lo"] ^ numpy.uint32(0xffffffff)).astype(numpy.int64)
    box = numpy.where(empty[..., None, None], -1, numpy.stack([lo, rows["hi"].astype(numpy.int64)], axis=-2)).astype(numpy.int32)
    key = ~rows["not_key"]
    field = lambda shift: ((key >> numpy.uint64(shift)) & numpy.uint64(0xffff)).astype(numpy.int64)   # noqa: E731
    witness = numpy.where(empty[..., None], -1, numpy.stack([field(32), field(16), field(0)], axis=-1)).astype(numpy.int32)
    return faces, sums, box, witness


def contacts(asm, resolution, patches=True, local=True, initial_components=None, initial_capacity=None, max_bytes=2 ** 32):
    """Which of the visible instances of the 3D assembly `asm` touch on the lattice of `interference(asm, resolution)`, over how
    many faces, where, and in what patches (the module's docstring defines them) -> ContactReport.

    `patches=False` skips the labelling of the contact patches.  `local=False` skips the labelling of tiles in LDS (the same
    result, the comparison arm of assembly_components()), `initial_components` caps the first guess of the patch table,
    `initial_capacity` that of every cell list of the voxel traversal.  Raises ValueError for what assembly_voxels() refuses, with
    patches for more than 2^31 label entries, and for volumes of more than `max_bytes` bytes together."""
    patches = bool(patches)
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes,
                                    sample_bytes=SAMPLE_BYTES if patches else SAMPLE_BYTES_NO_PATCHES,
                                    check_dims=_check_entries if patches else None)
    n = len(voxels.instances)
    shape = tuple(int(d) for d in voxels.dims)

    def report(faces, sums, box, witness, exposed, contact_ids, contact_counts, found, labels, runs):
        return ContactReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, voxels.part_ids, voxels.counts, faces, sums, box,
                             witness, exposed, contact_ids, contact_counts, found, labels, voxels.samples_evaluated, voxels.traversals,
                             runs)

    if volume is None:
        return report(*_decode(numpy.zeros(_ROWS, _ROW), n), numpy.zeros((3, 2, n), numpy.uint64), numpy.full(shape, EMPTY, numpy.uint8),
                      [0] * n, [], numpy.full(shape, NONE, numpy.uint32), 0)
    lib, queue = hip_manager.lib, hip_manager.queue
    nx, ny, pz = volume.shape
    rows = hip_util.Buffer(_ROW, _ROWS, queue=queue)
    check(lib.hu_memset(rows.device_ptr, 0, rows.size, queue.handle), "hu_memset")
    acc = hip_util.Buffer(numpy.uint64, _COUNTS, queue=queue)
    check(lib.hu_memset(acc.device_ptr, 0, acc.size, queue.handle), "hu_memset")
    contact = hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue)
    check(lib.hu_contact_faces(volume.device_ptr, contact.device_ptr, rows.device_ptr, acc.device_ptr, _dims(shape), pz, n, queue.handle),
          "hu_contact_faces")
    table, totals = rows.read(), acc.read()
    contact_ids = _cropped(contact, shape[2])
    for b in (volume, rows, acc):
        b.release()
    if patches:
        labels, found, runs = _label_volume(contact, shape, 1, local, initial_components)
        found = _components(found, voxels.corner, voxels.step)
    else:
        contact.release()
        labels, found, runs = numpy.full(shape, NONE, numpy.uint32), [], 0
    exposed = numpy.ascontiguousarray(totals[:6, :n].reshape(3, 2, n)).astype(numpy.uint64)
    return report(*_decode(table, n), exposed, contact_ids, [int(v) for v in totals[6, :n]], found, labels, runs)
