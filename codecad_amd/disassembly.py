"""Can it be taken apart: which part blocks which along the lattice axes of the part-id volume of an assembly, how far a part
travels before it meets another, and an order in which the parts come out by straight moves.

`disassembly(asm, resolution) -> DisassemblyReport`.  Everything is defined on the index space Z^3 of the lattice of
`assembly_voxels(asm, resolution)`, in integers, exact, and independent of the order in which anything ran.

  * INSTANCES, LATTICE, PART_IDS.  Exactly those of `assembly_voxels(asm, resolution)` with `retire=True`: the same
    ValueErrors, the same bytes, n <= 64 visible instances, and an overlap sample belongs to the lower index, as everywhere.
    No visible instance (or no top row) gives the empty report (every distance NEVER) and launches nothing.
  * LINE.  For axis a in {0, 1, 2}, a line is the samples that agree on the other two indices.
  * DISTANCE.  For an ordered pair i != j and axis a,
        D_a[i][j] = min { q[a] - p[a] : ids[p] = i, ids[q] = j, p and q on one line of a, q[a] > p[a] },
    NEVER = 0xffffffff when the set is empty, and NEVER on the diagonal.  Samples of third parts, and other samples of i or j,
    between p and q change nothing: the minimum already prefers the nearer sample.  Part i moved by t steps along +e_a first
    lands on a sample of j at t = D_a[i][j]: it travels D - 1 steps freely, and D = 1 is contact.  Along -e_a the roles swap:
    the distance from i to j along -a is D_a[j][i], so three matrices serve six directions.  `distance`: uint32[3, n, n].
  * WITNESS.  Among the p that attain D_a[i][j] with some q, the lexicographically first (x, y, z).  `witness`:
    int32[3, n, n, 3], -1 where D is NEVER.  The device forms the key D << 48 | x << 32 | y << 16 | z in a uint64 and keeps
    the least key per (a, i, j); all ones means NEVER.  Indices are at most 65535 as everywhere else, so D fits its 16 bits,
    and all ones is no real key: p[a] = 65535 has nothing beyond it.  The low 48 bits follow the witness of `separation`.
  * BLOCKS.  j blocks i along (a, up) when the distance from i to j in that direction is not NEVER.  A set G of parts is FREE
    along a direction among a set R when no part of R \\ G blocks any part of G there.  FREE means one straight translation
    along a lattice axis to infinity and nothing else.
  * ORDER.  Start with R = all parts.  The directions are tried in the order +x, -x, +y, -y, +z, -z.  Repeatedly take the
    lowest index k in R for which {k} is free among R in some direction, record (k, axis, up) with the first such direction
    and remove k from R; stop when R is empty or no k qualifies.  What is left in R is `stuck`: interlocked, as far as single
    axis moves of single parts go.  The last remaining part is always free.  Deterministic by construction.

ON THE DEVICE (csrc/instance_blocking.hip).  The ids stay on the device as `assembly_voxels` left them; a uint64[3, 64, 64]
key table is set to all ones and `hu_blocking_lines` is launched once per axis, one pass over one byte per sample each: a walk
up every line that carries the last index of every part and lowers keys where a run of one id starts.  The host does not wait
between the launches, reads the table back once, and the rest is plain host code on the two arrays.
DEVICE MEMORY.  The ids, one byte a sample of the device buffer nx * ny * pz (ValueError above `max_bytes`), and the 96 KiB
of keys.
"""
import collections
import collections.abc
import math

import numpy

from . import hip_util
from .assembly_voxels import _device_volume, _whole, _axis, _dims
from .hip_util import manager as hip_manager, check

NEVER = 0xffffffff              # no sample of j lies beyond a sample of i on any line of the axis
MAX_PARTS = 64                  # include/hip_util.h HU_BLOCKING_MAX_PARTS
DIRECTIONS = tuple((axis, up) for axis in range(3) for up in (True, False))     # the order ORDER tries them in
_KEYS = (3, MAX_PARTS, MAX_PARTS)
_ONES = 0xffffffffffffffff


def _indices(parts, n, what):
    group = (parts,) if _whole(parts, 0, n - 1) else tuple(parts) if isinstance(parts, collections.abc.Iterable) and not isinstance(parts, str) else None
    if group is None or not all(_whole(k, 0, n - 1) for k in group):
        raise ValueError("%s must be indices of the %d visible instances, not %r" % (what, n, parts))
    return sorted({int(k) for k in group})


class DisassemblyReport(collections.namedtuple("DisassemblyReport", "instances corner step dims part_ids counts distance witness "
                                                                    "samples_evaluated traversals")):
    """`instances`, `corner`, `step`, `dims`, `part_ids`, `counts`, `samples_evaluated`, `traversals`: as in AssemblyVoxels;
    `distance`: uint32[3, n, n], D; `witness`: int32[3, n, n, 3], p, -1 where D is NEVER (the module's docstring)."""
    __slots__ = ()

    def steps(self, i, j, axis, up):
        """The distance from part i to part j along (axis, up) in steps of the lattice, or NEVER."""
        n = len(self.instances)
        (i,), (j,), axis = _indices(i, n, "i"), _indices(j, n, "j"), _axis(axis)
        return int(self.distance[axis, i, j] if up else self.distance[axis, j, i])

    def blockers(self, parts, axis, up, among=None):
        """The parts of `among` (default: all) outside `parts` -- an index, or an iterable: a group that moves as one -- that
        block some part of the group along (axis, up), ascending."""
        n = len(self.instances)
        group, axis = _indices(parts, n, "parts"), _axis(axis)
        rest = [k for k in (range(n) if among is None else _indices(among, n, "among")) if k not in group]
        return [j for j in rest if any(self.steps(i, j, axis, up) != NEVER for i in group)]

    def travel(self, k, axis, up, among=None):
        """How far part k moves along (axis, up) before it lands on a part of `among`, in model units: (min D - 1) * step, and
        inf when nothing blocks it."""
        if not isinstance(k, (int, numpy.integer)):
            raise ValueError("travel moves one part, not %r" % (k,))
        least = min([self.steps(k, j, axis, up) for j in self.blockers(k, axis, up, among)], default=NEVER)
        return math.inf if least == NEVER else (least - 1) * float(self.step)

    def free_directions(self, parts, among=None):
        """The (axis, up) along which nothing of `among` outside `parts` blocks the group, in the order of DIRECTIONS."""
        return [(axis, up) for axis, up in DIRECTIONS if not self.blockers(parts, axis, up, among)]

    def order(self):
        """(sequence of (k, axis, up), stuck) by the ORDER rule of the module's docstring."""
        rest, sequence = list(range(len(self.instances))), []
        while rest:
            for k in rest:
                free = self.free_directions(k, rest)
                if free:
                    sequence.append((k,) + free[0])
                    rest.remove(k)
                    break
            else:
                break
        return sequence, rest

    def contacts(self, axis):
        """The ordered pairs (i, j) with D_axis[i][j] = 1: j lies right above i somewhere."""
        return [(int(i), int(j)) for i, j in numpy.argwhere(self.distance[_axis(axis)] == 1)]


def _decode(keys, n):
    """(distance uint32[3, n, n], witness int32[3, n, n, 3]) of the key table."""
    keys = numpy.ascontiguousarray(keys[:, :n, :n])
    never = keys == numpy.uint64(_ONES)
    field = lambda shift: ((keys >> numpy.uint64(shift)) & numpy.uint64(0xffff)).astype(numpy.int64)   # noqa: E731
    distance = numpy.where(never, NEVER, field(48)).astype(numpy.uint32)
    witness = numpy.where(never[..., None], -1, numpy.stack([field(32), field(16), field(0)], axis=-1)).astype(numpy.int32)
    return distance, witness


def disassembly(asm, resolution, initial_capacity=None, max_bytes=2 ** 32):
    """Which of the visible instances of the 3D assembly `asm` blocks which along the axes of the lattice of
    `interference(asm, resolution)`, and how far away (the module's docstring defines it) -> DisassemblyReport.

    `initial_capacity` caps the first guess of every cell list of the voxel traversal.  Raises ValueError for what
    assembly_voxels() refuses and for a volume of more than `max_bytes` bytes."""
    voxels, volume = _device_volume(asm, resolution, initial_capacity, True, max_bytes, sample_bytes=1)
    n = len(voxels.instances)

    def report(distance, witness):
        return DisassemblyReport(voxels.instances, voxels.corner, voxels.step, voxels.dims, voxels.part_ids, voxels.counts, distance,
                                 witness, voxels.samples_evaluated, voxels.traversals)

    if volume is None:
        return report(numpy.full((3, n, n), NEVER, numpy.uint32), numpy.full((3, n, n, 3), -1, numpy.int32))
    lib, queue = hip_manager.lib, hip_manager.queue
    pz = volume.shape[2]
    dims = _dims(voxels.dims)
    keys = hip_util.Buffer(numpy.uint64, _KEYS, queue=queue)
    check(lib.hu_memset(keys.device_ptr, 0xff, keys.size, queue.handle), "hu_memset")
    for axis in range(3):
        check(lib.hu_blocking_lines(volume.device_ptr, keys.device_ptr, dims, pz, axis, n, queue.handle), "hu_blocking_lines")
    table = keys.read()
    for b in (volume, keys):
        b.release()
    return report(*_decode(table, n))
