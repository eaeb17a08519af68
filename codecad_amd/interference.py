"""Interference between the instances of an assembly: which pairs overlap, and by how much.

`interference(asm, resolution) -> InterferenceReport`.  The answer is defined on a lattice of samples, densely: sample
(i, j, k) sits at `corner + step * (float)index` per axis in float32 (kernels.hpp sample(), the lattice of
oracle.grid_eval), and it is inside instance n when the tape of that instance alone, `nodes.make_program(
instance.shape())` (its placement inside the tape), gives w < 0 there -- strictly: surfaces that touch do not
interfere.  A pair's count, index sums and index box are, bit for bit, what evaluating every instance over the whole
lattice would give.

The lattice: step = float32(resolution); the union of the visible instances' bounding boxes [a, b] is covered by
dims = ceil((b - a) / step) cells of that size per axis, and the samples are their centres, corner = a + step / 2
(rounded to float32).

It is computed sparsely, on the device, one synchronisation in all (csrc/interference.hip):
  * the lattice is cut into cubic cells of 4^k samples, each with a 64-bit mask of candidate instances; the host seeds
    the top level from the instances' bounding boxes (grown by one step) and keeps the cells with two candidates or more;
  * every coarser level evaluates each candidate at the centre of each child cell and drops it when the distance
    proves that it has no sample inside the child: w >= thr, thr = (side * step * sqrt(3) / 2) * (1 + 2^-10) for a
    child of `side` samples.  side * step * sqrt(3) / 2 is the bound k_classify uses for a cell of that size (a
    subdivision cell of side * step); the child's samples lie within (side - 1) * step * sqrt(3) / 2 of its centre,
    so the bound leaves step * sqrt(3) / 2 plus 2^-10 of itself for the rounding of the centre and of w.  Children
    with two candidates or more go on, compacted on the device;
  * the finest level (cells of 4^3 samples) evaluates every remaining candidate at every sample and adds each pair's
    samples inside both to its accumulators.
The list lengths stay on the device between levels; when a list overflowed its capacity the whole traversal is run
again with the sizes it reported.

The culling assumes what `subdivision()` assumes: every instance's distance is a lower bound on the true distance
(Lipschitz constant at most 1).  Shapes from `shapes.unsafe` may break that, and then pairs may be missed.
"""
import collections
import ctypes
import math

import numpy

from . import util
from . import nodes
from . import hip_util
from . import subdivision
from .hip_util import manager as hip_manager, check

MAX_INSTANCES = 64          # one bit each in a cell's candidate mask
_ROW = 16                   # bytes per cell row {x0 | y0 << 16, z0, mask lo, mask hi}
_TABLE_RECORD = 24          # bytes per instance of the device table (launchers.hpp InstanceRec)
_PAIR = numpy.dtype([("sums", "<u8", (4,)), ("lo", "<u4", (3,)), ("hi", "<u4", (3,)), ("pad", "<u4", (2,))])   # PairAcc
_MAX_TOP_CELLS = 1 << 15
_TAPES_PER_PART = MAX_INSTANCES            # placements of one part whose uploaded tapes are kept (_instance_tape)

Instance = collections.namedtuple("Instance", "name instance")


class Overlap(collections.namedtuple("Overlap", "i j count volume centroid index_box bounding_box index_sums")):
    """Samples inside both instances i < j: `count` of them, `volume` = count * step^3, their `centroid` (Vector), the
    min and max lattice index per axis (`index_box`, ((x, y, z), (x, y, z))), the same in world coordinates
    (`bounding_box`, the samples' positions) and the sums of their x, y, z indices (`index_sums`)."""

    __slots__ = ()


class InterferenceReport(collections.namedtuple("InterferenceReport",
                                                 "instances corner step dims pairs samples_evaluated traversals")):
    """`instances`: the visible instances in all_instances() order, as Instance(name, instance); `corner` (float32[3]),
    `step` (float32) and `dims` (int[3]): the lattice; `pairs`: an Overlap per pair with samples inside both, ordered by
    (i, j); `samples_evaluated`: per-instance sample evaluations the last traversal did, on every level; `traversals`:
    how often the traversal ran (more than once when a cell list overflowed its first capacity; 0 when no top-level
    cell had two candidates)."""

    __slots__ = ()


def lattice(instances, resolution, grow=0.0):
    """(corner float32[3], step float32, dims int64[3]) of the lattice over the union of the instances' boxes, each grown
    by `grow` on every side (in float64; clearance.py grows them by half its gap)."""
    step = numpy.float32(resolution)
    boxes = [i.shape().bounding_box() for i in instances]
    a = numpy.array([min(b.a[k] for b in boxes) for k in range(3)], dtype=numpy.float64) - grow
    b = numpy.array([max(b.b[k] for b in boxes) for k in range(3)], dtype=numpy.float64) + grow
    if not (numpy.isfinite(a).all() and numpy.isfinite(b).all()):
        raise ValueError("interference needs instances with finite bounding boxes")
    dims = numpy.maximum(1, numpy.ceil((b - a) / float(step))).astype(numpy.int64)
    corner = (a + float(step) / 2).astype(numpy.float32)
    return corner, step, dims


def _visible(asm, resolution):
    if getattr(asm, "all_instances", None) is None:
        raise ValueError("interference takes an assembly (codecad_amd.assembly)")
    if asm.dimension() != 3:
        raise ValueError("interference is implemented for 3D assemblies only")
    if not (isinstance(resolution, (int, float, numpy.floating, numpy.integer)) and math.isfinite(resolution) and resolution > 0):
        raise ValueError("resolution must be a positive finite number, not %r" % (resolution,))
    placed = [i if asm.transform == util.Transformation.zero() else i._transformed(asm.transform) for i in asm.all_instances()]
    visible = [i for i in placed if i.visible]
    if len(visible) > MAX_INSTANCES:
        raise ValueError("interference handles at most %d visible instances, the assembly has %d" % (MAX_INSTANCES, len(visible)))
    return visible


def _top_side(dims):
    side = 16
    while numpy.prod(-(-dims // side)) > _MAX_TOP_CELLS:
        side *= 4
    return side


def _windows(instances, corner, step, dims, grow=0.0):
    """int64[n, 2, 3]: per instance, the first and last lattice index per axis of its box grown by `grow` and a step,
    clipped to the lattice."""
    out = numpy.zeros((len(instances), 2, 3), dtype=numpy.int64)
    for n, inst in enumerate(instances):
        box = inst.shape().bounding_box()
        lo = numpy.floor((numpy.array(tuple(box.a)) - grow - corner - step) / step)
        hi = numpy.ceil((numpy.array(tuple(box.b)) + grow - corner + step) / step)
        out[n, 0] = numpy.clip(lo, 0, dims - 1)
        out[n, 1] = numpy.clip(hi, 0, dims - 1)
    return out


def _cell_rows(windows, dims, side):
    """Rows of the top level: cells of `side` samples that two windows or more reach."""
    n_cells = -(-dims // side)
    masks = numpy.zeros(tuple(int(n) for n in n_cells), dtype=numpy.uint64)
    for n, (lo, hi) in enumerate(windows):
        lo, hi = lo // side, hi // side
        masks[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] |= numpy.uint64(1 << n)
    bits = numpy.unpackbits(masks.view(numpy.uint8).reshape(masks.shape + (8,)), axis=-1).sum(axis=-1)
    idx = numpy.argwhere(bits >= 2)
    rows = numpy.zeros((len(idx), 4), dtype=numpy.uint32)
    if len(idx):
        m = masks[tuple(idx.T)]
        rows[:, 0] = (idx[:, 0] * side) | ((idx[:, 1] * side) << 16)
        rows[:, 1] = idx[:, 2] * side
        rows[:, 2] = (m & numpy.uint64(0xffffffff)).astype(numpy.uint32)
        rows[:, 3] = (m >> numpy.uint64(32)).astype(numpy.uint32)
    return rows


def _top_cells(instances, corner, step, dims, side):
    """Rows of the top level: cells of `side` samples that two instances' boxes (grown by a step) reach."""
    return _cell_rows(_windows(instances, corner, step, dims), dims, side)


def _instance_tape(instance):
    """The uploaded tape of a placed part, kept on the part's shape for its last _TAPES_PER_PART placements: an instance's
    shape() is a new object on every call, and compiling and uploading a tape per instance and call would cost more than
    the traversal.  (A part swept through many placements keeps no more than that many tapes on the device.)"""
    data = instance.part.data
    cache = getattr(data, "_codecad_amd_instance_tapes", None)
    if cache is None:
        cache = collections.OrderedDict()
        try:
            data._codecad_amd_instance_tapes = cache
        except AttributeError:
            pass                                  # a shape that takes no attributes: nothing is kept
    tape = cache.get(instance.transform)
    if tape is None or not tape.alive or tape.device != hip_manager.device:
        tape = cache[instance.transform] = nodes.make_program_buffer(instance.shape())
    cache.move_to_end(instance.transform)
    while len(cache) > _TAPES_PER_PART:
        cache.popitem(last=False)                 # (the tape is freed with its last reference)
    return tape


def _device_table(instances, queue):
    """(device table of the instances' uploaded tapes, distance_only, lane_bytes): hu_interference_table."""
    tapes = [_instance_tape(i) for i in instances]
    n = len(tapes)
    handles = (ctypes.c_void_p * n)(*(t.device_ptr for t in tapes))
    host_table = numpy.zeros(n * _TABLE_RECORD, dtype=numpy.uint8)
    distance_only, lane_bytes = ctypes.c_int(0), ctypes.c_uint32(0)
    check(hip_manager.lib.hu_interference_table(handles, n, host_table.ctypes.data, host_table.nbytes,
                                                ctypes.byref(distance_only), ctypes.byref(lane_bytes)), "hu_interference_table")
    table = hip_util.Buffer(numpy.uint8, (host_table.size,), queue=queue)
    table.enqueue_write(host_table)
    return table, distance_only.value, lane_bytes.value


def _levels(side, n_top, initial_capacity):
    """(sides of the cells of every level above the finest one, the first capacity of every level's child list)."""
    sides = []
    s = side
    while s > 4:
        sides.append(s)
        s //= 4
    capacities = subdivision.first_capacities([64] * len(sides), n_top=n_top, row_bytes=_ROW)
    if initial_capacity is not None:
        capacities = [subdivision.checked_capacity(min(c, max(1, int(initial_capacity)))) for c in capacities]
    return sides, capacities


def _traverse(table, n, distance_only, lane_bytes, top, sides, corner, step, dims, capacities, queue):
    """Every level enqueued back to back, ONE synchronisation -> (list counts, evaluations, pair accumulators)."""
    lib = hip_manager.lib
    n_levels = len(sides)                   # levels of cells above the finest one
    # one device buffer of everything the host reads: [list headers: 16 B per level | evaluations: 16 B | pairs]
    head = 16 * n_levels + 16
    init = numpy.zeros(head + n * n * _PAIR.itemsize, dtype=numpy.uint8)
    pairs0 = init[head:].view(_PAIR)
    pairs0["lo"] = 0xffffffff
    results = hip_util.Buffer(numpy.uint8, (init.size,), queue=queue)
    results.enqueue_write(init)
    first = numpy.zeros((len(top) + 1, 4), dtype=numpy.uint32)
    first[0, 0] = len(top)
    first[1:] = top
    parents = hip_util.Buffer(numpy.uint32, first.shape, queue=queue)
    parents.enqueue_write(first)
    buffers, max_parents = [parents], len(top)
    d = (ctypes.c_uint32 * 3)(*(int(v) for v in dims))
    c = (ctypes.c_float * 3)(*(float(v) for v in corner))
    evaluations = results.device_ptr + 16 * n_levels
    for level, (side, capacity) in enumerate(zip(sides, capacities)):
        child = side // 4
        thr = numpy.float32(child * float(step) * math.sqrt(3) / 2 * (1 + 2.0 ** -10))
        children = hip_util.Buffer(numpy.uint32, (capacity + 1, 4), queue=queue)
        check(lib.hu_memset(children.device_ptr, 0, 16, queue.handle), "hu_memset")
        check(lib.hu_interference_cells_indirect(table.device_ptr, n, distance_only, lane_bytes, parents.device_ptr + 16,
                                                 parents.device_ptr, max_parents, child, d, c, step, thr,
                                                 children.device_ptr, children.device_ptr + 16, capacity, evaluations,
                                                 queue.handle), "hu_interference_cells_indirect")
        check(lib.hu_memcpy_d2d(results.device_ptr + 16 * level, children.device_ptr, 16, queue.handle), "hu_memcpy_d2d")
        buffers.append(children)
        parents, max_parents = children, capacity
    check(lib.hu_interference_leaf_indirect(table.device_ptr, n, distance_only, lane_bytes, parents.device_ptr + 16,
                                            parents.device_ptr, max_parents, d, c, step, results.device_ptr + head,
                                            evaluations, queue.handle), "hu_interference_leaf_indirect")
    got = results.read()                    # the one synchronisation
    for b in buffers + [results]:
        b.release()
    counts = [int(v) for v in got[:16 * n_levels].view(numpy.uint32).reshape(n_levels, 4)[:, 0]]
    return counts, int(got[16 * n_levels:head].view(numpy.uint64)[0]), got[head:].view(_PAIR).reshape(n, n).copy()


def interference(asm, resolution, initial_capacity=None):
    """Pairs of visible instances of the 3D assembly `asm` that share lattice samples at `resolution` (the module's
    docstring defines the lattice, what "inside" means and what the culling assumes) -> InterferenceReport.

    Raises ValueError for a 2D assembly, more than 64 visible instances or a resolution that is not a positive finite
    number.  `initial_capacity` caps the first guess of every cell list (rows); lists that overflow are regrown, so it
    changes how often the traversal runs, never the result."""
    instances = _visible(asm, resolution)
    corner, step, dims = lattice(instances, resolution) if instances else (numpy.zeros(3, numpy.float32), numpy.float32(resolution), numpy.ones(3, numpy.int64))
    if dims[0] > 65536 or dims[1] > 65536 or dims[2] > 65536:
        raise ValueError("resolution %g gives a lattice of %s samples: at most 65536 per axis" % (resolution, dims.tolist()))
    named = [Instance(i.name, i) for i in instances]
    empty = InterferenceReport(named, corner, step, dims, [], 0, 0)
    if len(instances) < 2:
        return empty
    side = _top_side(dims)
    top = _top_cells(instances, corner, float(step), dims, side)
    if len(top) == 0:
        return empty

    queue = hip_manager.queue
    n = len(instances)
    table, distance_only, lane_bytes = _device_table(instances, queue)
    sides, capacities = _levels(side, len(top), initial_capacity)
    traversals = 0
    while True:
        traversals += 1
        counts, evaluations, acc = _traverse(table, n, distance_only, lane_bytes, top, sides, corner, step, dims,
                                             capacities, queue)
        if all(k <= c for k, c in zip(counts, capacities)):
            break
        capacities = [subdivision.checked_capacity(max(c, int(k * 1.125) + 16)) for k, c in zip(counts, capacities)]
    table.release()

    pairs = []
    cell = float(step) ** 3
    for i in range(n):
        for j in range(i + 1, n):
            a = acc[i, j]
            count = int(a["sums"][0])
            if count == 0:
                continue
            sums = tuple(int(v) for v in a["sums"][1:])
            lo, hi = tuple(int(v) for v in a["lo"]), tuple(int(v) for v in a["hi"])
            centroid = util.Vector(*(float(corner[k]) + float(step) * sums[k] / count for k in range(3)))
            box = util.BoundingBox(util.Vector(*(float(corner[k] + step * numpy.float32(lo[k])) for k in range(3))),
                                   util.Vector(*(float(corner[k] + step * numpy.float32(hi[k])) for k in range(3))))
            pairs.append(Overlap(i, j, count, count * cell, centroid, (lo, hi), box, sums))
    return InterferenceReport(named, corner, step, dims, pairs, evaluations, traversals)
