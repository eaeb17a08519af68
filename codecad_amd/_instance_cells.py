"""The traversal under `interference` and `clearance` (interference.py, clearance.py define what each computes): a lattice
over the visible instances of an assembly, cut into cubic cells of 4^k samples with a 64-bit mask of candidate
instances each; a device table of the instances' tapes; cell lists the device counts; one synchronisation at the
end; the whole traversal again, with the sizes it reported, when a list overflowed (csrc/instance_pairs.hip).

A check says what differs: the dtype of a pair's accumulators and their initial values, the threshold of a level, the
windows (clearance only) and the entry points of the coarser levels and of the finest one.
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
from .hip_util._lib import CellsLaunch, CellsChildren

MAX_INSTANCES = 64          # one bit each in a cell's candidate mask
_ROW = 16                   # bytes per cell row {x0 | y0 << 16, z0, mask lo, mask hi}
_TABLE_RECORD = 24          # bytes per instance of the device table (instance_args.hpp InstanceRec)
_MAX_TOP_CELLS = 1 << 15
_TAPES_PER_PART = MAX_INSTANCES            # placements of one part whose uploaded tapes are kept (instance_tape)

Instance = collections.namedtuple("Instance", "name instance")
# the fields every pair has (interference.Overlap; clearance.NearMiss adds its own)
PairFields = collections.namedtuple("PairFields", "i j count volume centroid index_box bounding_box index_sums")


def lattice(instances, resolution, grow=0.0):
    """(corner float32[3], step float32, dims int64[3]) of the lattice over the union of the instances' boxes, each grown
    by `grow` on every side (in float64; clearance grows them by half its gap)."""
    step = numpy.float32(resolution)
    boxes = [i.shape().bounding_box() for i in instances]
    a = numpy.array([min(b.a[k] for b in boxes) for k in range(3)], dtype=numpy.float64) - grow
    b = numpy.array([max(b.b[k] for b in boxes) for k in range(3)], dtype=numpy.float64) + grow
    if not (numpy.isfinite(a).all() and numpy.isfinite(b).all()):
        raise ValueError("interference needs instances with finite bounding boxes")
    dims = numpy.maximum(1, numpy.ceil((b - a) / float(step))).astype(numpy.int64)
    corner = (a + float(step) / 2).astype(numpy.float32)
    return corner, step, dims


def visible(asm, resolution):
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


def checked_lattice(instances, resolution, grow=0.0):
    """lattice(), or a lattice of one sample for no instance at all; ValueError above 65536 samples on an axis (a cell
    row has 16 bits per index)."""
    corner, step, dims = lattice(instances, resolution, grow) if instances else (numpy.zeros(3, numpy.float32), numpy.float32(resolution), numpy.ones(3, numpy.int64))
    if dims[0] > 65536 or dims[1] > 65536 or dims[2] > 65536:
        raise ValueError("resolution %g gives a lattice of %s samples: at most 65536 per axis" % (resolution, dims.tolist()))
    return corner, step, dims


def top_side(dims, first=16, factor=4, most=None):
    """The side of the top level's cells: `first` samples, times `factor` (a level's cells per axis: 4 for the cubic
    cells of the checks, 8 for the square tiles of a section) while there would be more than `most` of them
    (_MAX_TOP_CELLS unless a check has a cap of its own)."""
    most = _MAX_TOP_CELLS if most is None else most
    side = first
    while numpy.prod(-(-numpy.asarray(dims, dtype=numpy.int64) // side)) > most:
        side *= factor
    return side


def windows(instances, corner, step, dims, grow=0.0):
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


def cell_rows(wins, dims, side, least=2):
    """Rows of the top level: cells of `side` samples that `least` windows or more reach (a section keeps a tile that one
    window reaches, and gives an instance that is no candidate anywhere an empty window, lo > hi)."""
    n_cells = -(-dims // side)
    masks = numpy.zeros(tuple(int(n) for n in n_cells), dtype=numpy.uint64)
    for n, (lo, hi) in enumerate(wins):
        if (lo > hi).any():
            continue
        lo, hi = lo // side, hi // side
        masks[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] |= numpy.uint64(1 << n)
    bits = numpy.unpackbits(masks.view(numpy.uint8).reshape(masks.shape + (8,)), axis=-1).sum(axis=-1)
    idx = numpy.argwhere(bits >= least)
    rows = numpy.zeros((len(idx), 4), dtype=numpy.uint32)
    if len(idx):
        m = masks[tuple(idx.T)]
        rows[:, 0] = (idx[:, 0] * side) | ((idx[:, 1] * side) << 16)
        rows[:, 1] = idx[:, 2] * side
        rows[:, 2] = (m & numpy.uint64(0xffffffff)).astype(numpy.uint32)
        rows[:, 3] = (m >> numpy.uint64(32)).astype(numpy.uint32)
    return rows


def all_rows(n, dims, side):
    """Rows of the top level: every cell of `side` samples, every one of the n instances a candidate."""
    counts = tuple(int(-(-d // side)) for d in dims)
    idx = numpy.indices(counts).reshape(3, -1).T.astype(numpy.int64) * side
    mask = (1 << n) - 1
    rows = numpy.zeros((len(idx), 4), dtype=numpy.uint32)
    rows[:, 0] = idx[:, 0] | (idx[:, 1] << 16)
    rows[:, 1] = idx[:, 2]
    rows[:, 2] = mask & 0xffffffff
    rows[:, 3] = mask >> 32
    return rows


def top_cells(instances, corner, step, dims, side):
    """Rows of the top level: cells of `side` samples that two instances' boxes (grown by a step) reach."""
    return cell_rows(windows(instances, corner, step, dims), dims, side)


def instance_tape(instance):
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


def device_table(instances, queue, full_programs=False):
    """(device table of the instances' uploaded tapes, distance_only, lane_bytes): hu_instance_table.  The checks take
    what it chooses (every instance's distance-only program when all have one); `full_programs` asks for the full
    programs whatever the instances have (the ray caster over instances follows their directions)."""
    tapes = [instance_tape(i) for i in instances]
    n = len(tapes)
    handles = (ctypes.c_void_p * n)(*(t.device_ptr for t in tapes))
    host_table = numpy.zeros(n * _TABLE_RECORD, dtype=numpy.uint8)
    distance_only, lane_bytes = ctypes.c_int(0), ctypes.c_uint32(0)
    check(hip_manager.lib.hu_instance_table(handles, n, int(bool(full_programs)), host_table.ctypes.data, host_table.nbytes,
                                            ctypes.byref(distance_only), ctypes.byref(lane_bytes)), "hu_instance_table")
    table = hip_util.Buffer(numpy.uint8, (host_table.size,), queue=queue)
    table.enqueue_write(host_table)
    return table, distance_only.value, lane_bytes.value


def levels(side, n_top, initial_capacity, factor=4, row_bytes=_ROW):
    """(sides of the cells of every level above the finest one, the first capacity of every level's child list); a cell
    has `factor` children per axis, 64 in all: 4^3 (the checks) or 8^2 (a section's tiles); a list's rows have `row_bytes`
    (32 for the mass properties' rows with a second mask)."""
    sides = []
    s = side
    while s > factor:
        sides.append(s)
        s //= factor
    capacities = subdivision.first_capacities([64] * len(sides), n_top=n_top, row_bytes=row_bytes)
    if initial_capacity is not None:
        capacities = [subdivision.checked_capacity(min(c, max(1, int(initial_capacity)))) for c in capacities]
    return sides, capacities


def _run(table, n, distance_only, lane_bytes, wins, top, sides, corner, step, dims, capacities, queue, pair_dtype, pair_init, thr,
         cells, finest, factor, frame, row_bytes=_ROW, cells_extra=None, accumulators=None):
    """Every level enqueued back to back, ONE synchronisation -> (list counts, evaluations, pair accumulators)."""
    lib = hip_manager.lib
    n_levels = len(sides)                   # levels of cells above the finest one
    # one device buffer of everything the host reads: [list headers: 16 B per level | evaluations: 16 B | pairs]
    head = 16 * n_levels + 16
    acc_shape = (n, n) if accumulators is None else (accumulators,)
    init = numpy.zeros(head + int(numpy.prod(acc_shape)) * pair_dtype.itemsize, dtype=numpy.uint8)
    pairs0 = init[head:].view(pair_dtype)
    for field, value in pair_init.items():
        pairs0[field] = value
    results = hip_util.Buffer(numpy.uint8, (init.size,), queue=queue)
    results.enqueue_write(init)
    words = row_bytes // 4                  # a list: [header row | rows...], the header's word 0 its length
    first = numpy.zeros((len(top) + 1, words), dtype=numpy.uint32)
    first[0, 0] = len(top)
    first[1:] = top
    parents = hip_util.Buffer(numpy.uint32, first.shape, queue=queue)
    parents.enqueue_write(first)
    buffers = [parents]
    # what every launch takes (include/hip_util.h hu_cells_launch); a level moves the parent fields on to its children
    launch = CellsLaunch(table_dev=table.device_ptr, windows_dev=None if wins is None else wins.device_ptr,
                         evaluations_dev=results.device_ptr + 16 * n_levels, stream=queue.handle, n=n, lane_bytes=lane_bytes,
                         distance_only=distance_only, dims=tuple(int(v) for v in dims), corner=tuple(float(v) for v in corner), step=step)

    def parents_are(buffer, capacity):
        launch.parents_dev, launch.n_parents_dev, launch.max_parents = buffer.device_ptr + row_bytes, buffer.device_ptr, capacity

    parents_are(parents, len(top))
    accumulators_dev = results.device_ptr + head
    extra = () if cells_extra is None else tuple(cells_extra) + (accumulators_dev,)
    for level, (side, capacity) in enumerate(zip(sides, capacities)):
        child = side // factor
        children = hip_util.Buffer(numpy.uint32, (capacity + 1, words), queue=queue)
        check(lib.hu_memset(children.device_ptr, 0, row_bytes, queue.handle), "hu_memset")
        listed = CellsChildren(counter_dev=children.device_ptr, children_dev=children.device_ptr + row_bytes, capacity=capacity,
                               child_side=child, thr=thr(child))
        check(getattr(lib, cells)(ctypes.byref(launch), ctypes.byref(listed), *frame, *extra), cells)
        check(lib.hu_memcpy_d2d(results.device_ptr + 16 * level, children.device_ptr, 16, queue.handle), "hu_memcpy_d2d")
        buffers.append(children)
        parents_are(children, capacity)
    for name, own in finest:                # in this order, on the one stream
        check(getattr(lib, name)(ctypes.byref(launch), *frame, *own, accumulators_dev), name)
    got = results.read()                    # the one synchronisation
    for b in buffers + [results]:
        b.release()
    counts = [int(v) for v in got[:16 * n_levels].view(numpy.uint32).reshape(n_levels, 4)[:, 0]]
    return counts, int(got[16 * n_levels:head].view(numpy.uint64)[0]), got[head:].view(pair_dtype).reshape(acc_shape).copy()


def traverse(instances, top, side, corner, step, dims, initial_capacity, pair_dtype, pair_init, thr, cells, finest, wins=None,
             factor=4, frame=(), row_bytes=_ROW, cells_extra=None, accumulators=None):
    """The traversal from the top-level rows `top` (cells of `side` samples), run again with larger lists while one
    overflowed -> (evaluations of the last run, pair accumulators [n, n], runs).  What the check decides: `pair_dtype`
    and `pair_init` ({field: initial value}) of the accumulators; `thr`, child side -> float32 threshold of a level;
    `cells`, the entry point of the coarser levels; `finest`, [(entry point of the finest level, its own arguments between
    `frame` and the accumulators)], launched in that order; `frame`, what both take first of their own arguments (a
    section's plane); `wins`, clearance's windows (int64[n, 2, 3]), uploaded for
    its entry points; `row_bytes`, the size of a row of `top` and of every list (16, or 32 for rows with a second mask);
    `cells_extra`, arguments of `cells` after `frame`, after which it then also gets the
    accumulators (the mass properties' levels add to them); `accumulators`, their number when it is not n * n."""
    queue = hip_manager.queue
    n = len(instances)
    table, distance_only, lane_bytes = device_table(instances, queue)
    wins_dev = None
    if wins is not None:
        host_wins = numpy.ascontiguousarray(wins.reshape(n, 6).astype(numpy.uint32))
        wins_dev = hip_util.Buffer(numpy.uint32, host_wins.shape, queue=queue)
        wins_dev.enqueue_write(host_wins)
    sides, capacities = levels(side, len(top), initial_capacity, factor, row_bytes)
    runs = 0
    while True:
        runs += 1
        counts, evaluations, acc = _run(table, n, distance_only, lane_bytes, wins_dev, top, sides, corner, step, dims, capacities,
                                        queue, pair_dtype, pair_init, thr, cells, finest, factor, frame, row_bytes, cells_extra,
                                        accumulators)
        if all(k <= c for k, c in zip(counts, capacities)):
            break
        capacities = [subdivision.checked_capacity(max(c, int(k * 1.125) + 16)) for k, c in zip(counts, capacities)]
    table.release()
    if wins_dev is not None:
        wins_dev.release()
    return evaluations, acc, runs


def traverse_records(instances, top, side, corner, step, dims, initial_capacity, capacity, words, thr, cells, leaf, wins, factor,
                     frame=(), too_many=None):
    """traverse() for a finest level that writes RECORDS of `words` uint32 (segments, triangles) into a buffer of `capacity`
    of them and counts them in n + 1 uint64 accumulators, all of them and per instance; `leaf` is its entry point.  Run
    again with int(count * 1.125) + 16 records while they did not fit -- a ValueError(too_many % count) where that is
    given and the new capacity is past 2^32 - 1 -> (evaluations, totals uint64[n + 1], runs of traverse() in all, the
    records written uint32[count, words])."""
    runs = 0
    while True:
        records = hip_util.Buffer(numpy.uint32, (capacity, words), queue=hip_manager.queue)
        try:
            evaluations, totals, ran = traverse(
                instances, top, side, corner, step, dims, initial_capacity, pair_dtype=numpy.dtype(numpy.uint64), pair_init={}, thr=thr,
                cells=cells, finest=[(leaf, (records.device_ptr, capacity))], wins=wins, factor=factor, frame=frame,
                accumulators=len(instances) + 1)
            runs += ran
            total = int(totals[0])
            if total <= capacity:
                rows = records.read()[:total].copy() if total else numpy.zeros((0, words), dtype=numpy.uint32)
                return evaluations, totals, runs, rows
        finally:
            records.release()
        capacity = int(total * 1.125) + 16
        if too_many is not None and capacity > 0xffffffff:
            raise ValueError(too_many % total)


def index_position(corner, step, index):
    """The position of the sample at `index`, as the kernels compute it (float32 per axis)."""
    return util.Vector(*(float(corner[k] + step * numpy.float32(index[k])) for k in range(3)))


def pair_fields(acc, corner, step, diagonal=False):
    """[(PairFields, accumulator)] of the pairs i < j with samples, ordered by (i, j), from the accumulators [n, n];
    `diagonal`: and of the entries [i, i] (a section keeps the samples inside instance i there)."""
    out = []
    cell = float(step) ** 3
    n = len(acc)
    for i in range(n):
        for j in range(i if diagonal else i + 1, n):
            a = acc[i, j]
            count = int(a["sums"][0])
            if count == 0:
                continue
            sums = tuple(int(v) for v in a["sums"][1:])
            lo, hi = tuple(int(v) for v in a["lo"]), tuple(int(v) for v in a["hi"])
            centroid = util.Vector(*(float(corner[k]) + float(step) * sums[k] / count for k in range(3)))
            box = util.BoundingBox(index_position(corner, step, lo), index_position(corner, step, hi))
            out.append((PairFields(i, j, count, count * cell, centroid, (lo, hi), box, sums), a))
    return out
