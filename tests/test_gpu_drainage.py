"""drainage() on the device against the reference of drainage_scenes.py, which is written from the definitions: the part ids, the
trapped ids and their counts, the labels and every field of every pool are EQUAL to the reference, entry for entry, on every
scene and in all six directions, whatever the labelling's arm and the pool table's first capacity were; and the four entry
points alone on raw id volumes whose padding holds ids that would change the answer, the rise driven pass by pass; and the
rise and the floors along z over more columns than the grid has wavefronts, where a wavefront takes a second column."""
import ctypes

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import hip_util
from codecad_amd.hip_util import check

import disassembly_scenes as dis_scenes
import drainage_scenes as scenes
import raw_volume_scenes as raw
import wide_volume_scenes as wide
from drainage_scenes import CASES, RAW_CASES, RAW_PARTS, reference, raw_reference, raw_ids, raw_labels, scene, EMPTY, NONE

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5
FLAG = 0x80000000


def run(name, axis, up, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    report = cc.drainage(asm, resolution, axis=axis, up=up, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert len(report.instances) == len(instances) and (report.axis, report.up) == (axis, up)
    return report


def check_against_reference(report, ref, axis, up):
    n = len(ref.counts)
    shape = ref.ids.shape
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    assert report.trapped_ids.dtype == numpy.uint8 and report.trapped_ids.flags.c_contiguous
    wrong = numpy.argwhere(report.trapped_ids != ref.trapped_ids)
    assert len(wrong) == 0, [(tuple(k), int(report.trapped_ids[tuple(k)]), int(ref.trapped_ids[tuple(k)])) for k in wrong[:8]]
    assert report.trapped_counts == ref.trapped_counts and all(type(c) is int for c in report.trapped_counts) and len(report.trapped_counts) == n
    assert report.trapped_volume == sum(ref.trapped_counts) * float(report.step) ** 3
    assert report.labels.dtype == numpy.uint32 and report.labels.flags.c_contiguous and numpy.array_equal(report.labels, ref.labels)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in report.pools]
    assert got == [tuple(r) for r in ref.pools]
    names = [i.name for i in report.instances]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for r in report.pools:
        assert r.volume == r.count * step ** 3
        assert tuple(r.centroid) == tuple(corner[k] + step * r.index_sums[k] / r.count for k in range(3))
        assert r.held_by == tuple(names[k] for k in r.parts) and r.level == scenes.level_of(r, shape, axis, up)
        assert report.mask(r).sum() == r.count and set(numpy.unique(report.trapped_ids[report.mask(r)]).tolist()) == set(r.parts)
    assert 1 <= report.passes <= shape[axis] + 1
    assert report.drains == (sum(ref.trapped_counts) == 0)


@pytest.mark.parametrize("name,axis,up", CASES)
def test_everything_equals_the_reference(hip, name, axis, up):
    ref = reference(name, axis, up)
    report = run(name, axis, up)
    print(name, "xyz"[axis], "+" if up else "-", "trapped", sum(report.trapped_counts), "reference", sum(ref.trapped_counts), "pools",
          len(report.pools), "reference", len(ref.pools), "passes", report.passes)
    check_against_reference(report, ref, axis, up)
    assert report.traversals == 1 and report.component_capacity_runs == 1
    other = run(name, axis, up, local=False)                                        # the comparison arm: the same bytes
    check_against_reference(other, ref, axis, up)
    small = run(name, axis, up, initial_components=1)                               # a pool table of one row
    check_against_reference(small, ref, axis, up)
    assert small.component_capacity_runs == (2 if len(ref.pools) > 1 else 1)
    again = run(name, axis, up)                                                     # the same bytes, whatever order anything ran in
    for field in ("part_ids", "trapped_ids", "labels"):
        for one in (other, small, again):
            assert getattr(one, field).tobytes() == getattr(report, field).tobytes(), field
    assert again.trapped_counts == report.trapped_counts and again.pools == report.pools == other.pools == small.pools


def test_a_straight_shaft_rises_in_one_pass(hip):
    """Downwards the shaft is open at layer 0 and 135 layers deep: the pass that raises it and the pass that finds nothing to do."""
    assert run("shaft", 2, False).passes == 2
    assert run("shaft", 2, True).passes == 1                                        # nothing under the blind end escapes: nothing to hand on


def test_the_empty_assembly_launches_nothing(hip):
    report = cc.drainage(dis_scenes.empty_assembly(), 0.1, axis=1)
    assert report.traversals == 0 and report.passes == 0 and report.pools == [] and report.component_capacity_runs == 0 and report.drains


# ---- the entry points alone ---------------------------------------------------------------------------------------------

def padded_ids(ids, pitch=None):
    """The volume in a buffer of pitch `pitch`, ceil16(nz) without one, whose padding alternates empty and solid: read as data,
    it would open ways out and lay floors."""
    return raw.padded(ids, raw.DRAIN_POISON, pitch)


def flagged_of(entries, empty, nz):
    """bool[nx, ny, nz]: the samples of E whose root's entry has bit 31 set, from the label buffer read back after a flatten."""
    flat = entries.ravel()
    own = entries[:, :, :nz]
    root = numpy.where(empty, own & (FLAG - 1), 0)                                   # a root's own entry may carry the flag
    return empty & (((own & FLAG) != 0) | ((flat[root] & FLAG) != 0))


def linear_of(entries, empty, nz):
    """uint32[nx, ny, nz]: the LINEAR index of an entry's buffer index on E (flags dropped), NONE elsewhere."""
    pz = entries.shape[2]
    q = (entries[:, :, :nz] & (FLAG - 1)).astype(numpy.int64)
    return numpy.where(empty, q - (q // pz) * (pz - nz), NONE).astype(numpy.uint32)


@pytest.mark.parametrize("name,axis,up", RAW_CASES)
def test_the_entry_points_alone_on_raw_volumes(hip, name, axis, up):
    ids, ref, layer_ref = raw_ids(name), raw_reference(name, axis, up), raw_labels(name, axis)
    nx, ny, nz = ids.shape
    na = ids.shape[axis]
    empty = ids == EMPTY
    padded, pz = padded_ids(ids)
    lib, queue = hip.lib, hip.queue
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    volume, trapped = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(2))
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (64,), queue=queue)
    word = hip_util.Buffer(numpy.uint32, (1,), queue=queue)
    volume.enqueue_write(padded)
    trapped.enqueue_fill(SENTINEL)
    acc.enqueue_fill(0)
    # stage 1, both arms: the least index of every layer's component
    for local in (0, 1):
        labels.enqueue_fill(SENTINEL)
        check(lib.hu_drain_layers(volume.device_ptr, labels.device_ptr, dims, pz, axis, local, queue.handle), "hu_drain_layers")
        check(lib.hu_components_flatten(labels.device_ptr, dims, pz, queue.handle), "hu_components_flatten")
        entries = labels.read().copy()
        assert numpy.array_equal(linear_of(entries, empty, nz), layer_ref), local
        assert (entries[:, :, :nz][~empty] == NONE).all() and (entries[:, :, nz:] == NONE).all()
    # stage 2: the seeds' components, no more
    check(lib.hu_drain_seed(labels.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_drain_seed")
    flagged = flagged_of(labels.read().copy(), empty, nz)
    assert numpy.array_equal(flagged, scenes.synchronous(empty, axis, up, 0, layer_ref))
    # stage 3, pass by pass: at least the synchronous steps, never beyond the fixed point
    passes = 0
    while True:
        word.enqueue_fill(0)
        check(lib.hu_drain_rise(labels.device_ptr, word.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_drain_rise")
        passes += 1
        changed = int(word.read()[0])
        entries = labels.read().copy()
        now = flagged_of(entries, empty, nz)
        assert not (scenes.synchronous(empty, axis, up, passes, layer_ref) & ~now).any(), passes
        assert not (now & ~ref.escapes).any() and not (flagged & ~now).any(), passes
        assert changed in (0, 1) and (changed == 1) == bool((now & ~flagged).any()), passes
        assert numpy.array_equal(linear_of(entries, empty, nz), layer_ref)          # the flags apart, no entry has moved
        flagged = now
        assert passes <= na + 1
        if not changed:
            break
    print(name, "xyz"[axis], "+" if up else "-", "passes", passes, "trapped", int(ref.trapped.sum()))
    assert numpy.array_equal(flagged, ref.escapes)                                  # the pass after the fixed point changed nothing
    # stage 4: the floors, every in-lattice byte, and no byte of the padding
    check(lib.hu_drain_floor(volume.device_ptr, labels.device_ptr, trapped.device_ptr, acc.device_ptr, dims, pz, axis, int(up),
                             queue.handle), "hu_drain_floor")
    written, totals = trapped.read().copy(), acc.read().copy()
    for b in (volume, trapped, labels, acc, word):
        b.release()
    wrong = numpy.argwhere(written[:, :, :nz] != ref.trapped_ids)
    assert len(wrong) == 0, [(tuple(k), int(written[tuple(k)]), int(ref.trapped_ids[tuple(k)])) for k in wrong[:8]]
    assert (written[:, :, nz:] == SENTINEL).all()
    assert [int(v) for v in totals[:RAW_PARTS]] == ref.trapped_counts


# ---- past the grid's cap: a wavefront takes a second column (wide_volume_scenes.py) ---------------------------------------------

def same_bytes(got, want, what):
    wrong = numpy.argwhere(got != want)
    assert len(wrong) == 0, (what, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]])


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("name", list(wide.REACH_SHAPES))
def test_a_wavefront_walks_a_second_column(hip, name, up):
    """hu_drain_floor and hu_drain_rise along z over more than GRID_WAVEFRONTS columns, on labels whose flags are crafted: every
    layer component is one sample, so the label buffer is written here and ONE pass of the rise is the fixed point.  The first
    columns end flagged and with a floor, the second begin unflagged or outside E: a carry or a floor taken along would show."""
    shape = wide.REACH_SHAPES[name]
    c = wide.reach_case(shape, "empty")
    nx, ny, nz = shape
    padded, pz = padded_ids(c.ids)
    lib, queue = hip.lib, hip.queue
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    volume, trapped = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(2))
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (64,), queue=queue)
    word = hip_util.Buffer(numpy.uint32, (1,), queue=queue)
    buffers = (volume, trapped, labels, acc, word)

    def floors(flagged, what):
        trapped.enqueue_fill(SENTINEL)
        acc.enqueue_fill(0)
        check(lib.hu_drain_floor(volume.device_ptr, labels.device_ptr, trapped.device_ptr, acc.device_ptr, dims, pz, 2, int(up),
                                 queue.handle), "hu_drain_floor")
        written, totals = trapped.read().copy(), acc.read().copy()
        want, counts = wide.trapped_of(c.ids, flagged, 2, up)
        same_bytes(written[:, :, :nz], want, what)
        assert (written[:, :, nz:] == SENTINEL).all() and [int(v) for v in totals] == counts and sum(counts) > 0, what

    try:
        volume.enqueue_write(padded)
        labels.enqueue_write(wide.own_labels(c.r, pz, c.flags))
        floors(c.flags, "the floors under the crafted flags")
        want = wide.risen(c.r, c.flags, 2, up)
        for changed in (1, 0):                                                          # the pass, and a pass that finds nothing to do
            word.enqueue_fill(0)
            check(lib.hu_drain_rise(labels.device_ptr, word.device_ptr, dims, pz, 2, int(up), queue.handle), "hu_drain_rise")
            assert int(word.read()[0]) == changed
            same_bytes(labels.read().copy(), wide.own_labels(c.r, pz, want), "the labels after the rise")
        floors(want, "the floors after the rise")
    finally:
        for b in buffers:
            b.release()
