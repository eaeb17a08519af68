"""islands() on the device against the reference of islands_scenes.py, which is written from the definitions: the part ids, the
three id volumes and their counts, the labels and every field of every island are EQUAL to the reference, entry for entry, on
every scene and direction the scenes name, whatever the labelling's arm and the island table's first capacity were; and the
three new entry points alone, after hu_overhang_first_layer, on raw id volumes whose padding holds ids that would ground or
join if read, the rise driven pass by pass."""
import ctypes

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import hip_util
from codecad_amd.hip_util import check

import disassembly_scenes as dis_scenes
import drainage_scenes
import islands_scenes as scenes
import raw_volume_scenes as raw
import wide_volume_scenes as wide
from islands_scenes import CASES, RAW_CASES, RAW_PARTS, reference, raw_reference, raw_ids, raw_labels, scene, EMPTY, NONE, SOLID

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5
FLAG = 0x80000000


def run(name, axis, up, of, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    report = cc.islands(asm, resolution, axis=axis, up=up, of=of, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert len(report.instances) == len(instances) and (report.axis, report.up, report.of) == (axis, up, of)
    return report


def check_against_reference(report, ref, axis, up):
    n = len(ref.floating_counts)
    shape = ref.ids.shape
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    assert report.first_layer == ref.first_layer
    for field in ("floating_ids", "start_ids", "join_ids"):
        got, want = getattr(report, field), getattr(ref, field)
        assert got.dtype == numpy.uint8 and got.flags.c_contiguous and got.shape == shape
        wrong = numpy.argwhere(got != want)
        assert len(wrong) == 0, (field, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]])
    for field in ("floating_counts", "start_counts", "join_counts"):
        got = getattr(report, field)
        assert got == getattr(ref, field) and all(type(c) is int for c in got) and len(got) == n, field
    assert report.floating_volume == sum(ref.floating_counts) * float(report.step) ** 3
    assert report.labels.dtype == numpy.uint32 and report.labels.flags.c_contiguous and numpy.array_equal(report.labels, ref.labels)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in report.islands]
    assert got == [tuple(r.expected) for r in ref.islands]
    names = [i.name for i in report.instances]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for r, want in zip(report.islands, ref.islands):
        assert r.volume == r.count * step ** 3
        assert tuple(r.centroid) == tuple(corner[k] + step * r.index_sums[k] / r.count for k in range(3))
        assert r.owners == tuple(names[k] for k in r.parts)
        assert (r.first_layer, r.starts, r.loose) == (want.first_layer, want.starts, want.loose)
        assert type(r.starts) is int and type(r.loose) is bool
        assert report.mask(r).sum() == r.count and set(numpy.unique(report.floating_ids[report.mask(r)]).tolist()) == set(r.parts)
    assert 1 <= report.passes <= shape[axis] + 1
    assert report.grounded == (sum(ref.floating_counts) == 0)


@pytest.mark.parametrize("name,axis,up,of", CASES)
def test_everything_equals_the_reference(hip, name, axis, up, of):
    ref = reference(name, axis, up, of)
    report = run(name, axis, up, of)
    print(name, "xyz"[axis], "+" if up else "-", of, "floating", sum(report.floating_counts), "reference", sum(ref.floating_counts), "islands",
          len(report.islands), "reference", len(ref.islands), "passes", report.passes)
    check_against_reference(report, ref, axis, up)
    assert report.traversals == 1 and report.component_capacity_runs == 1
    other = run(name, axis, up, of, local=False)                                    # the comparison arm: the same bytes
    check_against_reference(other, ref, axis, up)
    small = run(name, axis, up, of, initial_components=1)                           # an island table of one row
    check_against_reference(small, ref, axis, up)
    assert small.component_capacity_runs == (2 if len(ref.islands) > 1 else 1)
    again = run(name, axis, up, of)                                                 # the same bytes, whatever order anything ran in
    for field in ("part_ids", "floating_ids", "start_ids", "join_ids", "labels"):
        for one in (other, small, again):
            assert getattr(one, field).tobytes() == getattr(report, field).tobytes(), field
    assert again.floating_counts == report.floating_counts and again.islands == report.islands == other.islands == small.islands


def test_the_empty_assembly_launches_nothing(hip):
    report = cc.islands(dis_scenes.empty_assembly(), 0.1, axis=1)
    assert report.traversals == 0 and report.passes == 0 and report.islands == [] and report.component_capacity_runs == 0 and report.grounded


# ---- the entry points alone ---------------------------------------------------------------------------------------------

def padded_ids(ids, of, pitch=None):
    """The volume in a buffer of pitch `pitch`, ceil16(nz) without one, whose padding alternates empty and an id of S: read as
    data, it would ground, join and close starts."""
    return raw.padded(ids, raw.ground_poison(of), pitch)


def flagged_of(entries, s, nz):
    """bool[nx, ny, nz]: the samples of S whose root's entry has bit 31 set, from the label buffer read back after a flatten."""
    flat = entries.ravel()
    own = entries[:, :, :nz]
    root = numpy.where(s, own & (FLAG - 1), 0)                                       # a root's own entry may carry the flag
    return s & (((own & FLAG) != 0) | ((flat[root] & FLAG) != 0))


def linear_of(entries, s, nz):
    """uint32[nx, ny, nz]: the LINEAR index of an entry's buffer index on S (flags dropped), NONE elsewhere."""
    pz = entries.shape[2]
    q = (entries[:, :, :nz] & (FLAG - 1)).astype(numpy.int64)
    return numpy.where(s, q - (q // pz) * (pz - nz), NONE).astype(numpy.uint32)


@pytest.mark.parametrize("name,axis,up,of", RAW_CASES)
def test_the_entry_points_alone_on_raw_volumes(hip, name, axis, up, of):
    ids, ref, layer_ref = raw_ids(name), raw_reference(name, axis, up, of), raw_labels(name, axis, of)
    nx, ny, nz = ids.shape
    na = ids.shape[axis]
    s = ref.s
    code = 255 if of == SOLID else of
    padded, pz = padded_ids(ids, of)
    lib, queue = hip.lib, hip.queue
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    volume, floating, start, join = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(4))
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (3, 64), queue=queue)
    depth, word = (hip_util.Buffer(numpy.uint32, (1,), queue=queue) for _ in range(2))
    volume.enqueue_write(padded)
    for b in (floating, start, join):
        b.enqueue_fill(SENTINEL)
    acc.enqueue_fill(0)
    depth.enqueue_fill(0)
    check(lib.hu_overhang_first_layer(volume.device_ptr, depth.device_ptr, dims, pz, axis, int(up), code, queue.handle), "hu_overhang_first_layer")
    # stage 1, both arms: the least index of every layer's component of S
    for local in (0, 1):
        labels.enqueue_fill(SENTINEL)
        check(lib.hu_ground_layers(volume.device_ptr, labels.device_ptr, dims, pz, axis, code, local, queue.handle), "hu_ground_layers")
        check(lib.hu_components_flatten(labels.device_ptr, dims, pz, queue.handle), "hu_components_flatten")
        entries = labels.read().copy()
        assert numpy.array_equal(linear_of(entries, s, nz), layer_ref), local
        assert (entries[:, :, :nz][~s] == NONE).all() and (entries[:, :, nz:] == NONE).all()
    # stage 2: the depth word is read on the device; the components of layer h0, no more
    check(lib.hu_ground_seed(labels.device_ptr, depth.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_ground_seed")
    assert int(depth.read()[0]) == na - ref.first_layer
    flagged = flagged_of(labels.read().copy(), s, nz)
    assert numpy.array_equal(flagged, scenes.synchronous(s, axis, up, 0, layer_ref))
    # stage 3, pass by pass: at least the synchronous steps, never beyond the fixed point
    passes = 0
    while True:
        word.enqueue_fill(0)
        check(lib.hu_drain_rise(labels.device_ptr, word.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_drain_rise")
        passes += 1
        changed = int(word.read()[0])
        entries = labels.read().copy()
        now = flagged_of(entries, s, nz)
        assert not (scenes.synchronous(s, axis, up, passes, layer_ref) & ~now).any(), passes
        assert not (now & ~ref.grounded).any() and not (flagged & ~now).any(), passes
        assert changed in (0, 1) and (changed == 1) == bool((now & ~flagged).any()), passes
        assert numpy.array_equal(linear_of(entries, s, nz), layer_ref)              # the flags apart, no entry has moved
        flagged = now
        assert passes <= na + 1
        if not changed:
            break
    print(name, "xyz"[axis], "+" if up else "-", of, "passes", passes, "floating", int(ref.floating.sum()))
    assert numpy.array_equal(flagged, ref.grounded)                                 # the pass after the fixed point changed nothing
    # stage 4: the three volumes, every in-lattice byte, and no byte of the padding
    check(lib.hu_ground_mark(volume.device_ptr, labels.device_ptr, floating.device_ptr, start.device_ptr, join.device_ptr, acc.device_ptr,
                             dims, pz, axis, int(up), code, queue.handle), "hu_ground_mark")
    written = [b.read().copy() for b in (floating, start, join)]
    totals = acc.read().copy()
    for b in (volume, floating, start, join, labels, acc, depth, word):
        b.release()
    for got, want, field in zip(written, (ref.floating_ids, ref.start_ids, ref.join_ids), ("floating", "start", "join")):
        wrong = numpy.argwhere(got[:, :, :nz] != want)
        assert len(wrong) == 0, (field, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]])
        assert (got[:, :, nz:] == SENTINEL).all(), field
    assert [[int(v) for v in totals[k, :RAW_PARTS]] for k in range(3)] == [ref.floating_counts, ref.start_counts, ref.join_counts]


@pytest.mark.parametrize("name", ["two_ids", "19x21x70"])
def test_stage_one_alone_serves_the_three_predicates_from_one_kernel(hip, name):
    """hu_drain_layers (id == 255), hu_ground_layers(of=SOLID) (id != 255) and hu_ground_layers(of=k) (id == k) launch one
    kernel set with two words of its record: the sets that come out labelled are exactly those, on every axis and both arms,
    the padding poisoned with ids of the set that is asked for."""
    ids = raw_ids(name)
    nx, ny, nz = ids.shape
    lib, queue = hip.lib, hip.queue
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    volumes = {}
    for poison in (0, 1):                                                           # the padding alternates 255 and `poison`
        padded, pz = padded_ids(ids, poison)
        volumes[poison] = hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue)
        volumes[poison].enqueue_write(padded)
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    # (what to call, the volume it reads, the set by its definition, the layers' components of that set by flood fill)
    empty = ids == EMPTY
    predicates = {"empty": (None, 1, empty, lambda axis: drainage_scenes.layer_labels(empty, axis)),
                  "solid": (255, 1, ids != EMPTY, lambda axis: raw_labels(name, axis, SOLID)),
                  "of=0": (0, 0, ids == 0, lambda axis: raw_labels(name, axis, 0)),
                  "of=1": (1, 1, ids == 1, lambda axis: raw_labels(name, axis, 1))}
    for axis in range(3):
        for local in (0, 1):
            for key, (code, poison, want, layer_ref) in predicates.items():
                volume = volumes[poison]
                labels.enqueue_fill(SENTINEL)
                if code is None:
                    check(lib.hu_drain_layers(volume.device_ptr, labels.device_ptr, dims, pz, axis, local, queue.handle), "hu_drain_layers")
                else:
                    check(lib.hu_ground_layers(volume.device_ptr, labels.device_ptr, dims, pz, axis, code, local, queue.handle), "hu_ground_layers")
                check(lib.hu_components_flatten(labels.device_ptr, dims, pz, queue.handle), "hu_components_flatten")
                entries = labels.read().copy()
                got = entries[:, :, :nz] != NONE
                assert numpy.array_equal(got, want), (key, axis, local)
                assert (entries[:, :, nz:] == NONE).all(), (key, axis, local)
                assert numpy.array_equal(linear_of(entries, want, nz), layer_ref(axis)), (key, axis, local)
    for b in (volumes[0], volumes[1], labels):
        b.release()
    # what the four sets are to each other, so that no predicate can stand in for another
    e, s, zero, one = (predicates[key][2] for key in ("empty", "solid", "of=0", "of=1"))
    assert (e ^ s).all() and e.any() and s.any()                                    # the first two partition the lattice
    assert zero.any() and one.any() and not (zero & one).any() and not ((zero | one) & ~s).any()
    if name == "two_ids":
        assert numpy.array_equal(zero | one, s)                                     # the last two partition the solid
    else:
        assert set(numpy.unique(ids[s]).tolist()) == set(range(64)) and (s & ~(zero | one)).any()


# ---- past the grid's cap: a wavefront takes a second unit (wide_volume_scenes.py) -----------------------------------------------

def same_bytes(got, want, what):
    wrong = numpy.argwhere(got != want)
    assert len(wrong) == 0, (what, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]])


@pytest.mark.parametrize("of", [SOLID, 63])
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("name", list(wide.REACH_SHAPES))
def test_a_wavefront_walks_a_second_column(hip, name, up, of):
    """hu_ground_mark, hu_ground_seed and hu_drain_rise along z over more than GRID_WAVEFRONTS columns, on labels written here
    (every layer component is one sample) with crafted flags: the first columns end in a grounded sample of S, the second begin
    with a floating one or outside S."""
    shape = wide.REACH_SHAPES[name]
    c = wide.reach_case(shape, "solid")
    nx, ny, nz = shape
    s = scenes.in_set_of(c.ids, of)
    flags = c.flags & s
    code = 255 if of == SOLID else of
    padded, pz = padded_ids(c.ids, of)
    lib, queue = hip.lib, hip.queue
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    volume, floating, start, join = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(4))
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    acc = hip_util.Buffer(numpy.uint64, (3, 64), queue=queue)
    depth, word = (hip_util.Buffer(numpy.uint32, (1,), queue=queue) for _ in range(2))

    def marks(grounded, what):
        for b in (floating, start, join):
            b.enqueue_fill(SENTINEL)
        acc.enqueue_fill(0)
        check(lib.hu_ground_mark(volume.device_ptr, labels.device_ptr, floating.device_ptr, start.device_ptr, join.device_ptr, acc.device_ptr,
                                 dims, pz, 2, int(up), code, queue.handle), "hu_ground_mark")
        totals = acc.read().copy()
        for k, (b, (want, counts)) in enumerate(zip((floating, start, join), wide.marks_of(c.ids, s, grounded, 2, up))):
            got = b.read().copy()
            same_bytes(got[:, :, :nz], want, (what, k))
            assert (got[:, :, nz:] == SENTINEL).all() and [int(v) for v in totals[k]] == counts and sum(counts) > 0, (what, k)

    try:
        volume.enqueue_write(padded)
        labels.enqueue_write(wide.own_labels(s, pz, flags))
        marks(flags, "the marks under the crafted flags")
        want = wide.risen(s, flags, 2, up)
        for changed in (1, 0):
            word.enqueue_fill(0)
            check(lib.hu_drain_rise(labels.device_ptr, word.device_ptr, dims, pz, 2, int(up), queue.handle), "hu_drain_rise")
            assert int(word.read()[0]) == changed
            same_bytes(labels.read().copy(), wide.own_labels(s, pz, want), "the labels after the rise")
        marks(want, "the marks after the rise")
        # the seeds: the true first layer, and layers that the word only claims, in the second word and in the last lane of the first
        for h0 in (scenes.first_layer(s, 2, up), 65, 63):
            labels.enqueue_write(wide.own_labels(s, pz))
            depth.enqueue_write(numpy.array([nz - h0], dtype=numpy.uint32))
            check(lib.hu_ground_seed(labels.device_ptr, depth.device_ptr, dims, pz, 2, int(up), queue.handle), "hu_ground_seed")
            seeds = s & (drainage_scenes.layers(shape, 2, up) == h0)
            assert seeds.any() and int(depth.read()[0]) == nz - h0
            same_bytes(labels.read().copy(), wide.own_labels(s, pz, seeds), ("the seeds of layer", h0))
        assert numpy.array_equal(s & (drainage_scenes.layers(shape, 2, up) == scenes.first_layer(s, 2, up)), scenes.seeds(s, 2, up))
    finally:
        for b in (volume, floating, start, join, labels, acc, depth, word):
            b.release()


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("na", raw.WIDE_NA)
@pytest.mark.parametrize("axis", [0, 1])
def test_a_wavefront_seeds_a_second_line(hip, axis, na, up):
    """hu_ground_seed along x and y over 10000 line units: a layer component is a whole z line, its root the sample at z = 0, and
    the lanes of a unit share it.  Every layer in turn is claimed by the depth word."""
    ids, r = wide.seed_lines(axis, na)
    nx, ny, nz = ids.shape
    pz = raw.ceil16(nz) + 16
    lib, queue = hip.lib, hip.queue
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    labels = hip_util.Buffer(numpy.uint32, (nx, ny, pz), queue=queue)
    depth = hip_util.Buffer(numpy.uint32, (1,), queue=queue)
    try:
        for layer in sorted({0, na // 2, na - 1}):
            labels.enqueue_write(wide.line_labels(r, pz))
            depth.enqueue_write(numpy.array([na - (layer if up else na - 1 - layer)], dtype=numpy.uint32))
            check(lib.hu_ground_seed(labels.device_ptr, depth.device_ptr, dims, pz, axis, int(up), queue.handle), "hu_ground_seed")
            same_bytes(labels.read().copy(), wide.line_labels(r, pz, wide.seeded_lines(r, axis, layer, False)), ("layer", layer))
    finally:
        labels.release(), depth.release()
