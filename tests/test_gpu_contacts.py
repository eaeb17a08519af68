"""contacts() on the device against the reference of contacts_scenes.py, which is written from the definitions: the faces, the
sums, the boxes, the witnesses, the exposed counts, the contact ids and their counts, the labels and every field of every patch
are EQUAL to the reference, entry for entry, on every scene, whatever the labelling's arm and the patch table's first capacity
were; and hu_contact_faces alone on raw id volumes whose padding is filled with ids that would make contacts."""
import ctypes

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import hip_util
from codecad_amd.hip_util import check

import contacts_scenes as scenes
import disassembly_scenes as dis_scenes
import raw_volume_scenes as raw
from contacts_scenes import SCENES, NAMES, RAW_NAMES, RAW_PARTS, reference, raw_reference, raw_ids, scene, EMPTY, NONE

pytestmark = pytest.mark.gpu
con = __import__("sys").modules["codecad_amd.contacts"]
SENTINEL = 0xa5


def run(name, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    report = cc.contacts(asm, resolution, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert len(report.instances) == len(instances)
    return report


def check_tables(got, ref, n):
    """got: (faces, index_sums, box, witness, exposed, contact_ids, contact_counts)"""
    faces, sums, box, witness, exposed, contact_ids, contact_counts = got
    for array, want, dtype, shape in ((faces, ref.faces, numpy.uint64, (3, n, n)), (sums, ref.index_sums, numpy.uint64, (3, n, n, 3)),
                                      (box, ref.box, numpy.int32, (3, n, n, 2, 3)), (witness, ref.witness, numpy.int32, (3, n, n, 3)),
                                      (exposed, ref.exposed, numpy.uint64, (3, 2, n))):
        assert array.dtype == dtype and array.shape == shape
        wrong = numpy.argwhere(array != want)
        assert len(wrong) == 0, [(tuple(k), int(array[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]]
    assert contact_ids.dtype == numpy.uint8 and contact_ids.flags.c_contiguous and numpy.array_equal(contact_ids, ref.contact_ids)
    assert contact_counts == ref.contact_counts and all(type(c) is int for c in contact_counts)


def check_against_reference(report, ref, patches=True):
    n = len(ref.counts)
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    assert report.counts == ref.counts and all(type(c) is int for c in report.counts)
    check_tables((report.faces, report.index_sums, report.box, report.witness, report.exposed, report.contact_ids, report.contact_counts), ref, n)
    f = report.faces.astype(numpy.int64)                                            # ONE INVARIANT
    assert numpy.array_equal(report.exposed[:, 0].astype(numpy.int64) + f.sum(axis=2), report.exposed[:, 1].astype(numpy.int64) + f.sum(axis=1))
    assert report.labels.dtype == numpy.uint32 and report.labels.flags.c_contiguous and report.labels.shape == ref.ids.shape
    if not patches:
        assert report.patches == [] and (report.labels == NONE).all() and report.component_capacity_runs == 0
        return
    assert numpy.array_equal(report.labels, ref.labels)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in report.patches]
    assert got == [tuple(r) for r in ref.patches]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for r in report.patches:
        assert r.volume == r.count * step ** 3
        assert tuple(r.centroid) == tuple(corner[k] + step * r.index_sums[k] / r.count for k in range(3))
        assert report.mask(r).sum() == r.count and (report.contact_ids[report.mask(r)] != EMPTY).all()
    assert ((report.labels == NONE) == (report.contact_ids == EMPTY)).all()


@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name):
    report = run(name)
    ref, sc = reference(name), SCENES[name]
    print(name, "faces", report.faces.sum(axis=(1, 2)).tolist(), "reference", ref.faces.sum(axis=(1, 2)).tolist(), "exposed",
          report.exposed.sum(axis=2).tolist(), "reference", ref.exposed.sum(axis=2).tolist(), "interface", sum(report.contact_counts),
          "reference", sum(ref.contact_counts), "patches", len(report.patches), "reference", len(ref.patches))
    check_against_reference(report, ref)
    assert report.traversals == 1 and report.component_capacity_runs == (1 if len(ref.counts) else 0)
    for (axis, i, j), (count, (lo, hi), p) in sc.by_hand.items():
        assert int(report.faces[axis, i, j]) == count and report.box[axis, i, j].tolist() == [list(lo), list(hi)]
        assert tuple(report.witness[axis, i, j].tolist()) == tuple(p)
    if sc.groups is not None:
        assert report.groups() == sc.groups and report.loose() == sc.loose and [p.parts for p in report.patches] == sc.patches
    again = run(name)                                                               # the same bytes, whatever order anything ran in
    for field in ("faces", "index_sums", "box", "witness", "exposed", "contact_ids", "labels", "part_ids"):
        assert getattr(again, field).tobytes() == getattr(report, field).tobytes(), field
    assert again.contact_counts == report.contact_counts and again.patches == report.patches


@pytest.mark.parametrize("name", ["three", "two_patches", "stack_z", "hooks", "slabs64_z", "ownership"])
def test_the_other_arms_change_nothing(hip, name):
    ref = reference(name)
    check_against_reference(run(name, local=False), ref)
    small = run(name, initial_components=1)
    check_against_reference(small, ref)
    assert small.component_capacity_runs == (2 if len(ref.patches) > 1 else 1) and small.traversals == 1
    bare = run(name, patches=False)
    check_against_reference(bare, ref, patches=False)


def test_two_runs_of_the_patch_table(hip):
    ref = reference("two_patches")
    assert len(ref.patches) == 2
    small = run("two_patches", initial_components=1)
    check_against_reference(small, ref)
    assert small.component_capacity_runs == 2


@pytest.mark.parametrize("name", ["peg", "words", "ownership"])
def test_a_face_is_a_distance_of_one_on_the_device(hip, name):
    asm, resolution = scene(name)[:2]
    report, other = cc.contacts(asm, resolution, patches=False), cc.disassembly(asm, resolution)
    touching = report.faces > 0
    assert touching.any() and numpy.array_equal(touching, other.distance == 1)
    assert numpy.array_equal(report.witness[touching], other.witness[touching])
    for axis in range(3):
        assert other.contacts(axis) == [(int(i), int(j)) for i, j in numpy.argwhere(touching[axis])]


def raw_call(hip, name, with_contact_ids, pitch=None):
    """hu_contact_faces alone over a raw volume in a buffer of pitch `pitch`, ceil16(nz) without one, whose padding alternates 0
    and 1 -> the tables as contacts() decodes them, and the output buffer, which was filled with SENTINEL."""
    ids = raw_ids(name)
    nx, ny, nz = ids.shape
    padded, pz = raw.padded(ids, raw.CONTACT_POISON, pitch)                        # would make contacts
    lib, queue = hip.lib, hip.queue
    volume, out = (hip_util.Buffer(numpy.uint8, (nx, ny, pz), queue=queue) for _ in range(2))
    volume.enqueue_write(padded)
    out.enqueue_fill(SENTINEL)
    rows = hip_util.Buffer(con._ROW, con._ROWS, queue=queue)
    acc = hip_util.Buffer(numpy.uint64, con._COUNTS, queue=queue)
    rows.enqueue_fill(0)
    acc.enqueue_fill(0)
    dims = (ctypes.c_uint32 * 3)(nx, ny, nz)
    check(lib.hu_contact_faces(volume.device_ptr, out.device_ptr if with_contact_ids else None, rows.device_ptr, acc.device_ptr, dims, pz,
                               RAW_PARTS, queue.handle), "hu_contact_faces")
    table, totals, written = rows.read().copy(), acc.read().copy(), out.read().copy()
    for b in (volume, out, rows, acc):
        b.release()
    n = RAW_PARTS
    exposed = numpy.ascontiguousarray(totals[:6, :n].reshape(3, 2, n))
    return con._decode(table, n) + (exposed, [int(v) for v in totals[6, :n]]), written, nz


@pytest.mark.parametrize("name", RAW_NAMES)
def test_the_kernel_alone_on_raw_volumes(hip, name):
    ref = raw_reference(name)
    (faces, sums, box, witness, exposed, contact_counts), written, nz = raw_call(hip, name, True)
    print(name, "faces", faces.sum(axis=(1, 2)).tolist(), "reference", ref.faces.sum(axis=(1, 2)).tolist(), "rows in use",
          int((faces > 0).sum()), "reference", int((ref.faces > 0).sum()), "interface", sum(contact_counts), "reference", sum(ref.contact_counts))
    check_tables((faces, sums, box, witness, exposed, numpy.ascontiguousarray(written[:, :, :nz]), contact_counts), ref, RAW_PARTS)
    assert (written[:, :, nz:] == SENTINEL).all()                                   # the padding is never written
    # ... and without the contact volume: the same tables, nothing written at all
    (faces2, sums2, box2, witness2, exposed2, counts2), untouched, nz = raw_call(hip, name, False)
    check_tables((faces2, sums2, box2, witness2, exposed2, ref.contact_ids, counts2), ref, RAW_PARTS)
    assert (untouched == SENTINEL).all()


def test_the_empty_assembly_launches_nothing(hip):
    for patches in (True, False):
        report = cc.contacts(dis_scenes.empty_assembly(), 0.1, patches=patches)
        assert report.traversals == 0 and report.faces.shape == (3, 0, 0) and report.patches == [] and report.component_capacity_runs == 0
        assert report.pairs() == [] and report.groups() == []
