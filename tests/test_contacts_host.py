"""The reference and the scenarios of test_gpu_contacts.py, and the host side of contacts(), checked without a device.

contacts_scenes.reference_faces is written from the definitions: shifted slices and argwhere.  That a walk up every line which
records where a run of one id ends and the next begins gives the same tables on every scene and raw volume, and that both give
the values written by hand, is the first test.  Then the invariant, the relation to the reference of disassembly, the report's
methods against their rules restated, the driver over a recording library, the C ABI, the entry point's refusals and the
kernel's resources."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.hip_util import _lib

import contacts_scenes as scenes
import disassembly_scenes as dis_scenes
from contacts_scenes import SCENES, NAMES, MINE, FROM_DISASSEMBLY, RAW_NAMES, reference, raw_reference, scene, EMPTY, NONE, NZ

con = sys.modules["codecad_amd.contacts"]              # (the package's attribute of that name is the function)
av = sys.modules["codecad_amd.assembly_voxels"]
ac = sys.modules["codecad_amd.assembly_components"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERYTHING = [("scene", name) for name in NAMES] + [("raw", name) for name in RAW_NAMES]


def ref_of(kind, name):
    return reference(name) if kind == "scene" else raw_reference(name)


def report_of(name):
    """A ContactReport over the reference of a scene: the methods are plain host code on the arrays."""
    asm, resolution, instances, corner, step, dims = scene(name)
    ref = reference(name)
    return con.ContactReport(list(instances), corner, step, dims, ref.ids, ref.counts, ref.faces, ref.index_sums, ref.box, ref.witness,
                             ref.exposed, ref.contact_ids, ref.contact_counts, list(ref.patches), ref.labels, 0, 1, 1)


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_a_volume_by_hand():
    """2 x 1 x 4: the line x = 0 reads 0 0 1 ., the line x = 1 reads 1 . 1 0."""
    ids = numpy.array([[[0, 0, 1, 255]], [[1, 255, 1, 0]]], dtype=numpy.uint8)
    faces, sums, box, witness, exposed, contact_ids, contact_counts = scenes.reference_faces(ids, 2)
    assert faces[2].tolist() == [[0, 1], [1, 0]] and faces[0].tolist() == [[0, 1], [0, 0]] and (faces[1] == 0).all()
    assert witness[2, 0, 1].tolist() == [0, 0, 1] and witness[2, 1, 0].tolist() == [1, 0, 2] and witness[0, 0, 1].tolist() == [0, 0, 0]
    assert sums[2, 0, 1].tolist() == [0, 0, 1] and box[0, 0, 1].tolist() == [[0, 0, 0], [0, 0, 0]] and (box[0, 1, 0] == -1).all()
    #                 +x      -x      +y      -y      +z      -z     of part 0, part 1
    assert exposed.tolist() == [[[2, 2], [3, 1]], [[3, 3], [3, 3]], [[1, 2], [1, 2]]]
    assert contact_ids.tolist() == [[[0, 0, 1, 255]], [[1, 255, 1, 0]]] and contact_counts == [3, 3]
    again = scenes.running_faces(ids, 2)
    for a, b in zip((faces, sums, box, witness, exposed), again):
        assert numpy.array_equal(a, b)


@pytest.mark.parametrize("kind,name", EVERYTHING)
def test_the_two_ways_agree_and_the_invariant_holds(kind, name):
    ref = ref_of(kind, name)
    n = len(ref.counts)
    faces, sums, box, witness, exposed = scenes.running_faces(ref.ids, n)
    for got, want, dtype in ((faces, ref.faces, numpy.uint64), (sums, ref.index_sums, numpy.uint64), (box, ref.box, numpy.int32),
                             (witness, ref.witness, numpy.int32), (exposed, ref.exposed, numpy.uint64)):
        assert got.dtype == want.dtype == dtype and numpy.array_equal(got, want)
    assert ref.faces.shape == (3, n, n) and ref.index_sums.shape == (3, n, n, 3) and ref.box.shape == (3, n, n, 2, 3)
    assert ref.witness.shape == (3, n, n, 3) and ref.exposed.shape == (3, 2, n)
    assert not ref.faces[:, numpy.arange(n), numpy.arange(n)].any()                 # the diagonal is empty
    empty = ref.faces == 0
    assert ((ref.witness == -1).all(axis=-1) == empty).all() and ((ref.box == -1).all(axis=(-1, -2)) == empty).all()
    # ONE INVARIANT: both sides count the maximal runs of i along the lines of a
    f = ref.faces.astype(numpy.int64)
    upper, lower = ref.exposed[:, 0].astype(numpy.int64) + f.sum(axis=2), ref.exposed[:, 1].astype(numpy.int64) + f.sum(axis=1)
    assert numpy.array_equal(upper, lower)
    for axis in range(3):                                                           # ... restated: the runs, counted directly
        lines = numpy.moveaxis(ref.ids, axis, 0)
        starts = numpy.concatenate([numpy.ones((1,) + lines.shape[1:], bool), lines[1:] != lines[:-1]])
        assert upper[axis].tolist() == [int((starts & (lines == i)).sum()) for i in range(n)]
    # the interface samples, restated: a face of some pair lies on them
    touched = numpy.zeros(ref.ids.shape, bool)
    for axis in range(3):
        lo, hi = scenes._along(axis, slice(None, -1)), scenes._along(axis, slice(1, None))
        pair = (ref.ids[lo] != EMPTY) & (ref.ids[hi] != EMPTY) & (ref.ids[lo] != ref.ids[hi])
        touched[lo] |= pair
        touched[hi] |= pair
    assert numpy.array_equal(ref.contact_ids, numpy.where(touched, ref.ids, EMPTY)) and sum(ref.contact_counts) == int(touched.sum())
    assert ((ref.labels == NONE) == (ref.contact_ids == EMPTY)).all()
    assert all(len(p.parts) >= 2 and p.count >= 2 for p in ref.patches)            # a patch is two samples thick at the least
    at = numpy.argwhere(~empty)
    for axis, i, j in at[:: max(1, len(at) // 50)]:                                 # a witness is a sample of i with one of j right above
        p = ref.witness[axis, i, j].copy()
        assert ref.ids[tuple(p)] == i and (ref.box[axis, i, j, 0] <= p).all() and (p <= ref.box[axis, i, j, 1]).all()
        p[axis] += 1
        assert ref.ids[tuple(p)] == j


@pytest.mark.parametrize("name", list(MINE))
def test_the_values_by_hand_hold(name):
    sc, ref = SCENES[name], reference(name)
    assert tuple(int(d) for d in scene(name)[5]) == tuple(sc.scene.frame) == ref.ids.shape
    assert sc.by_hand and all(c > 0 for c in ref.counts)
    for (axis, i, j), (count, (lo, hi), p) in sc.by_hand.items():
        assert int(ref.faces[axis, i, j]) == count and ref.box[axis, i, j].tolist() == [list(lo), list(hi)], (axis, i, j)
        assert tuple(ref.witness[axis, i, j].tolist()) == tuple(p), (axis, i, j)
    for (axis, side, i), count in sc.exposed.items():
        assert int(ref.exposed[axis, side, i]) == count, (axis, side, i)
    assert [p.parts for p in ref.patches] == sc.patches
    report = report_of(name)
    assert report.groups() == sc.groups and report.loose() == sc.loose


def test_the_scenarios_hold_what_they_are_for():
    stack = reference("stack_z")
    assert av.volume_shape(stack.ids.shape, 2 ** 32)[2] == 144 > NZ == 138 and NZ % 16 != 0
    assert [int(stack.witness[2, k, k + 1, 2]) for k in range(3)] == [63, 127, NZ - 2]
    border = reference("border")
    assert all(border.exposed[a, s, 1] > 0 for a in range(3) for s in range(2)) and not border.exposed[:, :, 0].any()
    three = reference("three")
    assert len(three.patches) == 1 and three.patches[0].parts == (0, 1, 2)
    two = reference("two_patches")
    assert [p.parts for p in two.patches] == [(0, 1), (0, 1)] and len(report_of("two_patches").pairs()) == 1
    for name, axis in (("slabs64_x", 0), ("slabs64_z", 2)):
        ref = reference(name)
        i, j = numpy.indices((64, 64))
        assert numpy.array_equal(ref.faces[axis], numpy.where(j == i + 1, 16, 0)) and not ref.faces[[a for a in range(3) if a != axis]].any()
        assert report_of(name).groups() == [list(range(64))]
    every = raw_reference("every_pair")
    assert scenes.unordered_pairs(every.faces)[:, ~numpy.eye(64, dtype=bool)].all()         # every pair on every axis
    assert every.ids.shape == scenes.RAW_SHAPE == (5, 7, 130) and set(numpy.unique(every.ids).tolist()) == set(range(64)) | {EMPTY}
    rand = raw_reference("random")
    assert set(numpy.unique(rand.ids).tolist()) == set(range(64)) | {EMPTY} and rand.exposed.all() and len(rand.patches) >= 1
    one = raw_reference("one_id")
    assert not one.faces.any() and (one.contact_ids == EMPTY).all() and one.patches == [] and one.exposed[:, :, 7].all()
    assert [scenes.raw_ids(name).shape for name in ("one_sample", "one_line_65", "3x1x16", "1x3x17")] == [(1, 1, 1), (1, 1, 65), (3, 1, 16), (1, 3, 17)]
    assert raw_reference("one_sample").exposed[:, :, 0].tolist() == [[1, 1]] * 3
    assert all(raw_reference(name).faces.any() for name in ("one_line_65", "3x1x16", "1x3x17"))


@pytest.mark.parametrize("name", FROM_DISASSEMBLY)
def test_a_face_is_a_distance_of_one(name):
    ref, other = reference(name), dis_scenes.reference(name)
    touching = ref.faces > 0
    assert numpy.array_equal(touching, other.distance == 1)
    assert numpy.array_equal(ref.witness[touching], other.witness[touching])
    report = report_of(name)
    dis = sys.modules["codecad_amd.disassembly"].DisassemblyReport(report.instances, report.corner, report.step, report.dims, other.ids,
                                                                  other.counts, other.distance, other.witness, 0, 1)
    for axis in range(3):
        assert dis.contacts(axis) == [(int(i), int(j)) for i, j in numpy.argwhere(ref.faces[axis] > 0)]


# ---- the report's methods ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_every_method_follows_its_rule(name):
    report, ref = report_of(name), reference(name)
    n = len(ref.counts)
    step, corner = float(numpy.float32(report.step)), [float(c) for c in report.corner]
    f = ref.faces.astype(object)                                                    # Python ints
    both = f + numpy.swapaxes(f, 1, 2)
    graph = both.sum(axis=0) > 0
    todo = range(n) if n <= 8 else sorted({0, 1, n // 2, n - 2, n - 1})
    for i in todo:
        assert report.touching(i) == [j for j in range(n) if graph[i, j]]
        assert report.exposed_area(i) == int(ref.exposed[:, :, i].sum()) * step ** 2
        assert report.surface_area(i) == (int(ref.exposed[:, :, i].sum()) + int(both[:, i].sum())) * step ** 2
        for j in todo:
            assert report.area(i, j) == int(both[:, i, j].sum()) * step ** 2 == report.area(j, i)
            assert report.normal(i, j) == tuple(int(f[a, i, j] - f[a, j, i]) for a in range(3)) == tuple(-v for v in report.normal(j, i))
            assert all(type(v) is int for v in report.normal(i, j))
            for axis in range(3):
                assert report.projected_area(i, j, axis) == int(both[axis, i, j]) * step ** 2
            if i == j or not graph[i, j]:
                assert report.centroid(i, j) is None
                continue
            centres = []                                                            # every face centre, one by one
            for axis in range(3):
                for a, b in ((i, j), (j, i)):
                    at = numpy.argwhere((ref.ids[scenes._along(axis, slice(None, -1))] == a) & (ref.ids[scenes._along(axis, slice(1, None))] == b))
                    half = numpy.zeros(3)
                    half[axis] = 0.5
                    centres += [at + half] if len(at) else []
            mean = numpy.concatenate(centres).mean(axis=0)
            got = report.centroid(i, j)
            assert tuple(got) == tuple(report.centroid(j, i))
            assert numpy.allclose(tuple(got), [corner[k] + step * mean[k] for k in range(3)], rtol=0, atol=1e-9)
    assert report.pairs() == [(i, j) for i in range(n) for j in range(i + 1, n) if graph[i, j]]
    assert report.loose() == [i for i in range(n) if not graph[i].any()]
    groups = report.groups()
    assert sorted(k for g in groups for k in g) == list(range(n)) and [g[0] for g in groups] == sorted(g[0] for g in groups)
    assert all(g == sorted(g) for g in groups)
    for g in groups:                                                                # closed under touching, and connected
        assert all(set(report.touching(i)) <= set(g) for i in g)
        reached, grew = {g[0]}, True
        while grew:
            more = {j for i in reached for j in report.touching(i)} - reached
            reached, grew = reached | more, bool(more)
        assert sorted(reached) == g
    for patch in report.patches:
        assert report.mask(patch).sum() == patch.count and set(numpy.unique(ref.contact_ids[report.mask(patch)])) == set(patch.parts)


def test_the_centroid_by_hand_and_the_refusals_of_the_methods():
    face = report_of("face_x")
    step, corner = float(face.step), [float(c) for c in face.corner]
    assert face.area(0, 1) == 30 * step ** 2 == face.projected_area(0, 1, 0) and face.projected_area(0, 1, 2) == 0.0
    assert face.normal(0, 1) == (30, 0, 0) and face.normal(1, 0) == (-30, 0, 0)
    assert tuple(face.centroid(0, 1)) == (corner[0] + step * 3.5, corner[1] + step * 2.0, corner[2] + step * 2.5)
    assert face.surface_area(0) == 2 * (4 * 5 + 4 * 6 + 5 * 6) * step ** 2 and face.exposed_area(0) == (2 * (20 + 24 + 30) - 30) * step ** 2
    loose = report_of("loose")
    assert loose.centroid(0, 2) is None and loose.touching(2) == [] and loose.pairs() == [(0, 1)] and loose.area(0, 2) == 0.0
    for bad in (2, -1, True, 0.0, "0", None, [0, 1]):
        for call in (lambda b: face.area(b, 0), lambda b: face.area(0, b), lambda b: face.normal(b, 0), lambda b: face.centroid(0, b),
                     lambda b: face.touching(b), lambda b: face.surface_area(b), lambda b: face.exposed_area(b),
                     lambda b: face.projected_area(b, 0, 0)):
            with pytest.raises(ValueError):
                call(bad)
    for bad in (3, -1, True, None, "x", 1.0):
        with pytest.raises(ValueError, match="axis"):
            face.projected_area(0, 1, bad)


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals():
    one = cc.assembly("one", [shapes.sphere(r=1).make_part("ball")])
    with pytest.raises(ValueError):
        cc.contacts(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.contacts(one, -1)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.contacts(one, 0.125, max_bytes=5 * 16 * 16 * 16 - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.contacts(one, 0.125, patches=False, max_bytes=2 * 16 * 16 * 16 - 1)
    with pytest.raises(ValueError, match="64"):
        cc.contacts(cc.assembly("many", [shapes.box(1).make_part("b%d" % k).translated_x(2 * k) for k in range(65)]), 0.5)
    assert {"contacts", "ContactReport"} <= set(cc.__all__) and "contacts(" in cc.__doc__
    doc = con.__doc__
    for word in ("FACE", "CONTACT", "EXPOSED", "INTERFACE SAMPLES", "PATCHES", "ONE INVARIANT", "TWO SAMPLES THICK", "more\n    than two parts",
                 "sqrt(3)", "OUT OF SCOPE", "clearance", "26 neighbours", "2D assemblies"):
        assert word in doc, word


def test_no_visible_instance_gives_the_empty_report():
    for patches, least in ((True, 5 * 16), (False, 2 * 16)):
        report = cc.contacts(dis_scenes.empty_assembly(), 0.1, patches=patches, max_bytes=least)
        assert report.instances == [] and report.counts == [] and report.traversals == 0 and report.samples_evaluated == 0
        assert report.faces.shape == (3, 0, 0) and report.faces.dtype == numpy.uint64 and report.index_sums.shape == (3, 0, 0, 3)
        assert report.box.shape == (3, 0, 0, 2, 3) and report.box.dtype == numpy.int32 and report.witness.shape == (3, 0, 0, 3)
        assert report.exposed.shape == (3, 2, 0) and report.exposed.dtype == numpy.uint64 and report.contact_counts == []
        assert report.part_ids.shape == (1, 1, 1) == report.contact_ids.shape == report.labels.shape
        assert report.contact_ids[0, 0, 0] == 255 and report.labels[0, 0, 0] == NONE and report.labels.dtype == numpy.uint32
        assert report.patches == [] and report.component_capacity_runs == 0
        assert report.pairs() == [] and report.groups() == [] and report.loose() == []
        with pytest.raises(ValueError):
            cc.contacts(dis_scenes.empty_assembly(), 0.1, patches=patches, max_bytes=least - 1)


def fake_device(monkeypatch, rows, counts):
    """contacts() over a library that records its calls and tables that read back as `rows` and `counts`."""
    calls = []

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x100000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            calls.append(("read", self.device_ptr))
            if self.dtype == con._ROW:
                return rows.copy()
            if self.dtype == ac._ROW:
                return numpy.zeros(self.shape, self.dtype)                          # the counter reads 0: no patch
            return counts.copy() if self.dtype == numpy.uint64 else numpy.full(self.shape, 1, self.dtype)

        def release(self):
            calls.append(("release", self.device_ptr))

    class Lib:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name, args))
                return 0
            return call

    def traverse(inst, top, side, c, s, d, initial_capacity, **kwargs):
        calls.append(("traverse", initial_capacity, kwargs["cells_extra"][0]))
        return 77, numpy.array([5, 6, 7, 999], dtype=numpy.uint64), 2

    manager = types.SimpleNamespace(lib=Lib(), queue=types.SimpleNamespace(handle=0x99))
    for module in (av, ac, con):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


def tables():
    rows = numpy.zeros((3, 64, 64), con._ROW)
    rows[0, 0, 1] = (2, (3, 9, 121), ~numpy.uint64(1 << 32 | 4 << 16 | 60), (~numpy.uint32(1), ~numpy.uint32(4), ~numpy.uint32(60)), (2, 5, 61))
    rows[2, 2, 0] = (1 << 40, (1 << 50, 2, 3), ~numpy.uint64(65535 << 32 | 40000 << 16 | 7), (~numpy.uint32(65535), ~numpy.uint32(40000), ~numpy.uint32(7)),
                     (65535, 65535, 9))
    rows[1, 5, 6]["count"] = 1                                                      # beyond n = 3: never looked at
    counts = numpy.arange(7 * 64, dtype=numpy.uint64).reshape(7, 64)
    return rows, counts


def test_the_driver_sets_each_table_once_and_launches_once(monkeypatch):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    calls = fake_device(monkeypatch, *tables())
    report = cc.contacts(asm, resolution, initial_capacity=7, initial_components=3, max_bytes=5 * 14 * 10 * 144)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names[:4] == ["buffer", "hu_memset", "traverse", "read"]                 # the ids, as assembly_voxels() leaves them
    assert names[4:16] == ["buffer", "hu_memset", "buffer", "hu_memset", "buffer", "hu_contact_faces", "read", "read", "read",
                           "release", "release", "release"]
    assert names[16:] == ["buffer", "hu_components_local", "hu_components_merge", "hu_components_flatten", "buffer", "hu_memset",
                          "hu_components_stats", "read", "release", "release", "hu_components_finish", "read", "release"]
    assert names.count("hu_contact_faces") == 1 and names.count("hu_memset") == 4 and "hu_stream_synchronize" not in names
    assert calls[2][1:] == (7, 1)                                                   # retire=True, the cell lists' capacity
    ids, rows, acc, contact = 0x100000, 0x200000, 0x300000, 0x400000
    assert calls[4][1:] == (con._ROW, (3, 64, 64)) and calls[5][1] == (rows, 0, 3 * 64 * 64 * 64, 0x99)
    assert calls[6][1:] == (numpy.dtype(numpy.uint64), (7, 64)) and calls[7][1] == (acc, 0, 7 * 64 * 8, 0x99)
    assert calls[8][1:] == (numpy.dtype(numpy.uint8), (14, 10, 144))
    launch = calls[9][1]
    #      ids, contact ids, rows, counts | pitch, n, stream
    assert launch[:4] + launch[5:] == (ids, contact, rows, acc, 144, 3, 0x99) and list(launch[4]) == [14, 10, 138]
    assert [c[1] for c in calls[10:16]] == [rows, acc, contact, ids, rows, acc]     # both tables read once, the ids released
    assert calls[17][1][0] == contact and calls[17][1][4:6] == (1, 1)               # the contact volume is labelled: solid, local
    assert calls[25] == ("release", contact)                                        # ... and released by the labelling
    assert report.faces.shape == (3, 3, 3) and report.faces.dtype == numpy.uint64 and int(report.faces.astype(object).sum()) == 2 + (1 << 40)
    assert report.index_sums[0, 0, 1].tolist() == [3, 9, 121] and report.index_sums[2, 2, 0].tolist() == [1 << 50, 2, 3]
    assert report.box[0, 0, 1].tolist() == [[1, 4, 60], [2, 5, 61]] and report.box[2, 2, 0].tolist() == [[65535, 40000, 7], [65535, 65535, 9]]
    assert report.witness[0, 0, 1].tolist() == [1, 4, 60] and report.witness[2, 2, 0].tolist() == [65535, 40000, 7]
    assert (report.witness[report.faces == 0] == -1).all() and (report.box[report.faces == 0] == -1).all()
    assert report.box.dtype == report.witness.dtype == numpy.int32 and report.exposed.dtype == numpy.uint64
    assert report.exposed.tolist() == [[[64 * (2 * a + s) + i for i in range(3)] for s in range(2)] for a in range(3)]
    assert report.contact_counts == [384, 385, 386] and all(type(v) is int for v in report.contact_counts)
    assert report.counts == [5, 6, 7] and report.traversals == 2 and report.samples_evaluated == 77
    assert report.part_ids.shape == (14, 10, 138) == report.contact_ids.shape == report.labels.shape and len(report.instances) == 3
    assert report.patches == [] and report.component_capacity_runs == 1 and report.pairs() == [(0, 1), (0, 2)]


def test_without_patches_nothing_is_labelled(monkeypatch):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    calls = fake_device(monkeypatch, *tables())
    report = cc.contacts(asm, resolution, patches=False, max_bytes=2 * 14 * 10 * 144)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names[4:] == ["buffer", "hu_memset", "buffer", "hu_memset", "buffer", "hu_contact_faces", "read", "read", "read",
                         "release", "release", "release", "release"]
    assert report.patches == [] and (report.labels == NONE).all() and report.labels.dtype == numpy.uint32 and report.component_capacity_runs == 0
    assert report.labels.shape == (14, 10, 138) and report.witness[0, 0, 1].tolist() == [1, 4, 60]


def test_max_bytes_counts_five_bytes_a_sample_or_two_before_any_call(monkeypatch):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    calls = fake_device(monkeypatch, *tables())
    with pytest.raises(ValueError, match="max_bytes"):
        cc.contacts(asm, resolution, max_bytes=5 * 14 * 10 * 144 - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.contacts(asm, resolution, patches=False, max_bytes=2 * 14 * 10 * 144 - 1)
    with monkeypatch.context() as m:
        m.setattr(con, "_check_entries", lambda dims: (_ for _ in ()).throw(ValueError("entries")))
        with pytest.raises(ValueError, match="entries"):
            cc.contacts(asm, resolution)                                            # the label volume's own refusal, with patches only
    assert calls == []
    cc.contacts(dis_scenes.empty_assembly(), 0.1)
    cc.contacts(dis_scenes.empty_assembly(), 0.1, patches=False)
    assert calls == []                                                              # nothing visible: nothing launched


# ---- the C ABI, the entry point's refusals and the kernel's resources -------------------------------------------------

def test_abi_of_the_new_entry_point():
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    name = "hu_contact_faces"
    assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto)
    assert [" ".join(a.split()) for a in proto.split(",")] == ["const void* ids_dev", "void* contact_ids_dev", "void* rows_dev", "uint64_t* counts_dev",
                                                              "const uint32_t dims[3]", "uint32_t pitch", "uint32_t n", "void* stream"]
    assert len(_lib.PROTOTYPES[name]) == 8 and _lib.PROTOTYPES[name][4] is _lib.PROTOTYPES["hu_blocking_lines"][2]       # dims
    assert _lib.PROTOTYPES[name][5] is ctypes.c_uint32 and _lib.PROTOTYPES[name][6] is ctypes.c_uint32
    assert ("int %s(" % name) in integration and "hu_contact_row" in integration
    assert int(re.search(r"#define HU_CONTACT_MAX_PARTS (\d+)", header).group(1)) == con.MAX_PARTS == con._ROWS[1] == con._ROWS[2] == 64
    # the row: 64 bytes, the fields of the header in the header's order
    struct = re.search(r"typedef struct hu_contact_row \{(.*?)\} hu_contact_row;", header, re.S).group(1)
    fields = re.findall(r"(uint64_t|uint32_t) (\w+)(?:\[(\d+)\])?;", struct)
    assert [(f[1], {"uint64_t": "<u8", "uint32_t": "<u4"}[f[0]], int(f[2] or 1)) for f in fields] == \
        [(nm, con._ROW[nm].base.str, int(numpy.prod(con._ROW[nm].shape, dtype=int))) for nm in con._ROW.names]
    assert con._ROW.itemsize == 64 and con._ROW.names == ("count", "sums", "not_key", "not_lo", "hi")
    assert [con._ROW.fields[nm][1] for nm in con._ROW.names] == [0, 8, 32, 40, 52] and con._COUNTS == (7, 64)


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def faces(ids=p, contact=p, rows=p, counts=p, dims=d(4, 4, 4), pitch=16, n=2):
        return lib.hu_contact_faces(ids, contact, rows, counts, dims, pitch, n, None)

    refused = [faces(ids=None), faces(rows=None), faces(counts=None), faces(dims=None), faces(rows=p + 4), faces(rows=p + 1), faces(counts=p + 4),
               faces(counts=p + 2), faces(pitch=24), faces(pitch=0), faces(pitch=8), faces(dims=d(4, 4, 17)), faces(dims=d(0, 4, 4)),
               faces(dims=d(4, 0, 4)), faces(dims=d(4, 4, 0)), faces(dims=d(65537, 4, 4)), faces(dims=d(4, 65537, 4)), faces(n=0), faces(n=65),
               faces(contact=None, n=0), faces(contact=None, rows=None), faces(pitch=65536 + 16, dims=d(1, 1, 65537))]
    assert refused == [-3] * len(refused)
    assert faces(n=65) == -3 and b"n must" in lib.hu_last_error()
    assert faces(pitch=24) == -3 and b"16" in lib.hu_last_error()
    assert faces(rows=p + 4) == -3 and b"aligned" in lib.hu_last_error()
    assert faces(counts=p + 4) == -3 and b"aligned" in lib.hu_last_error()
    assert faces(ids=None) == -3 and b"NULL" in lib.hu_last_error()


def test_the_kernel_uses_no_scratch_no_lds_and_the_registers_the_design_states(tmp_path):
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, no LDS, and the VGPR
    count written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_contacts.hip" in builder.SOURCES and "instance_contacts.hip" not in builder.FLAGGED_SOURCES
    with open(os.path.join(builder.CSRC, "instance_contacts.hip")) as f:
        assert '#include "id_volume.hpp"' in f.read()
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        stated = re.search(r"`k_contact_faces` (\d+) VGPRs and (\d+) B of LDS", f.read())
    assert stated, "DESIGN.md section 9 states the VGPRs and the LDS of k_contact_faces"
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_contacts.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_contacts.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    blocks = metadata.split("\n  - .agpr_count:")[1:]
    assert len(blocks) == 1
    block = blocks[0]
    assert re.search(r"\.name:\s+\S*15k_contact_facesENS_11ContactArgsE", block)
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)) == 0 == int(stated.group(2))
    assert int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)) == int(stated.group(1))
