"""The references and the scenarios of test_gpu_islands.py, and the host side of islands(), checked without a device.

islands_scenes.grounded_set is written from the definition: seeds, then growth by shifted arrays to the fixed point.  That the
layer-by-layer restatement gives the same set on every scene, direction and raw volume, that the consequences the module's
docstring lists hold, that A = F & O against the overhangs reference, that G is the escape set of the complemented volume where
the two definitions meet, and that all give the values written by hand, come first.  Then the driver over a recording library,
the C ABI, the entry points' refusals and the kernels' resources."""
import ctypes
import os
import re
import sys
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.hip_util import _lib

import disassembly_scenes as dis_scenes
import drainage_scenes
import overhangs_scenes
import reach_kernels as reach
import islands_scenes as scenes
from islands_scenes import SCENES, MINE, CASES, RAW_CASES, DIRECTIONS, reference, raw_reference, scene, shifted, EMPTY, NONE, SOLID

isl = sys.modules["codecad_amd.islands"]               # (the package's attribute of that name is the function)
av = sys.modules["codecad_amd.assembly_voxels"]
ac = sys.modules["codecad_amd.assembly_components"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hu_ground_layers", "hu_ground_seed", "hu_ground_mark")
KERNELS = ("k_ground_seed", "k_ground_mark<false>", "k_ground_mark<true>")
EVERYTHING = [("scene",) + c for c in CASES] + [("raw",) + c for c in RAW_CASES]


def ref_of(kind, name, axis, up, of):
    return reference(name, axis, up, of) if kind == "scene" else raw_reference(name, axis, up, of)


def labels_of(kind, name, axis, of):
    return scenes.labels_of(name, axis, of) if kind == "scene" else scenes.raw_labels(name, axis, of)


# ---- the references ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,axis,up,of", EVERYTHING)
def test_the_two_ways_agree_and_the_consequences_hold(kind, name, axis, up, of):
    ref = ref_of(kind, name, axis, up, of)
    s, g, f = ref.s, ref.grounded, ref.floating
    sign = 1 if up else -1
    labels = labels_of(kind, name, axis, of)
    assert numpy.array_equal(scenes.layered_grounded(s, axis, up, labels), g)
    assert numpy.array_equal(scenes.synchronous(s, axis, up, s.shape[axis], labels), g)
    assert numpy.array_equal(f, s & ~g) and not (g & ~s).any()
    h = scenes.layers(s.shape, axis, up)
    assert not (f & (h == ref.first_layer)).any() and (not s.any() or (s & (h == ref.first_layer)).any()) and not (s & (h < ref.first_layer)).any()
    assert not (f & shifted(g, axis, sign)).any()                                   # the sample below a floating one is in F or outside S
    for a in range(3):
        if a != axis:                                                               # ... and so are its lateral neighbours
            assert not (f & (shifted(g, a, 1) | shifted(g, a, -1))).any()
    # F and G touch only where a sample of G lies directly above one of F
    touching = numpy.zeros(s.shape, dtype=bool)
    for a in range(3):
        for d in (1, -1):
            touching |= f & shifted(g, a, d)
    j = ref.join_ids != EMPTY
    assert numpy.array_equal(touching, j) and numpy.array_equal(j, f & shifted(g, axis, -sign))
    # the starts are the floating overhangs of reach 0, and every island holds one
    started = ref.start_ids != EMPTY
    h0, o = overhangs_scenes.overhang_set(s, axis, up, 0)
    assert h0 == ref.first_layer and numpy.array_equal(started, f & o)
    for v, m, c in ((ref.floating_ids, f, ref.floating_counts), (ref.start_ids, started, ref.start_counts), (ref.join_ids, j, ref.join_counts)):
        assert numpy.array_equal(v, numpy.where(m, ref.ids, EMPTY)) and sum(c) == int(m.sum())
    assert ((ref.labels == NONE) == ~f).all() and sum(i.expected.count for i in ref.islands) == int(f.sum())
    for i in ref.islands:
        mask = ref.labels == i.expected.label
        assert i.starts >= 1 and i.starts == int((started & mask).sum()) and i.loose == (not (j & mask).any())
        assert i.first_layer == int(h[mask].min()) > ref.first_layer


@pytest.mark.parametrize("name", scenes.BOTH_SETS)
def test_the_raw_volumes_hold_both_sets_and_the_duality_with_drainage(name):
    ids = scenes.raw_ids(name)
    of = scenes.RAW_OF.get(name, SOLID)
    for axis, up in DIRECTIONS:
        ref = raw_reference(name, axis, up, of)
        assert ref.floating.any() and ref.grounded.any() and (ref.join_ids != EMPTY).any(), (name, axis, up)
        # S kept off the lateral borders, h0 = 0: grounding is the drainage of the complemented volume
        s = scenes.in_set_of(ids, of).copy()
        for a in range(3):
            if a != axis:
                edge = [slice(None)] * 3
                for at in (0, -1):
                    edge[a] = at
                    s[tuple(edge)] = False
        if scenes.first_layer(s, axis, up) == 0:
            assert numpy.array_equal(scenes.grounded_set(s, axis, up), drainage_scenes.escape_set(s, axis, up)), (name, axis, up)
        else:
            assert name == "raised" and axis != 1


@pytest.mark.parametrize("name", list(MINE))
def test_the_values_by_hand_hold(name):
    sc = SCENES[name]
    assert tuple(int(d) for d in scene(name)[5]) == tuple(sc.frame) == scenes.part_ids(name).shape
    assert set(sc.floating) <= set(sc.runs)
    for (axis, up, of), samples in sc.floating.items():
        want = numpy.zeros(sc.frame, dtype=bool)
        for p in samples:
            want[p] = True
        assert numpy.array_equal(reference(name, axis, up, of).floating, want), (name, axis, up, of)


def test_the_peg_the_arch_and_the_ball_by_hand():
    peg = reference("peg", 2, True)
    assert peg.floating_counts == [0, 136] and peg.start_counts == [0, 4] and peg.join_counts == [0, 4] and peg.first_layer == 0
    (island,) = peg.islands
    assert tuple(island.expected) == (((6 * 10 + 4) * scenes.NZ + 100), 136, ((6, 4, 100), (7, 5, 133)), (6.5 * 136, 4.5 * 136, 116.5 * 136),
                                      False, (1,))
    assert (island.first_layer, island.starts, island.loose) == (100, 4, False)
    assert (peg.start_ids[6:8, 4:6, 100] == 1).all() and (peg.join_ids[6:8, 4:6, 133] == 1).all() and peg.join_ids[6, 4, 132] == EMPTY
    assert reference("peg", 2, False).islands == [] and reference("peg", 2, False).first_layer == 0
    arch = reference("arch", 2, True)
    assert arch.floating_counts == [80] and arch.start_counts == [8] and arch.join_counts == [8]
    (island,) = arch.islands
    assert island.expected.box == ((10, 0, 6), (11, 3, 15)) and (island.first_layer, island.starts, island.loose) == (6, 8, False)
    for axis, up in DIRECTIONS:
        ball = reference("ball_captive", axis, up)
        assert ball.floating_counts == [0, 8] and ball.start_counts == [0, 4] and ball.join_counts == [0, 0]
        (island,) = ball.islands
        assert island.loose and island.starts == 4 and island.first_layer == 4 and island.expected.parts == (1,)
        assert island.expected.box == ((4, 4, 4), (5, 5, 5))
    resting = reference("ball_resting", 2, False)
    # downwards the resting ball is laid before the floor it rests on, and held when that floor is laid over it
    assert resting.floating_counts == [0, 8] and resting.join_counts == [0, 4] and not resting.islands[0].loose
    assert resting.islands[0].first_layer == 10 - 1 - 2


def test_the_scenarios_hold_what_they_are_for():
    assert av.volume_shape(scenes.PEG, 2 ** 32)[2] == 144 and scenes.NZ % 16 != 0 and scenes.NZ % 64 != 0
    firsts = reference("firsts", 2, True)
    assert sorted(i.first_layer for i in firsts.islands) == [63, 64, 65] and all(i.loose for i in firsts.islands)
    up, down = reference("join_up", 2, True), reference("join_down", 2, False)
    assert (up.join_ids[8:10, :, 63] == 0).all() and up.grounded[8, 0, 64] and int((up.join_ids != EMPTY).sum()) == 8
    assert (down.join_ids[8:10, :, 64] == 0).all() and down.grounded[8, 0, 63] and int((down.join_ids != EMPTY).sum()) == 8
    # the zigzag needs many handovers: one synchronous step does not reach the fixed point, in either direction of z
    for direction in (True, False):
        s = scenes.part_ids("zigzag") != EMPTY
        assert not numpy.array_equal(scenes.synchronous(s, 2, direction, 1, scenes.labels_of("zigzag", 2)), s)
        assert reference("zigzag", 2, direction).grounded.all() or numpy.array_equal(reference("zigzag", 2, direction).grounded, s)
    # the plate's layer component crosses tile faces on both lateral axes
    plate = scenes.labels_of("plate", 2)[:, :, 3]
    assert len(numpy.unique(plate)) == 1 and plate.shape[0] > 2 * ac.TILE[0] and plate.shape[1] > 2 * ac.TILE[1]
    # part 1 alone starts at layer 3; its second body starts at layer 5 and floats
    raised = reference("raised", 2, True, 1)
    assert raised.first_layer == 3 and [i.first_layer for i in raised.islands] == [5] and raised.islands[0].loose
    feet = reference("feet", 2, True, 1)
    assert feet.first_layer == 2 and [(i.first_layer, i.loose, i.starts) for i in feet.islands] == [(4, False, 8)]
    assert reference("feet", 2, True).islands == []
    ball = reference("ball_over_slab", 2, True)
    assert len(ball.floating_counts) == 3
    assert all(reference("nothing", axis, up).islands == [] for axis, up in DIRECTIONS)
    edge = [reference("edge", axis, up) for axis, up in DIRECTIONS]
    assert [len(r.islands) for r in edge] == [1, 1, 0, 0, 1, 1] and all(i.loose for r in edge for i in r.islands)


@pytest.mark.parametrize("kind,name", sorted({c[:2] for c in EVERYTHING}))
def test_down_an_axis_is_up_the_flipped_volume(kind, name):
    for axis, up, of in sorted({c[2:] for c in EVERYTHING if c[:2] == (kind, name) and not c[3]}, key=str):
        down = ref_of(kind, name, axis, False, of)
        n = len(down.floating_counts)
        flipped = scenes.reference_of(numpy.ascontiguousarray(numpy.flip(down.ids, axis)), n, axis, True, of)
        for field in ("floating_ids", "start_ids", "join_ids"):
            assert numpy.array_equal(numpy.flip(getattr(flipped, field), axis), getattr(down, field)), field
        assert flipped.floating_counts == down.floating_counts and len(flipped.islands) == len(down.islands)
        assert flipped.first_layer == down.first_layer


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals_and_exports():
    one = cc.assembly("one", [shapes.sphere(r=1).make_part("ball")])
    with pytest.raises(ValueError):
        cc.islands(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.islands(one, -1)
    for bad in (3, -1, True, None, "z", 2.0):
        with pytest.raises(ValueError, match="axis"):
            cc.islands(one, 0.125, axis=bad)
    for bad in (1, -1, True, None, "empty_space", 0.0):
        with pytest.raises(ValueError, match="of must be"):
            cc.islands(one, 0.125, of=bad)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.islands(one, 0.125, max_bytes=8 * 16 * 16 * 16 - 1)
    with pytest.raises(ValueError, match="64"):
        cc.islands(cc.assembly("many", [shapes.box(1).make_part("b%d" % k).translated_x(2 * k) for k in range(65)]), 0.5)
    with pytest.raises(ValueError, match="2\\^31"):
        isl._check_flag((32768, 4096, 16), False)
    isl._check_flag((32768, 4096, 16), True)
    isl._check_flag((32768, 4096, 15), True)
    assert {"islands", "IslandReport", "Island"} <= set(cc.__all__) and "islands(" in cc.__doc__ and isl.SAMPLE_BYTES == 8
    assert cc.islands is isl.islands and cc.Island is isl.Island and cc.IslandReport is isl.IslandReport
    assert isl.IslandReport._fields == ("instances", "corner", "step", "dims", "of", "axis", "up", "first_layer", "part_ids", "floating_ids",
                                        "start_ids", "join_ids", "floating_counts", "start_counts", "join_counts", "floating_volume",
                                        "islands", "labels", "passes", "samples_evaluated", "traversals", "component_capacity_runs")
    assert isl.Island._fields == ac.Component._fields + ("owners", "first_layer", "starts", "loose")
    for word in ("GROUNDED", "FLOATING", "STARTS", "JOINS", "ISLANDS", "OUT OF SCOPE", "lateral reach", "6-neighbourhood", "do not ground each other",
                 "supports of `overhangs()`", "off the lattice axes", "64 instances", "several devices", "retire=True", "reach_sq=0"):
        assert word in isl.__doc__, word
    for module in ("drainage", "overhangs"):                                        # their out-of-scope sentences are still there
        assert "grounded" in sys.modules["codecad_amd." + module].__doc__


def test_no_visible_instance_gives_the_empty_report():
    report = cc.islands(dis_scenes.empty_assembly(), 0.1, axis=0, up=False, max_bytes=8 * 16)
    assert report.instances == [] and report.traversals == 0 and report.samples_evaluated == 0 and report.passes == 0
    assert report.part_ids.shape == (1, 1, 1) == report.floating_ids.shape == report.labels.shape and (report.axis, report.up) == (0, False)
    for v in (report.floating_ids, report.start_ids, report.join_ids):
        assert v[0, 0, 0] == 255 and v.dtype == numpy.uint8
    assert report.labels[0, 0, 0] == NONE and report.labels.dtype == numpy.uint32 and report.first_layer == 1 and report.of == SOLID
    assert report.floating_counts == [] == report.start_counts == report.join_counts and report.floating_volume == 0.0
    assert report.islands == [] and report.component_capacity_runs == 0 and report.grounded
    with pytest.raises(ValueError):
        cc.islands(dis_scenes.empty_assembly(), 0.1, max_bytes=8 * 16 - 1)


def fake_device(monkeypatch, changed, counts):
    """islands() over a library that records its calls; the changed word reads as the values of `changed` in turn."""
    calls, words = [], list(changed)

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x100000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            calls.append(("read", self.device_ptr, self.size))
            if self.dtype == ac._ROW:
                return numpy.zeros(self.shape, self.dtype)                          # the counter reads 0: no island
            if self.shape == (1,):
                return numpy.array([words.pop(0)], dtype=numpy.uint32)
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
    for module in (av, ac, isl):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


@pytest.mark.parametrize("axis,up,of", [(2, True, SOLID), (0, False, 1)])
def test_the_driver_reads_one_word_a_pass_and_labels_the_floating_ids(monkeypatch, axis, up, of):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    counts = numpy.arange(100, 356, dtype=numpy.uint64).reshape(4, 64)
    counts[3, 0] = 138 - 5 if axis == 2 else 14 - 5                                 # the depth word: h0 = 5
    calls = fake_device(monkeypatch, [1, 1, 0], counts)
    report = cc.islands(asm, resolution, axis=axis, up=up, of=of, local=False, initial_capacity=7, initial_components=3,
                        max_bytes=8 * 14 * 10 * 144)
    monkeypatch.undo()
    code = 255 if of == SOLID else of
    names = [c[0] for c in calls]
    assert names[:4] == ["buffer", "hu_memset", "traverse", "read"]                 # the ids, as assembly_voxels() leaves them
    assert names[4:12] == ["buffer", "hu_memset", "buffer", "buffer", "hu_overhang_first_layer", "hu_ground_layers", "hu_components_flatten",
                           "hu_ground_seed"]
    assert names[12:21] == ["hu_memset", "hu_drain_rise", "read"] * 3               # three passes: the third sets nothing
    assert names[21:35] == ["buffer"] * 3 + ["hu_ground_mark"] + ["read"] * 4 + ["release"] * 6
    assert names[35:] == ["buffer", "hu_components_local", "hu_components_merge", "hu_components_flatten", "buffer", "hu_memset",
                          "hu_components_stats", "read", "release", "release", "hu_components_finish", "read", "release"]
    assert "hu_stream_synchronize" not in names and calls[2][1:] == (7, 1)
    ids, acc, word, layers, floating, start, join = (0x100000 * k for k in range(1, 8))
    depth = acc + 8 * 3 * 64
    assert calls[4][1:] == (numpy.dtype(numpy.uint64), (4, 64)) and calls[5][1] == (acc, 0, 2048, 0x99)
    assert calls[6][1:] == (numpy.dtype(numpy.uint32), (1,)) and calls[7][1:] == (numpy.dtype(numpy.uint32), (14, 10, 144))
    first = calls[8][1]
    assert first[:2] + first[3:] == (ids, depth, 144, axis, int(up), code, 0x99) and list(first[2]) == [14, 10, 138]
    launch = calls[9][1]
    assert launch[:2] + launch[3:] == (ids, layers, 144, axis, code, 0, 0x99) and list(launch[2]) == [14, 10, 138]
    assert calls[10][1][0] == layers and calls[11][1][:2] + calls[11][1][3:] == (layers, depth, 144, axis, int(up), 0x99)
    for k in range(3):
        assert calls[12 + 3 * k][1] == (word, 0, 4, 0x99)
        rise = calls[13 + 3 * k][1]
        assert rise[:2] + rise[3:] == (layers, word, 144, axis, int(up), 0x99)
        assert calls[14 + 3 * k] == ("read", word, 4)                               # four bytes a pass
    assert all(c[1:] == (numpy.dtype(numpy.uint8), (14, 10, 144)) for c in calls[21:24])
    mark = calls[24][1]
    assert mark[:6] + mark[7:] == (ids, layers, floating, start, join, acc, 144, axis, int(up), code, 0x99)
    assert [c[1] for c in calls[25:35]] == [floating, start, join, acc, layers, ids, start, join, acc, word]   # one read-back, then all but the floating ids go
    assert calls[36][1][0] == floating and calls[36][1][4:6] == (1, 0)              # the floating ids are labelled: solid, the same arm
    assert calls[44] == ("release", floating)
    n = len(report.instances)
    assert report.passes == 3 and report.first_layer == 5 and report.of == of and (report.axis, report.up) == (axis, up)
    assert report.floating_counts == [100, 101, 102][:n] and report.start_counts == [164, 165, 166][:n] and report.join_counts == [228, 229, 230][:n]
    assert all(type(v) is int for c in (report.floating_counts, report.start_counts, report.join_counts) for v in c) and n == 3
    assert report.floating_volume == 303 * float(report.step) ** 3 and not report.grounded
    assert report.part_ids.shape == (14, 10, 138) == report.floating_ids.shape == report.start_ids.shape == report.join_ids.shape == report.labels.shape
    assert report.islands == [] and report.component_capacity_runs == 1 and report.traversals == 2 and report.samples_evaluated == 77


def test_max_bytes_counts_eight_bytes_a_sample_before_any_launch(monkeypatch):
    asm, resolution = dis_scenes.scene("hooks")[:2]
    calls = fake_device(monkeypatch, [0], numpy.zeros((4, 64), numpy.uint64))
    with pytest.raises(ValueError, match="max_bytes"):
        cc.islands(asm, resolution, max_bytes=8 * 14 * 10 * 144 - 1)
    with pytest.raises(ValueError, match="axis"):
        cc.islands(asm, resolution, axis=3)
    with pytest.raises(ValueError, match="of must be"):
        cc.islands(asm, resolution, of=3)
    with monkeypatch.context() as m:
        m.setattr(isl, "_check_entries", lambda dims: (_ for _ in ()).throw(ValueError("entries")))
        with pytest.raises(ValueError, match="entries"):
            cc.islands(asm, resolution)
    assert calls == []
    cc.islands(dis_scenes.empty_assembly(), 0.1)
    assert calls == []                                                              # nothing visible: nothing launched
    cc.islands(asm, resolution, max_bytes=8 * 14 * 10 * 144)
    assert [c[0] for c in calls].count("hu_ground_mark") == 1


def test_an_island_takes_its_fields_from_its_row_and_the_host_volumes():
    voxels = types.SimpleNamespace(instances=[types.SimpleNamespace(name="a"), types.SimpleNamespace(name="b")], corner=(0.0, 0.0, 0.0),
                                   step=numpy.float32(0.5), dims=(10, 20, 30))
    rows = numpy.zeros(2, ac._ROW)
    rows[0] = (4, (8, 12, 16), 0b10, (~numpy.uint32(1), ~numpy.uint32(2), ~numpy.uint32(3)), (4, 5, 6), 77, 0)
    rows[1] = (2, (2, 2, 2), 0b11, (~numpy.uint32(1), ~numpy.uint32(1), ~numpy.uint32(1)), (1, 1, 1), 30, 0)
    labels = numpy.full((10, 20, 30), NONE, dtype=numpy.uint32)
    labels[1:3, 2, 3] = 77
    labels[4, 5, 6] = 77
    labels[1, 1, 1] = 30
    start_ids, join_ids = (numpy.full((10, 20, 30), EMPTY, dtype=numpy.uint8) for _ in range(2))
    start_ids[1:3, 2, 3] = start_ids[1, 1, 1] = 1
    join_ids[4, 5, 6] = 1
    for axis, up, first in ((2, True, 3), (2, False, 23), (0, True, 1), (0, False, 5), (1, False, 14)):
        small, island = isl._islands(rows, voxels, axis, up, labels, start_ids, join_ids)
        assert (island.label, island.count, island.box, island.parts, island.owners) == (77, 4, ((1, 2, 3), (4, 5, 6)), (1,), ("b",))
        assert (island.first_layer, island.starts, island.loose) == (first, 2, False)
        assert island.volume == 4 * 0.125 and tuple(island.centroid) == (1.0, 1.5, 2.0)
        assert (small.label, small.owners, small.starts, small.loose) == (30, ("a", "b"), 1, True)
    assert isl._islands(rows[:0], voxels, 2, True, labels, start_ids, join_ids) == []


# ---- the C ABI, the entry points' refusals and the kernels' resources --------------------------------------------------

def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    want = {"hu_ground_layers": ["const void* ids_dev", "void* labels_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis", "uint32_t of",
                                 "int local", "void* stream"],
            "hu_ground_seed": ["void* labels_dev", "const uint32_t* word_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis", "int up",
                               "void* stream"],
            "hu_ground_mark": ["const void* ids_dev", "const void* labels_dev", "void* floating_dev", "void* start_dev", "void* join_dev",
                               "uint64_t* counts_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis", "int up", "uint32_t of", "void* stream"]}
    assert tuple(want) == ENTRY_POINTS
    for name, args in want.items():
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == args
        assert len(_lib.PROTOTYPES[name]) == len(args)
        dims = args.index("const uint32_t dims[3]")
        assert _lib.PROTOTYPES[name][dims] is _lib.PROTOTYPES["hu_components_flatten"][1] and _lib.PROTOTYPES[name][dims + 1] is ctypes.c_uint32
        assert ("int %s(" % name) in integration
    section = integration[integration.index("### What a print starts in mid-air"):]                   # the call order, in its section
    order = [section.index(word) for word in ("Call `hu_overhang_first_layer`", "`hu_ground_layers`,", "`hu_components_flatten`,",
                                              "`hu_ground_seed` once", "call `hu_drain_rise`", "then `hu_ground_mark`")]
    assert order == sorted(order)
    assert int(re.search(r"#define HU_ABI_VERSION (\d+)", header).group(1)) == 3 == lib.hu_abi_version()    # additive: the version stayed


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def layers(ids=p, labels=p, dims=d(4, 4, 4), pitch=16, axis=2, of=255):
        return lib.hu_ground_layers(ids, labels, dims, pitch, axis, of, 1, None)

    def seed(labels=p, word=p, dims=d(4, 4, 4), pitch=16, axis=2, up=1):
        return lib.hu_ground_seed(labels, word, dims, pitch, axis, up, None)

    def mark(ids=p, labels=p, floating=p, start=p, join=p, counts=p, dims=d(4, 4, 4), pitch=16, axis=2, of=255):
        return lib.hu_ground_mark(ids, labels, floating, start, join, counts, dims, pitch, axis, 1, of, None)

    refused = [layers(ids=None), layers(labels=None), layers(dims=None), seed(labels=None), seed(word=None), seed(dims=None), mark(ids=None),
               mark(labels=None), mark(floating=None), mark(start=None), mark(join=None), mark(counts=None), mark(dims=None)]
    refused += [f(axis=bad) for f in (layers, seed, mark) for bad in (3, -1)]
    refused += [f(pitch=bad) for f in (layers, seed, mark) for bad in (24, 0, 8)]
    refused += [f(dims=bad) for f in (layers, seed, mark) for bad in (d(4, 4, 17), d(0, 4, 4), d(4, 0, 4), d(4, 4, 0), d(65537, 4, 4))]
    refused += [f(of=bad) for f in (layers, mark) for bad in (64, 254, 256)]
    refused += [layers(ids=p + 8), layers(ids=p + 1), layers(labels=p + 2), seed(labels=p + 1), seed(word=p + 2), mark(ids=p + 4),
                mark(labels=p + 2), mark(counts=p + 4)]
    big = d(65536, 32768, 1)                                                          # 2^31 lines of pitch 16: 2^35 entries
    refused += [layers(dims=big), seed(dims=big), mark(dims=big), seed(dims=d(65536, 32768, 17), pitch=32), seed(dims=d(32768, 4097, 16)),
                seed(dims=d(32768, 4096, 16), up=0)]
    assert refused == [-3] * len(refused)
    assert seed(dims=big) == -3 and b"2^31" in lib.hu_last_error()
    assert seed(dims=d(32768, 4096, 16), up=0) == -3 and b"exactly 2^31" in lib.hu_last_error()
    assert mark(axis=3) == -3 and b"axis" in lib.hu_last_error()
    assert mark(pitch=24) == -3 and b"16" in lib.hu_last_error()
    assert layers(ids=p + 8) == -3 and b"aligned" in lib.hu_last_error()
    assert mark(counts=p + 4) == -3 and b"aligned" in lib.hu_last_error()
    assert seed(word=p + 2) == -3 and b"aligned" in lib.hu_last_error()
    assert seed(word=None) == -3 and b"NULL" in lib.hu_last_error()
    assert layers(of=64) == -3 and b"HU_OVERHANG_SOLID" in lib.hu_last_error()


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states():
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, and the VGPR counts and
    the LDS written in DESIGN.md; no LDS in the kernels islands() adds; the moved helpers once, in id_volume.hpp."""
    from codecad_amd.hip_util import builder
    assert reach.UNIT in builder.SOURCES and reach.UNIT not in builder.FLAGGED_SOURCES
    everything = reach.sources()
    assert "instance_ground.hip" not in everything and not os.path.exists(os.path.join(builder.CSRC, "instance_ground.hip"))
    source = everything[reach.UNIT]
    assert '#include "id_volume.hpp"' in source and '#include "label_kernels.hpp"' in source
    for function in ("constexpr uint32_t kFlag = 0x80000000u", "uint32_t live(", "bool escapes(", "bool raise("):
        assert [name for name, other in everything.items() if function in other] == ["id_volume.hpp"], function
        assert everything["id_volume.hpp"].count(function) == 1, function
    for helper in ("escapes(", "raise<", "label_tile<", "label_merge_faces(", "label_merge_all(", "gather_counts(", "line_unit<"):
        assert helper in source, helper
    for wrapped in ("label_tile<", "label_merge_faces(", "label_merge_all("):       # one stage-1 kernel set for every predicate
        assert source.count(wrapped) == 1, wrapped
    assert "hipMemset" not in source and "__shared__" not in source
    assert "__shared__" not in everything["id_volume.hpp"] and "__shared__" in everything["label_kernels.hpp"]
    for prefix in ("k_ground_", "k_drain_"):
        assert [name for name, other in everything.items() if prefix in other] == [reach.UNIT], prefix
    documented = reach.documented_resources(KERNELS)
    found = reach.compiled_resources()
    if found is None:
        pytest.skip("no hipcc in this environment")
    assert set(KERNELS) == set(reach.GROUND) and set(found) == set(reach.DRAIN) | set(reach.GROUND)
    assert all(private == 0 for _, _, private in found.values()), found
    assert {k: v[:2] for k, v in found.items() if k in KERNELS} == documented
    assert not any(found[k][1] for k in KERNELS)
