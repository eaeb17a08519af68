"""The reference and the scenarios of test_gpu_overhangs.py, and the host side of overhangs(), checked without a device.

overhangs_scenes.reference_overhangs is written from the definitions: shifted sets for O, a search along every line for P and
L.  That a running maximum along the axis, and the +z rule on the transposed and flipped ids, give the same volumes on every
case is the first test.  Every scenario is then inspected: the edge it was built for is IN THE REFERENCE, as numbers."""
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

import overhangs_scenes as scenes
from overhangs_scenes import CASES, NAMES, BY_NAME, reference, scene, SOLID, NONE, EMPTY, NZ

ov = sys.modules["codecad_amd.overhangs"]              # (the package's attribute of that name is the function)
ac = sys.modules["codecad_amd.assembly_components"]
av = sys.modules["codecad_amd.assembly_voxels"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_over_first", "k_over_mark", "k_over_columns<true>", "k_over_columns<false>")


def sets_of(ref):
    return {"O": sum(ref.overhang_counts), "P": sum(ref.support_counts), "L": sum(ref.landing_counts), "G": ref.plate_landings}


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_a_line_by_hand():
    """One line along z, upwards: solid at z = 0, 1 (on the plate), 5 (hangs), 6 (rests on 5), 9 (hangs), lattice of 11."""
    ids = numpy.full((1, 1, 11), EMPTY, dtype=numpy.uint8)
    ids[0, 0, [0, 1, 5, 6, 9]] = 0
    ref = scenes.reference_overhangs(ids, 2, True, 1, SOLID, 1)
    assert ref.first_layer == 0
    assert (ref.overhang_ids.ravel() != EMPTY).tolist() == [z in (5, 9) for z in range(11)]
    assert (ref.support_ids.ravel() != EMPTY).tolist() == [z in (2, 3, 4, 7, 8) for z in range(11)]     # nothing above z = 9
    assert (ref.landing_ids.ravel() != EMPTY).tolist() == [z in (1, 6) for z in range(11)]
    assert (ref.overhang_counts, ref.support_counts, ref.landing_counts, ref.plate_landings) == ([2], [5], [2], 0)
    assert [c.count for c in ref.supports] == [3, 2] and [c.label for c in ref.supports] == [2, 7]
    down = scenes.reference_overhangs(ids, 2, False, 1, SOLID, 1)                    # downwards the plate is over z = 9: h0 = 1
    assert down.first_layer == 1
    assert (down.overhang_ids.ravel() != EMPTY).tolist() == [z in (1, 6) for z in range(11)]
    assert (down.support_ids.ravel() != EMPTY).tolist() == [z in (2, 3, 4, 7, 8) for z in range(11)]    # z = 10 is below h0
    assert (down.landing_ids.ravel() != EMPTY).tolist() == [z in (5, 9) for z in range(11)]
    assert down.plate_landings == 0
    alone = numpy.full((1, 1, 6), EMPTY, dtype=numpy.uint8)
    alone[0, 0, 2], alone[0, 0, 4] = 0, 1
    ref = scenes.reference_overhangs(alone, 2, True, 0, SOLID, 2)                    # h0 = 2: P stops there
    assert ref.first_layer == 2 and ref.support_ids.ravel().tolist() == [EMPTY, EMPTY, EMPTY, 1, EMPTY, EMPTY]
    assert ref.landing_ids.ravel().tolist() == [EMPTY, EMPTY, 0, EMPTY, EMPTY, EMPTY] and ref.plate_landings == 0
    ref = scenes.reference_overhangs(alone, 2, True, 0, 1, 2)                        # of=1: part 0 is air, h0 = 4, nothing hangs
    assert ref.first_layer == 4 and sets_of(ref) == {"O": 0, "P": 0, "L": 0, "G": 0}
    assert scenes.reference_overhangs(numpy.full((2, 3, 4), EMPTY, numpy.uint8), 1, False, 1, SOLID, 0).first_layer == 3


def test_the_offsets_of_n():
    assert [len(scenes.offsets(r)) for r in range(9)] == [1, 5, 9, 9, 13, 21, 21, 21, 25]
    assert ov.MAX_REACH_SQ == 8 and scenes.MAX_REACH ** 2 * 2 == 8


@pytest.mark.parametrize("name", NAMES)
def test_the_three_ways_agree_and_the_invariant_holds(name):
    c, ref = BY_NAME[name], reference(name)
    n = len(ref.overhang_counts)
    wanted = (ref.first_layer, ref.overhang_ids, ref.support_ids, ref.landing_ids)
    for other in (scenes.accumulated_overhangs(ref.ids, c.axis, c.up, c.reach_sq, c.of),
                  scenes.canonical_overhangs(ref.ids, c.axis, c.up, c.reach_sq, c.of, n)):
        assert other[0] == wanted[0] and all(numpy.array_equal(a, b) for a, b in zip(other[1:], wanted[1:]))
    held, over, lands = ref.support_ids != EMPTY, ref.overhang_ids != EMPTY, ref.landing_ids != EMPTY
    sets = sets_of(ref)
    assert sets["O"] == sets["L"] + sets["G"]                                       # every overhang heads one column with one foot
    assert not (held & ref.in_set).any()                                            # P and S are disjoint
    assert (over <= ref.in_set).all() and (lands <= ref.in_set).all()
    assert numpy.array_equal(ref.overhang_ids[over], ref.ids[over]) and numpy.array_equal(ref.landing_ids[lands], ref.ids[lands])
    h = scenes.layers(ref.ids.shape, c.axis, c.up)
    assert (h[held] >= ref.first_layer).all() and (h[over] > ref.first_layer).all()
    assert sum(r.count for r in ref.supports) == sets["P"] and ((ref.labels == NONE) == ~held).all()
    assert sorted({k for r in ref.supports for k in r.parts}) == sorted(set(ref.support_ids[held].tolist()))


@pytest.mark.parametrize("name", NAMES)
def test_no_scenario_is_vacuous(name):
    """Every case leaves the sets it names non-empty; a case that does not name O has no overhang, and so nothing else."""
    c, ref = BY_NAME[name], reference(name)
    sets = sets_of(ref)
    assert ref.in_set.any() and all(sets[k] > 0 for k in c.nonempty), sets
    assert "O" in c.nonempty or sets == {"O": 0, "P": 0, "L": 0, "G": 0}
    dims = ref.ids.shape
    assert 130 <= dims[2] <= 150 and dims[2] % 16 and max(dims[:2]) < 40 and av.volume_shape(dims, 2 ** 32)[2] == 144 > dims[2]


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(scenes.STAIRS))
def test_the_staircases_sit_on_their_thresholds(name):
    rx, ry = scenes.STAIRS[name]
    clean, hangs = scenes.STAIR_THRESHOLDS[name]
    assert clean == rx * rx + ry * ry and hangs == max(r for r in (0, 1, 2, 4, 5, 8) if r < clean)
    ids = scenes.part_ids(name)
    for reach_sq in range(9):
        for up in (True, False):
            h0, o = scenes.overhang_set(ids != EMPTY, 2, up, reach_sq)
            assert h0 == 0 and bool(o.any()) == (reach_sq < clean), (reach_sq, up)
    h0, o = scenes.overhang_set(ids != EMPTY, 2, True, hangs)
    z = numpy.argwhere(o)[:, 2]
    assert z.min() == scenes.STAIR_BASE + 1 and z.max() == scenes.STAIR_BASE + scenes.STAIR_LAYERS - 1 and z.min() < 64 <= z.max()


def test_the_cuboid_has_no_overhang_in_any_direction():
    ids = scenes.part_ids("cuboid")
    assert (ids == 0).all()
    for axis, up in scenes.DIRECTIONS:
        assert not scenes.overhang_set(ids != EMPTY, axis, up, 0)[1].any()


def test_the_tee_and_the_bridge_stand_on_the_plate():
    tee = reference("tee_z+_r1")
    assert tee.plate_landings == sum(tee.overhang_counts) == 16 * 8 - 4 * 4 - 4 * 4 and tee.landing_counts == [0]   # the stem's rim holds at reach 1
    assert sum(tee.support_counts) == tee.plate_landings * 130 and len(tee.supports) == 1
    bridge = reference("bridge_z+_r1")
    assert bridge.landing_counts == [3 * 4] and bridge.plate_landings == sum(bridge.overhang_counts) - 12
    column = bridge.support_ids[7, 3]                                                # over the block: lands at z = 19
    assert (column[20:132] == 0).all() and (column[:20] == EMPTY).all() and bridge.landing_ids[7, 3, 19] == 0
    assert not bridge.in_set[7, 3, 64:128].any()                                     # the middle word of that line holds no solid


def test_the_ball_lands_on_the_slab_and_ownership_decides_the_holder():
    ref = reference("ball_z+_r1")
    ids = ref.ids
    assert (ids == 0).sum() == 4 ** 3 and ((ids == 0) & (ref.overhang_ids == 0)).any()       # the cap owns overhangs of the ball's shape
    assert ref.support_counts[0] > 0 and ref.support_counts[1] > 0
    assert ref.support_counts[2] == 24 * 24 * 10 - 3 * 3 * 2                         # the slab itself hangs over the plate and the pad
    assert ref.landing_counts[:2] == [0, 3 * 3] and ref.landing_counts[2] > 0 and ref.plate_landings == 24 * 24 - 3 * 3
    lands = numpy.argwhere(ref.landing_ids == 2)
    assert (lands[:, 2] == 15).all()                                                 # on the slab's top layer
    x, y = 12, 12
    assert ref.support_ids[x, y, 16:114].tolist() == [0] * 98                       # under the cap: held for part 0
    alone = reference("ball_z+_r1_of1")
    assert alone.first_layer == 0 and alone.landing_counts == [0, 0, 0] and alone.plate_landings == sum(alone.overhang_counts) > 0
    assert (alone.support_ids[:, :, 10:16] == 1).any() and (alone.ids[:, :, 10:16] == 2).all()   # through the slab
    assert reference("ball_z+_r1_of0").first_layer == 114


def test_the_words_scene_holds_every_edge_of_a_word():
    up, down = reference("words_z+_r1"), reference("words_z-_r1")
    for ref in (up, down):
        for x, z in ((0, 63), (0, 127), (2, 64), (2, 128)):
            assert (ref.overhang_ids[x, 2:5, z] == 0).all()                          # overhangs at both ends of a word, both ways
    assert {63, 64, 127, 128} == set(scenes.WORD_EDGES)
    column = up.support_ids[4, 3]                                                    # from the top word across the middle one to the floor
    assert (column[2:130] == 0).all() and not up.in_set[4, 3, 2:130].any() and up.landing_ids[4, 3, 1] == 0
    line = up.support_ids[6, 3] != EMPTY                                             # closes and reopens twice inside word 0
    runs = numpy.flatnonzero(numpy.diff(numpy.concatenate([[0], line[:64].astype(int), [0]])))
    assert runs.tolist() == [2, 20, 21, 30, 41, 50, 51, 64]                          # [2, 20) [21, 30) -- closed 31..39 -- [41, 50) [51, ...
    assert up.overhang_ids[6, 3, 40] == EMPTY and reference("words_z+_r0").overhang_ids[6, 3, 40] == 0
    assert up.in_set[14, 0].all() and up.in_set[15, 7].all()                         # lines whose words are wholly solid
    assert up.in_set[8, 3, 60:70].all() and up.overhang_ids[8, 3, 60] == 0 and (up.overhang_ids[8, 3, 61:70] == EMPTY).all()
    assert up.support_ids[10, 3, 2] == 0 and up.landing_ids[10, 3, 1] == 0           # a column of one sample
    assert up.in_set[:, :, NZ - 1].all() and (up.overhang_ids[:9, :, 136] == 0).all()        # the roof touches the top and hangs
    assert (down.overhang_ids[:12, :, 1] == 0).all() and down.first_layer == 0


def test_raised_stops_at_its_first_layer():
    ref = reference("raised_z+_r1")
    assert ref.first_layer == scenes.RAISED_FIRST and not ref.in_set[:, :, :5].any() and ref.in_set[:, :, NZ - 1].any()
    assert (ref.support_ids[:, :, :5] == EMPTY).all() and (ref.support_ids[0, 0, 5:100] == 0).all()
    assert ref.plate_landings == sum(ref.overhang_counts) == 3 * 8                   # x = 3 is held from x = 4 at reach 1
    assert reference("raised_z-_r1").first_layer == 0


def test_the_lateral_taps_cross_a_word_edge_and_leave_the_lattice():
    for name, swap in (("lateral_x_x+_r1", False), ("lateral_y_y+_r1", True)):
        ref = reference(name)
        at = (lambda x, y, z: (y, x, z)) if swap else (lambda x, y, z: (x, y, z))
        assert ref.overhang_ids[at(6, 8, 0)] == 0 and ref.overhang_ids[at(6, 8, NZ - 1)] == 0     # taps at z = -1 and z = nz
        stair = [at(2 + k, 3, 61 + 2 * k) for k in range(1, 8)]                    # the leading sample of each layer
        assert all(ref.overhang_ids[p] == 0 for p in stair) and any(p[2] == 63 for p in stair) and any(p[2] == 65 for p in stair)
        assert ref.overhang_ids[at(4, 3, 64)] == EMPTY and ref.in_set[at(4, 3, 64)] and ref.in_set[at(3, 3, 63)]   # held across 63 | 64
    assert sum(reference("lateral_x_x+_r4").overhang_counts) == 2 * 3 * 3           # only the floating ledges' undersides
    assert reference("lateral_x_x+_r1").support_counts == reference("lateral_y_y+_r1").support_counts


def test_the_six_directions_differ():
    refs = [reference(c.name) for c in scenes.SIX_CASES]
    assert len({(tuple(r.overhang_counts), tuple(r.support_counts), tuple(r.landing_counts), r.plate_landings) for r in refs}) == 6
    assert all(sum(r.overhang_counts) for r in refs) and sum(bool(r.overhang_counts[0] and r.overhang_counts[1]) for r in refs) >= 3
    ids = scenes.part_ids("six")
    assert (ids[8:11, 2:5, 124:126] == 0).all() and (ids[8:11, 2:7, 126:] == 1).all()   # the arm owns what both contain
    alone = reference("six_z+_r1_of1")
    assert alone.first_layer == 60 and (alone.support_ids[:, :, :60] == EMPTY).all()


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals():
    ball = shapes.sphere(r=1).make_part("ball")
    one = cc.assembly("one", [ball])
    for bad in ("void", None, ac.EMPTY_SPACE, 1, -1, 64, True, 0.0):
        with pytest.raises(ValueError):
            cc.overhangs(one, 0.5, of=bad)
    for bad in (3, -1, None, "z", True, 1.0):
        with pytest.raises(ValueError, match="axis"):
            cc.overhangs(one, 0.5, axis=bad)
    for bad in (9, -1, None, 1.5, True, "1"):
        with pytest.raises(ValueError, match="reach_sq"):
            cc.overhangs(one, 0.5, reach_sq=bad)
    with pytest.raises(ValueError):
        cc.overhangs(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.overhangs(one, -1)
    rod = cc.assembly("long", [shapes.box(40000 * 0.01, 300 * 0.01, 300 * 0.01).make_part("rod")])
    with pytest.raises(ValueError, match="2\\^31"):
        cc.overhangs(rod, 0.01, max_bytes=2 ** 40)
    assert {"overhangs", "OverhangReport"} <= set(cc.__all__) and ov.SAMPLE_BYTES == 5
    assert "overhangs(" in cc.__doc__


def test_no_visible_instance_gives_the_empty_report():
    ghost = shapes.box(1).make_part("ghost").hidden()
    report = cc.overhangs(cc.assembly("nothing", [ghost]), 0.1, axis=1, up=False, reach_sq=4, max_bytes=5 * 16)
    assert report.supports == [] and report.component_capacity_runs == 0 and report.traversals == 0
    assert report.overhang_counts == [] == report.support_counts == report.landing_counts == report.counts
    assert (report.axis, report.up, report.reach_sq, report.of, report.plate_landings) == (1, False, 4, SOLID, 0)
    assert report.first_layer == int(report.dims[1]) == 1
    for volume in (report.overhang_ids, report.support_ids, report.landing_ids):
        assert volume.shape == (1, 1, 1) and volume.dtype == numpy.uint8 and volume[0, 0, 0] == EMPTY
    assert report.labels[0, 0, 0] == NONE and report.labels.dtype == numpy.uint32
    assert report.self_supporting and report.support_volume() == 0.0 and report.overhang_area() == 0.0
    with pytest.raises(ValueError):
        cc.overhangs(cc.assembly("nothing", [ghost]), 0.1, max_bytes=5 * 16 - 1)
    with pytest.raises(ValueError):
        cc.overhangs(cc.assembly("nothing", [ghost]), 0.1, of=0)


def fake_device(monkeypatch, n_regions=2):
    """overhangs() over a library that records its calls and a support table with `n_regions` roots."""
    calls = []

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x10000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            calls.append(("read", self.device_ptr))
            out = numpy.zeros(self.shape, self.dtype)
            if self.dtype == ac._ROW:
                out[:1].view(numpy.uint32)[0] = n_regions
                for k in range(1, len(out)):
                    out[k] = (k, (k, 2 * k, 3 * k), 1, (0xffffffff - 1,) * 3, (2, 3, 4), 100000 - k, 1)
            elif self.dtype == numpy.uint64:
                out[0, :2], out[1, :2], out[2, :2] = (3, 4), (30, 40), (1, 2)
                out[3, 0], out[3, 1] = 4, 100                                         # the plate landings, the depth word
            elif self.dtype == numpy.uint32:
                out[...] = 7
            elif self.dtype == numpy.uint8:
                out[...] = self.device_ptr >> 16
            return out

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
        return 77, numpy.array([5, 6, 999], dtype=numpy.uint64), 2

    manager = types.SimpleNamespace(lib=Lib(), queue=types.SimpleNamespace(handle=0x99))
    for module in (av, ac, ov):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


@pytest.mark.parametrize("axis,up", [(2, True), (0, False)])
def test_the_driver_launches_three_kernels_and_labels_the_support_ids(monkeypatch, axis, up):
    asm, resolution = scene("six")[:2]
    calls = fake_device(monkeypatch)
    report = cc.overhangs(asm, resolution, axis=axis, up=up, reach_sq=5, of=1, initial_components=9, initial_capacity=7,
                          max_bytes=5 * 14 * 18 * 144)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names == ["buffer", "hu_memset", "traverse", "read",                       # the ids, as assembly_voxels() leaves them
                     "buffer", "hu_memset", "buffer", "buffer", "buffer",             # the accumulators, then the three id volumes
                     "hu_overhang_first_layer", "hu_overhang_mark", "hu_overhang_columns",
                     "read", "read", "read", "read", "release", "release", "release", "release",
                     "buffer", "hu_components_local", "hu_components_merge", "hu_components_flatten",
                     "buffer", "hu_memset", "hu_components_stats", "read", "release",
                     "release", "hu_components_finish", "read", "release"]
    assert calls[2][1:] == (7, 1)                                                     # retire=True, the cell lists' capacity
    ids, acc, over, support, landing, labels = (0x10000 * k for k in (1, 2, 3, 4, 5, 6))
    u8, shape = numpy.dtype(numpy.uint8), (14, 18, 144)
    assert [c[1:] for c in calls if c[0] == "buffer"][:6] == [(u8, shape), (numpy.dtype(numpy.uint64), (4, 64)), (u8, shape), (u8, shape),
                                                              (u8, shape), (numpy.dtype(numpy.uint32), shape)]
    assert calls[5][1] == (acc, 0, 2048, 0x99)
    word = acc + 8 * 193
    first, mark, columns = (calls[k][1] for k in (9, 10, 11))
    #      ids, word | pitch, axis, up, of, stream
    assert first[:2] + first[3:] == (ids, word, 144, axis, int(up), 1, 0x99)
    #      ids, overhang, word, counts | pitch, axis, up, reach_sq, of, stream
    assert mark[:4] + mark[5:] == (ids, over, word, acc, 144, axis, int(up), 5, 1, 0x99)
    #      ids, overhang, support, landing, word, counts | pitch, axis, up, of, stream
    assert columns[:6] + columns[7:] == (ids, over, support, landing, word, acc + 512, 144, axis, int(up), 1, 0x99)
    assert all(list(c) == [14, 18, 138] for c in (first[2], mark[4], columns[6]))
    assert [c[1] for c in calls[12:20]] == [over, support, landing, acc, over, landing, ids, acc]   # 5 bytes a sample from here on
    local = calls[21][1]
    assert (local[0], local[1], list(local[2]), local[3:]) == (support, labels, [14, 18, 138], (144, 1, 1, 0x99))   # solid = 1, local
    stats = calls[26][1]
    assert stats[:2] == (support, labels) and stats[3:6] == (144, 1, 1) and stats[8] == 9
    assert calls[29] == ("release", support)
    assert (report.of, report.axis, report.up, report.reach_sq) == (1, axis, up, 5)
    assert report.first_layer == (138, 14)[axis == 0] - 100 and report.plate_landings == 4
    assert report.counts == [5, 6] and report.overhang_counts == [3, 4] and report.support_counts == [30, 40] and report.landing_counts == [1, 2]
    for volume, value in ((report.overhang_ids, 3), (report.support_ids, 4), (report.landing_ids, 5), (report.part_ids, 1)):
        assert volume.shape == (14, 18, 138) and (volume == value).all() and volume.dtype == numpy.uint8
    assert report.overhang_ids.flags.c_contiguous and (report.labels == 7).all() and report.labels.shape == (14, 18, 138)
    assert [r.label for r in report.supports] == [99998, 99999] and report.component_capacity_runs == 1
    assert report.traversals == 2 and report.samples_evaluated == 77 and report.mask(7).all() and not report.mask(report.supports[0]).any()
    step = float(report.step)
    assert report.support_volume() == 70 * step ** 3 and report.overhang_area() == 7 * step ** 2 and not report.self_supporting
    assert report.supports[0].volume == 2 * step ** 3 and report.supports[0].parts == (0,)


def test_max_bytes_counts_five_bytes_a_sample_before_any_launch(monkeypatch):
    asm, resolution = scene("six")[:2]
    calls = fake_device(monkeypatch)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.overhangs(asm, resolution, max_bytes=5 * 14 * 18 * 144 - 1)
    with pytest.raises(ValueError):
        cc.overhangs(asm, resolution, of=2)
    with pytest.raises(ValueError):
        cc.overhangs(asm, resolution, reach_sq=9)
    with pytest.raises(ValueError):
        cc.overhangs(asm, resolution, axis=3)
    assert calls == []
    cc.overhangs(asm, resolution, max_bytes=5 * 14 * 18 * 144)
    monkeypatch.undo()
    launched = [c for c in calls if c[0].startswith("hu_overhang")]
    assert [c[0] for c in launched] == ["hu_overhang_first_layer", "hu_overhang_mark", "hu_overhang_columns"]
    assert launched[0][1][3:7] == (144, 2, 1, 255) and launched[1][1][5:10] == (144, 2, 1, 1, 255)      # +z, reach_sq = 1, SOLID


# ---- the C ABI, the entry points' refusals and the kernels' resources -------------------------------------------------

ENTRY_POINTS = ("hu_overhang_first_layer", "hu_overhang_mark", "hu_overhang_columns")


def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(_lib.PROTOTYPES[name]) == len(proto.split(","))
        assert ("int %s(" % name) in integration
    constant = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))   # noqa: E731
    assert constant("HU_OVERHANG_SOLID") == av._SOLID_CODE == EMPTY
    assert constant("HU_OVERHANG_MAX_REACH_SQ") == ov.MAX_REACH_SQ
    assert ov._ACC == (4, 64) and (ov._PLATE, ov._WORD) == (192, 193)                 # the columns' counts start at row 1: 64 + 64 + 1


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def first(ids=p, word=p, dims=d(4, 4, 4), pitch=16, axis=2, of=255):
        return lib.hu_overhang_first_layer(ids, word, dims, pitch, axis, 1, of, None)

    def mark(ids=p, over=p, word=p, counts=p, dims=d(4, 4, 4), pitch=16, axis=2, reach_sq=1, of=255):
        return lib.hu_overhang_mark(ids, over, word, counts, dims, pitch, axis, 1, reach_sq, of, None)

    def columns(ids=p, over=p, support=p, landing=p, word=p, counts=p, dims=d(4, 4, 4), pitch=16, axis=0, of=255):
        return lib.hu_overhang_columns(ids, over, support, landing, word, counts, dims, pitch, axis, 0, of, None)

    refused = [first(ids=None), first(word=None), first(dims=None), first(pitch=24), first(pitch=0), first(dims=d(4, 4, 17)),
               first(dims=d(0, 4, 4)), first(dims=d(4, 65537, 4)), first(axis=3), first(axis=-1), first(of=64), first(of=254),
               first(word=p + 2),
               mark(ids=None), mark(over=None), mark(word=None), mark(counts=None), mark(dims=None), mark(pitch=8), mark(pitch=20),
               mark(dims=d(4, 4, 0)), mark(axis=3), mark(reach_sq=9), mark(of=100), mark(counts=p + 4),
               columns(ids=None), columns(over=None), columns(support=None), columns(landing=None), columns(word=None),
               columns(counts=None), columns(dims=None), columns(pitch=3), columns(dims=d(65537, 4, 4)), columns(axis=3),
               columns(of=64), columns(counts=p + 4), columns(word=p + 1)]
    assert refused == [-3] * len(refused)
    assert mark(reach_sq=9) == -3 and b"reach_sq" in lib.hu_last_error()
    assert first(axis=3) == -3 and b"axis" in lib.hu_last_error()
    assert columns(pitch=24) == -3 and b"16" in lib.hu_last_error()


def documented_resources():
    """{kernel: (VGPRs, LDS bytes)} as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    found = {}
    for name in KERNELS:
        m = re.search(r"`%s` (\d+) VGPRs and (\d+) B of LDS" % re.escape(name), text)
        assert m, "DESIGN.md section 9 states the VGPRs and the LDS of " + name
        found[name] = (int(m.group(1)), int(m.group(2)))
    return found


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states(tmp_path):
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, no LDS, and the VGPR
    counts written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_overhang.hip" in builder.SOURCES and "instance_overhang.hip" not in builder.FLAGGED_SOURCES
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_overhang.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_overhang.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"\d+(k_over_first|k_over_mark|k_over_columns)(?:ILb([01])EEEv|E)NS_8OverArgsE", name)
        assert m, name
        kernel = m.group(1) + ("" if m.group(2) is None else "<%s>" % ("false", "true")[int(m.group(2))])
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[kernel] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)))
    assert found == documented_resources()
    assert all(lds == 0 for _, lds in found.values())
