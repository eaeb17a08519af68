"""The reference and the scenarios of test_gpu_thin_walls.py, and the host side of thin_walls(), checked without a device.

thin_walls_scenes.reference_thin is written from the definitions, offset by offset; that three capped 1D min-plus passes per
transform -- the way the device goes -- give the same depth, core and thin set on every scenario is the first test.  Every
scenario is then inspected: the edge it was built for is IN THE REFERENCE, as numbers."""
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

import thin_walls_scenes as scenes
from thin_walls_scenes import CASES, NAMES, BY_NAME, reference, scene, SOLID, NONE, EMPTY, MIXED, ALL_THIN, NONE_THIN

tw = sys.modules["codecad_amd.thin_walls"]             # (the package's attribute of that name is the function)
ac = sys.modules["codecad_amd.assembly_components"]
av = sys.modules["codecad_amd.assembly_voxels"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_thick_z<false, true>", "k_thick_z<false, false>", "k_thick_z<true, true>", "k_thick_z<true, false>",
           "k_thick_axis<0, true>", "k_thick_axis<0, false>", "k_thick_axis<1, true>", "k_thick_axis<1, false>",
           "k_thick_axis<2, true>", "k_thick_axis<2, false>")


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_a_line_by_hand():
    ids = numpy.full((1, 1, 9), 0, dtype=numpy.uint8)
    ids[0, 0, 7] = EMPTY                                                             # S = z in 0..6 and z = 8
    ref = scenes.reference_thin(ids, SOLID, 1, 1, 1)
    assert ref.depth_sq.ravel().tolist() == [1] * 7 + [0, 1] and not ref.core.any()   # x and y leave the lattice one step out
    wide = numpy.pad(ids, ((2, 2), (2, 2), (0, 0)), constant_values=0)                # 5 x 5 x 9: the middle line is two steps in
    ref = scenes.reference_thin(wide, SOLID, 1, 1, 1)
    assert ref.depth_sq[2, 2].tolist() == [1, 2, 2, 2, 2, 2, 1, 0, 1]
    assert ref.core[2, 2].tolist() == [False, True, True, True, True, True, False, False, False]
    assert (ref.thin_ids[2, 2] != EMPTY).tolist() == [False] * 7 + [False, True]      # z = 8 is two steps from the core
    assert ref.thin_counts == [int((ref.thin_ids != EMPTY).sum())] and ref.core_counts == [int(ref.core.sum())] == [57]


@pytest.mark.parametrize("name", NAMES)
def test_the_offsets_agree_with_three_capped_passes(name):
    c, ref = BY_NAME[name], reference(name)
    depth, core, thin = scenes.separable_thin(ref.ids, c.of, c.r2, c.c2)
    assert numpy.array_equal(depth, ref.depth_sq) and numpy.array_equal(core, ref.core)
    assert numpy.array_equal(thin, ref.thin_ids != EMPTY)
    assert numpy.array_equal(ref.thin_ids[thin], ref.ids[thin]) and (ref.depth_sq[~ref.in_set] == 0).all()
    assert ref.depth_sq.max() <= c.r2 + 1 and max(ref.ids.shape) <= (70 if c.scene == "tower" else 64)
    assert sum(r.count for r in ref.regions) == int(thin.sum()) == sum(ref.thin_counts)


@pytest.mark.parametrize("name", NAMES)
def test_no_scenario_is_vacuous(name):
    """Every scenario but the named all-thin and none-thin ones has T and O both non-empty; those have what their name says."""
    c, ref = BY_NAME[name], reference(name)
    thin, cover = int((ref.thin_ids != EMPTY).sum()), int(ref.cover.sum())
    assert ref.in_set.any()
    assert {MIXED: thin > 0 and cover > 0, ALL_THIN: thin > 0 and cover == 0, NONE_THIN: thin == 0 and cover > 0}[c.expect]


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def test_the_slabs_follow_the_rule_on_every_axis():
    for axis in range(3):
        for k, w in scenes.SLABS:
            c = BY_NAME["slab_%s_k%d_w%d" % ("xyz"[axis], k, w)]
            dims = [int(d) for d in scene(c.scene)[5]]
            assert dims[axis] == w and sorted(dims)[1:] == [scenes.PLATE] * 2 and (c.r2, c.c2) == (k * k, 3 * k * k)
            assert c.expect == (ALL_THIN if (w + 1) // 2 <= k else NONE_THIN)
    assert sum(c.expect == ALL_THIN for c in CASES if c.scene.startswith("slab")) == 9


def test_the_bars_tell_radii_and_diagonals_apart():
    one, two = reference("bars_r1_c1"), reference("bars_r2_c2")
    assert not numpy.array_equal(one.thin_ids, two.thin_ids)
    assert one.thin_counts == [56, 48] and two.thin_counts == [8, 48]               # |o|^2 = 2 reaches the edges of the 3 x 3 bar
    assert reference("bars_r1_c3").thin_counts == [0, 48]                            # ... and 3 its corners at the ends
    assert not numpy.array_equal(one.depth_sq, two.depth_sq)
    assert reference("bars_r3_c3").core_counts == [10, 0] and reference("bars_r4_c4").core_counts == [0, 0]
    assert len(two.regions) == 9 and all(r.count == 1 for r in two.regions[:8])      # the eight end corners, and the 2 x 2 bar


def test_the_cuboids_sit_on_the_threshold():
    assert reference("cuboid_5").core_counts == [1] and reference("cuboid_5").thin_counts == [0]
    assert reference("cuboid_4").core_counts == [0] and reference("cuboid_4").thin_counts == [100]


def test_the_rib_and_the_floor_are_two_regions_and_the_cover_bleeds_into_their_roots():
    ref = reference("rib")
    rib, floor = ref.regions
    assert rib.parts == floor.parts == (0,) and not (ref.labels == NONE).all()
    assert rib.box[0][0] == 5 and rib.box[1][0] == 6 and rib.box[1][2] == 15         # 2 wide, up to the top
    assert rib.box[0][2] == 11 > 10                                                   # its root at z = 10 is covered from the body
    assert floor.box[1] == (23, 11, 1) and floor.box[0][0] == 12                      # the floor beside the body
    assert ref.thin_ids[12, 6, 1] == EMPTY and ref.thin_ids[12, 6, 0] == 0            # (9 + 1 <= 12 < 9 + 4 from the core)
    assert rib.touches_border and floor.touches_border
    assert reference("rib_r0").core_counts == [int(ref.in_set.sum())]                 # R2 = 0: E = S


def test_only_the_tip_of_the_wedge_is_thin():
    ref = reference("wedge")
    (tip,) = ref.regions
    assert tip.box[1][2] < 8 and tip.box[0][2] == 0                                   # the steps of 2 and of 4 samples, not all of them
    assert (ref.thin_ids[:, :, 8:] == EMPTY).all() and (ref.thin_ids[3:5, :, 0] == 0).all()


def test_ragged_reaches_every_border_and_the_largest_radii():
    dims = [int(d) for d in scene("ragged")[5]]
    assert dims == [13, 9, 11] and av.volume_shape(dims, 2 ** 32)[2] == 16 > dims[2]
    ref = reference("ragged")
    assert ref.in_set[0].any() and ref.in_set[-1].any() and ref.in_set[:, 0].any() and ref.in_set[:, -1].any()
    assert ref.in_set[:, :, 0].all() and ref.in_set[:, :, -1].any()
    (wall,) = ref.regions                                                             # the wall of 2, not the wall of 3
    assert wall.box[0][0] == 0 and wall.box[1][0] == 1 and wall.box[1][2] == 10 and wall.touches_border
    far = BY_NAME["ragged_far"]
    assert scenes.isqrt(far.r2) > max(dims) and far.c2 == tw.MAX_COVER_SQ == 65534 and scenes.isqrt(far.c2) == 255
    assert tw.axis_tile(255, True) == (64, 0) and tw.axis_tile(scenes.isqrt(far.r2), True) == (216, 1)


def test_the_tower_is_thin_exactly_across_the_edge_of_two_segments():
    dims = [int(d) for d in scene("tower")[5]]
    assert dims == [12, 12, 70] and av.volume_shape(dims, 2 ** 32)[2] == 80 and (dims[2] + 63) // 64 == 2
    c, ref = BY_NAME["tower"], reference("tower")
    assert (c.r2, c.c2) == (4, 12)
    plate = ref.in_set[:, :, 63:65]
    assert plate.all() and not ref.in_set[:, :, 56:63].any() and ref.in_set[:, :, :56].all()
    thin = ref.thin_ids != EMPTY
    assert set(numpy.argwhere(thin)[:, 2].tolist()) == {63, 64}                      # nothing else is thin, and both layers are
    assert thin[:, :, 63].sum() > 72 and thin[:, :, 64].sum() > 72 and not thin[:, :, 63].all() and not thin[:, :, 64].all()
    assert ref.core[:, :, :56].any() and ref.core[:, :, 65:].any() and not ref.core[:, :, 63:65].all()
    assert int(ref.depth_sq[0, 0, 63]) == 1 == int(ref.depth_sq[0, 0, 64])          # each layer has the other and then background
    # the thin plate's distances cross z = 63 | 64: the z pass of either segment takes a tap from the other
    above = scenes.min_plus_1d(numpy.where(ref.in_set, c.r2 + 1, 0)[:, :, 64:], 2, 2, c.r2 + 1, 0)
    whole = scenes.min_plus_1d(numpy.where(ref.in_set, c.r2 + 1, 0), 2, 2, c.r2 + 1, 0)
    assert not numpy.array_equal(above[:, :, :2], whole[:, :, 64:66])                # under the pillar z = 64 is two steps from z = 62
    (region,) = ref.regions
    assert region.box[0][2] == 63 and region.box[1][2] == 64


def test_ragged_crosses_the_switch_from_lds_tiles_to_global_taps():
    low, high = BY_NAME["ragged_k96"], BY_NAME["ragged_k97"]
    assert (low.scene, high.scene) == ("ragged", "ragged") and (low.r2, high.r2) == (2, 2)
    assert (low.c2, high.c2) == (96 * 96, 97 * 97) and (scenes.isqrt(low.c2), scenes.isqrt(high.c2)) == (96, 97)
    assert scenes.isqrt(low.c2 - 1) == 95 and tw._MAX_LDS_K == 96
    assert tw.axis_tile(96, True) == (64, 1) and tw.axis_tile(97, True) == (64, 0) and tw.axis_tile(96, False) == (64, 0)
    for c in (low, high):
        ref = reference(c.name)
        assert ref.core.any() and ref.cover.sum() == ref.in_set.sum() and ref.thin_counts == [0] and ref.regions == []
        assert numpy.array_equal(ref.depth_sq, reference("ragged").depth_sq)         # the first transform is that of `ragged`


def test_ownership_decides_between_two_parts():
    assert reference("glued_solid").thin_counts == [0, 0] and reference("glued_plate").thin_counts == [288, 0]
    assert reference("glued_block").thin_counts == [0, 0] and reference("glued_block").core_counts[0] == 0
    assert reference("pressed_solid").thin_counts == [0, 0] and reference("pressed_pin").thin_counts == [48, 0]
    assert int((scenes.part_ids("pin_in_block") == 0).sum()) == 2 * 2 * 12            # the pin owns what both contain
    (region,) = reference("pressed_pin").regions
    assert region.parts == (0,)


def test_the_shell_is_thin_everywhere():
    ref = reference("shell")
    assert ref.core_counts == [0] and ref.thin_counts == [int(ref.in_set.sum())] and len(ref.regions) == 1
    assert not ref.regions[0].touches_border or ref.regions[0].count > 18000


# ---- the two facts of the docstring ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(1, 7))
def test_the_slab_rule_and_the_cuboid_fact(k):
    r2, side = k * k, 2 * k + 1
    for sides in ((side, side, side), (side, side + 3, side + 1)):
        ref = scenes.reference_thin(numpy.zeros(sides, numpy.uint8), SOLID, r2, 3 * r2, 1)
        assert ref.core.any() and not (ref.thin_ids != EMPTY).any()
        corner_to_core = min(int(((numpy.array(p)) ** 2).sum()) for p in numpy.argwhere(ref.core))
        assert corner_to_core == 3 * r2                                               # the corner sample is exactly at the cover radius
    for w in range(1, 2 * k + 3):
        for axis in range(3):
            sides = [side] * 3
            sides[axis] = w
            ref = scenes.reference_thin(numpy.zeros(sides, numpy.uint8), SOLID, r2, 3 * r2, 1)
            thin = ref.thin_ids != EMPTY
            assert thin.all() if ((w + 1) // 2) ** 2 <= r2 else not thin.any(), (k, w, axis)


def test_the_default_radii():
    assert tw.radii(numpy.float32(0.0625), 0.25) == (4, 12) and tw.radii(numpy.float32(0.0625), 0.3) == (5, 15)
    assert tw.radii(numpy.float32(0.0625), 0.0) == (0, 0) and tw.radii(numpy.float32(0.1), 0.2) == (0, 0)   # (float32(0.1) > 0.1)
    assert tw.radii(numpy.float32(1), None, 7) == (7, 21) and tw.radii(numpy.float32(1), None, 7, 9) == (7, 9)
    assert tw.radii(numpy.float32(1), 5, 400, 65534) == (400, 65534)
    for bad in ((-1.0,), (float("nan"),), (float("inf"),), (None,), ("1",), (None, 5, 4), (None, 21845, None), (None, 1, 65535),
                (None, -1), (None, 1.5), (296,)):
        with pytest.raises(ValueError):
            tw.radii(numpy.float32(1), *bad)
    with pytest.raises(ValueError, match="coarser resolution"):
        tw.radii(numpy.float32(1), None, 1, 65535)
    with pytest.raises(ValueError, match="coarser resolution"):
        tw.radii(numpy.float32(0.001), 1.0)


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals():
    ball = shapes.sphere(r=1).make_part("ball")
    one = cc.assembly("one", [ball])
    for bad in ("void", None, ac.EMPTY_SPACE, 1, -1, 64, True, 0.0):
        with pytest.raises(ValueError):
            cc.thin_walls(one, 0.5, 0.5, of=bad)
    for bad in (-0.1, float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            cc.thin_walls(one, 0.5, bad)
    with pytest.raises(ValueError):
        cc.thin_walls(one, 0.5, radius_sq=5, cover_sq=4)
    with pytest.raises(ValueError, match="coarser resolution"):
        cc.thin_walls(one, 0.5, radius_sq=5, cover_sq=65535)
    with pytest.raises(ValueError):
        cc.thin_walls(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1, 0.1)
    with pytest.raises(ValueError):
        cc.thin_walls(one, -1, 0.1)
    rod = cc.assembly("long", [shapes.box(40000 * 0.01, 300 * 0.01, 300 * 0.01).make_part("rod")])
    with pytest.raises(ValueError, match="2\\^31"):
        cc.thin_walls(rod, 0.01, 0.05, max_bytes=2 ** 40)
    assert {"thin_walls", "ThinWallReport"} <= set(cc.__all__) and tw.SAMPLE_BYTES == 7


def test_no_visible_instance_gives_a_report_with_nothing_thin():
    ghost = shapes.box(1).make_part("ghost").hidden()
    report = cc.thin_walls(cc.assembly("nothing", [ghost]), 0.1, 0.3, max_bytes=7 * 16)
    assert report.regions == [] and report.component_capacity_runs == 0 and report.traversals == 0
    assert report.thin_counts == [] == report.core_counts == report.counts and (report.radius_sq, report.cover_sq) == (2, 6)
    assert report.depth_sq.shape == (1, 1, 1) and report.depth_sq.dtype == numpy.uint16 and report.depth_sq[0, 0, 0] == 0
    assert report.thin_ids.dtype == numpy.uint8 and report.thin_ids[0, 0, 0] == EMPTY and report.labels[0, 0, 0] == NONE
    with pytest.raises(ValueError):
        cc.thin_walls(cc.assembly("nothing", [ghost]), 0.1, 0.3, max_bytes=7 * 16 - 1)
    with pytest.raises(ValueError):
        cc.thin_walls(cc.assembly("nothing", [ghost]), 0.1, 0.3, of=0)


def fake_device(monkeypatch, n_regions=2):
    """thin_walls() over a library that records its calls and a region table with `n_regions` roots."""
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
                out[0, :2], out[1, :2] = (11, 12), (3, 4)
            elif self.dtype == numpy.uint32:
                out[...] = 7
            elif self.dtype == numpy.uint16:
                out[...] = 5
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
    for module in (av, ac, tw):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


@pytest.mark.parametrize("lds", [True, False])
def test_the_driver_launches_six_passes_and_labels_the_thin_ids(monkeypatch, lds):
    asm, resolution = scene("plate_on_block")[:2]
    calls = fake_device(monkeypatch)
    report = cc.thin_walls(asm, resolution, of=1, radius_sq=5, cover_sq=14, lds=lds, initial_components=9, initial_capacity=7,
                           max_bytes=7 * 12 * 12 * 16)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names == ["buffer", "hu_memset", "traverse", "read",                       # the ids, as assembly_voxels() leaves them
                     "buffer", "buffer", "buffer", "hu_memset",                       # depth, a second volume, the counts
                     "hu_thickness_pass_z", "hu_thickness_pass_axis", "hu_thickness_pass_axis",
                     "buffer", "hu_thickness_pass_z", "hu_thickness_pass_axis", "release", "buffer", "hu_thickness_pass_axis",
                     "read", "read", "read", "release", "release", "release", "release",
                     "buffer", "hu_components_local", "hu_components_merge", "hu_components_flatten",
                     "buffer", "hu_memset", "hu_components_stats", "read", "release",
                     "release", "hu_components_finish", "read", "release"]
    assert calls[2][1:] == (7, 1)                                                     # retire=True, the cell lists' capacity
    ids, depth, other, acc, third, thin, labels = (0x10000 * k for k in (1, 2, 3, 4, 5, 6, 7))
    u16, shape = numpy.dtype(numpy.uint16), (12, 12, 16)
    assert [c[1:] for c in calls if c[0] == "buffer"][:7] == [(numpy.dtype(numpy.uint8), shape), (u16, shape), (u16, shape),
                                                              (numpy.dtype(numpy.uint64), (2, 64)), (u16, shape),
                                                              (numpy.dtype(numpy.uint8), shape), (numpy.dtype(numpy.uint32), shape)]
    assert calls[7][1] == (acc, 0, 1024, 0x99)
    dims = lambda a: list(a)                                                          # noqa: E731
    flag = int(lds)
    z1, y1, x1, z2, y2, x2 = (calls[k][1] for k in (8, 9, 10, 12, 13, 16))
    assert (z1[:3], dims(z1[3]), z1[4:]) == ((ids, None, depth), [12, 12, 12], (16, 1, 5, 2, 6, flag, 0x99))
    assert (z2[:3], dims(z2[3]), z2[4:]) == ((None, depth, other), [12, 12, 12], (16, 1, 5, 3, 15, flag, 0x99))
    tile1, tile2 = ((252, 1), (250, 1)) if lds else ((64, 0), (64, 0))
    #            in, out, ids, thin, counts | pitch, axis, of, K, cap, outside, finish, tile, lds, stream
    assert y1[:5] + y1[6:] == (depth, other, None, None, None, 16, 1, 1, 2, 6, 0, 0) + tile1 + (0x99,)
    assert x1[:5] + x1[6:] == (other, depth, ids, None, acc, 16, 0, 1, 2, 6, 0, 1) + tile1 + (0x99,)
    assert y2[:5] + y2[6:] == (other, third, None, None, None, 16, 1, 1, 3, 15, 15, 0) + tile2 + (0x99,)
    assert x2[:5] + x2[6:] == (third, None, ids, thin, acc + 512, 16, 0, 1, 3, 15, 15, 2) + tile2 + (0x99,)
    assert all(dims(c[5]) == [12, 12, 12] for c in (y1, x1, y2, x2))
    assert calls[14] == ("release", other)                                            # before the thin ids are allocated: 7 bytes a sample
    assert [c[1] for c in calls[17:24]] == [depth, thin, acc, depth, third, ids, acc]
    local = calls[25][1]
    assert (local[0], local[1], dims(local[2]), local[3:]) == (thin, labels, [12, 12, 12], (16, 1, 1, 0x99))   # solid = 1, local
    stats = calls[30][1]
    assert stats[:2] == (thin, labels) and stats[3:6] == (16, 1, 1) and stats[8] == 9
    assert calls[33] == ("release", thin)
    assert report.of == 1 and (report.radius_sq, report.cover_sq) == (5, 14)
    assert report.counts == [5, 6] and report.core_counts == [11, 12] and report.thin_counts == [3, 4]
    assert report.depth_sq.shape == (12, 12, 12) and (report.depth_sq == 5).all() and report.depth_sq.flags.c_contiguous
    assert report.thin_ids.shape == (12, 12, 12) and report.part_ids.shape == (12, 12, 12) and (report.labels == 7).all()
    assert [r.label for r in report.regions] == [99998, 99999] and report.component_capacity_runs == 1
    assert report.traversals == 2 and report.samples_evaluated == 77 and report.mask(7).all() and not report.mask(report.regions[0]).any()
    step = float(report.step)
    assert report.regions[0].volume == 2 * step ** 3 and report.regions[0].parts == (0,)


def test_wide_radii_take_their_taps_from_global_memory(monkeypatch):
    asm, resolution = scene("ragged")[:2]
    calls = fake_device(monkeypatch)
    cc.thin_walls(asm, resolution, radius_sq=400, cover_sq=65534)
    monkeypatch.undo()
    z = [c[1] for c in calls if c[0] == "hu_thickness_pass_z"]
    axis = [c[1] for c in calls if c[0] == "hu_thickness_pass_axis"]
    assert [c[7:10] for c in z] == [(20, 401, 1), (255, 65535, 1)] and all(c[5] == 255 for c in z)        # of: the SOLID code
    assert [c[9:15] for c in axis] == [(20, 401, 0, 0, 216, 1), (20, 401, 0, 1, 216, 1),
                                       (255, 65535, 65535, 0, 64, 0), (255, 65535, 65535, 2, 64, 0)]


def test_max_bytes_counts_seven_bytes_a_sample_before_any_launch(monkeypatch):
    asm, resolution = scene("ragged")[:2]
    calls = fake_device(monkeypatch)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.thin_walls(asm, resolution, 0.25, max_bytes=7 * 13 * 9 * 16 - 1)
    with pytest.raises(ValueError):
        cc.thin_walls(asm, resolution, 0.25, of=1)
    with pytest.raises(ValueError):
        cc.thin_walls(asm, resolution, radius_sq=3, cover_sq=2)
    assert calls == []
    cc.thin_walls(asm, resolution, 0.25, max_bytes=7 * 13 * 9 * 16)
    monkeypatch.undo()
    assert [c[0] for c in calls].count("hu_thickness_pass_axis") == 4


# ---- the C ABI, the entry points' refusals and the kernels' resources -------------------------------------------------

ENTRY_POINTS = ("hu_thickness_pass_z", "hu_thickness_pass_axis")


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
    assert constant("HU_THICKNESS_SOLID") == av._SOLID_CODE == EMPTY
    assert constant("HU_THICKNESS_LDS_ROWS") == tw.LDS_ROWS and constant("HU_THICKNESS_MAX_K") == 255 == scenes.isqrt(tw.MAX_COVER_SQ)
    assert all(sum(tw.axis_tile(k, True)) - 1 + 2 * k <= tw.LDS_ROWS for k in range(0, tw._MAX_LDS_K + 1))
    assert tw.axis_tile(tw._MAX_LDS_K, True) == (64, 1) and tw.axis_tile(tw._MAX_LDS_K + 1, True) == (64, 0)


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def z(ids=p, depth=None, out=p, dims=d(4, 4, 4), pitch=16, of=255, r2=1, K=1, cap=2):
        return lib.hu_thickness_pass_z(ids, depth, out, dims, pitch, of, r2, K, cap, 1, None)

    def axis(source=p, out=p + 0x1000, ids=None, thin=None, counts=None, dims=d(4, 4, 4), pitch=16, which=0, of=255, K=1, cap=2,
             outside=0, finish=0, tile=64, lds=1):
        return lib.hu_thickness_pass_axis(source, out, ids, thin, counts, dims, pitch, which, of, K, cap, outside, finish, tile, lds, None)

    refused = [z(ids=None), z(out=None), z(dims=None), z(pitch=24), z(pitch=0), z(dims=d(4, 4, 17)), z(dims=d(0, 4, 4)),
               z(dims=d(4, 65537, 4)), z(cap=65536), z(K=256), z(of=64), z(of=254),
               axis(source=None), axis(out=None), axis(dims=None), axis(pitch=8), axis(pitch=20), axis(dims=d(4, 4, 0)),
               axis(dims=d(65537, 4, 4)), axis(cap=65536), axis(K=256), axis(of=100), axis(which=2), axis(finish=3),
               axis(finish=1, ids=p), axis(finish=1, counts=p), axis(finish=2, ids=p, counts=p, out=None),
               axis(tile=0), axis(K=97, cap=65535, tile=64), axis(K=2, tile=253), axis(outside=3)]
    assert refused == [-3] * len(refused)
    assert b"outside" in lib.hu_last_error()
    assert z(K=256) == -3 and b"255" in lib.hu_last_error()
    assert z(pitch=24) == -3 and b"16" in lib.hu_last_error()


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
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, and the VGPR counts
    and LDS sizes written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_thickness.hip" in builder.SOURCES and "instance_thickness.hip" not in builder.FLAGGED_SOURCES
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_thickness.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_thickness.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"(k_thick_z|k_thick_axis)IL([bi])([012])ELb([01])EEEvNS_9ThickArgsE", name)
        assert m, name
        first = {"b": {"1": "true", "0": "false"}, "i": {"0": "0", "1": "1", "2": "2"}}[m.group(2)][m.group(3)]
        kernel = "%s<%s, %s>" % (m.group(1), first, {"1": "true", "0": "false"}[m.group(4)])
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[kernel] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)))
    assert found == documented_resources()
    assert max(lds for _, lds in found.values()) == tw.LDS_ROWS * 128
