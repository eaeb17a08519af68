"""The references and the scenarios of test_gpu_wall_thickness.py and test_gpu_thickness_local.py, and the host side of
wall_thickness(), checked without a device.

wall_thickness_scenes.reference_thickness is written from the definition, offset by offset; opening_thickness takes the greatest
opening that keeps a sample, with the openings of thin_walls_scenes.  That both give the same map on every scenario and on
seeded random volumes is the first test -- it is the proof of WHAT IT MEANS in codecad_amd/wall_thickness.py; what follows from
the definition is the second."""
import ctypes
import math
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

import thin_walls_scenes as thin
import wall_thickness_scenes as scenes
from wall_thickness_scenes import CASES, NAMES, BY_NAME, reference, scene, SOLID, EMPTY

wt = sys.modules["codecad_amd.wall_thickness"]         # (the package's attribute of that name is the function)
tw = sys.modules["codecad_amd.thin_walls"]
ac = sys.modules["codecad_amd.assembly_components"]
av = sys.modules["codecad_amd.assembly_voxels"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_thick_local<0, 256>": 0, "k_thick_local<4, 256>": 4, "k_thick_local<10, 512>": 10, "k_thick_local<16, 1024>": 16}


def consequences(ids, of, r2, n, ref):
    """What the definition implies, on one volume."""
    s, depth, L = ref.in_set, ref.depth_sq.astype(numpy.int64), ref.thickness_sq.astype(numpy.int64)
    assert (L[~s] == 0).all() and (L[s] >= depth[s]).all() and (depth[s] >= 1).all() and L.max() <= r2 + 1
    # {L <= R2} is the thin set of the opening by the ball of R2: thin_walls with cover_sq = radius_sq
    opened = thin.reference_thin(ids, of, r2, r2, n)
    assert numpy.array_equal(opened.depth_sq, ref.depth_sq)
    assert numpy.array_equal((L > 0) & (L <= r2), opened.thin_ids != EMPTY)
    assert ref.core_counts == opened.core_counts
    # the uncapped map agrees wherever it is at most R2 (and only there need it)
    uncapped = scenes.uncapped_thickness(s)
    small = s & (uncapped <= r2)
    assert numpy.array_equal(L[small], uncapped[small]) and (L[s & (uncapped > r2)] <= r2 + 1).all()
    assert (numpy.minimum(uncapped, r2 + 1) >= L).all()                              # capping the uncapped map never reads less
    if r2 == 0:
        assert (L[s] == 1).all()
    # the per-part fields restated
    for k in range(n):
        own = L[(ids == k) & s]
        assert ref.min_sq[k] == (int(own.min()) if own.size else None)
        assert ref.capped_counts[k] == int((own == r2 + 1).sum())
        if own.size:
            x, y, z = ref.thinnest[k]
            assert ids[x, y, z] == k and L[x, y, z] == ref.min_sq[k]
            flat = numpy.flatnonzero(((ids == k) & s & (L == ref.min_sq[k])).ravel())
            assert flat[0] == numpy.ravel_multi_index((x, y, z), ids.shape)
        else:
            assert ref.thinnest[k] is None


# ---- the references ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_the_consequences_hold_on_every_scenario(name):
    c, ref = BY_NAME[name], reference(name)
    ids, n = scenes.part_ids(c.scene), len(scene(c.scene)[2])
    consequences(ids, c.of, c.r2, n, ref)
    assert ref.in_set.any() and max(ids.shape) <= 70 and ref.counts == [int((ids == k).sum()) for k in range(n)]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree_on_the_scenarios(name):
    c, ref = BY_NAME[name], reference(name)
    assert numpy.array_equal(scenes.opening_thickness(scenes.part_ids(c.scene), c.of, c.r2, len(scene(c.scene)[2])), ref.thickness_sq)


@pytest.mark.parametrize("seed", range(40))
def test_random_volumes(seed):
    ids, of, r2, n = scenes.random_volume(seed)
    ref = scenes.reference_thickness(ids, of, r2, n)
    assert numpy.array_equal(scenes.opening_thickness(ids, of, r2, n), ref.thickness_sq)
    consequences(ids, of, r2, n, ref)


def test_the_capped_map_is_not_the_capped_uncapped_map():
    """Digital openings are not nested: somewhere on the random volumes a sample reads at most R2 under the cap although a ball
    of a squared radius above R2 contains it -- so L is defined with the cap, not cut off afterwards."""
    found = 0
    for seed in range(40):
        ids, of, r2, n = scenes.random_volume(seed)
        s = thin.in_set_of(ids, of)
        uncapped = scenes.uncapped_thickness(s)
        L = scenes.reference_thickness(ids, of, r2, n).thickness_sq
        found += int(((L <= r2) & (uncapped > r2) & s).sum())
    assert found > 0


def test_a_line_by_hand():
    ids = numpy.zeros((1, 1, 9), dtype=numpy.uint8)
    ids[0, 0, 7] = EMPTY                                                             # a line: every sample is 1 from the outside
    ref = scenes.reference_thickness(ids, SOLID, 4, 1)
    assert ref.thickness_sq.ravel().tolist() == [1] * 7 + [0, 1] and ref.min_sq == [1] and ref.thinnest == [(0, 0, 0)]
    wide = numpy.zeros((9, 9, 9), dtype=numpy.uint8)                                 # a cube of 9: the middle is 5 deep
    ref = scenes.reference_thickness(wide, SOLID, 16, 1)
    assert ref.depth_sq[4, 4].tolist() == [1, 4, 9, 16, 17, 16, 9, 4, 1] and ref.core_counts == [1] and ref.capped_counts[0] > 1
    assert ref.thickness_sq[4, 4].tolist() == [17] * 9                               # the ball of the centre, 16 < 17, covers its axis
    assert ref.thickness_sq[0, 0, 0] == 4 and ref.min_sq == [4] and ref.thinnest == [(0, 0, 0)]      # the ball of (1, 1, 1): 3 < 4; of (2, 2, 2): 12 >= 9
    two = numpy.zeros((4, 1, 1), dtype=numpy.uint8)
    two[2:] = 1
    ref = scenes.reference_thickness(two, 1, 4, 2)
    assert ref.thickness_sq.ravel().tolist() == [0, 0, 1, 1] and ref.min_sq == [None, 1] and ref.thinnest == [None, (2, 0, 0)]


@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("w", range(1, 8))
def test_the_slab_rule(axis, w):
    """A slab of w samples normal to `axis`, 24 x 24 otherwise, reads ceil(w / 2)^2 throughout the samples at least ceil(w / 2)
    from its rim while that is at most R2, the cap otherwise; the scenario of that name holds the same."""
    half = -(-w // 2)
    shape = [24, 24, 24]
    shape[axis] = w
    for r2 in (1, 4, 9, 16):
        L = scenes.reference_thickness(numpy.zeros(shape, numpy.uint8), SOLID, r2, 1).thickness_sq
        inner = [slice(half - 1, 24 - half + 1)] * 3
        inner[axis] = slice(None)
        assert (L[tuple(inner)] == (half * half if half * half <= r2 else r2 + 1)).all(), (w, r2)
    ref = reference("slab_%s_w%d" % ("xyz"[axis], w))
    dims = list(ref.ids.shape)
    assert dims[axis] == w and sorted(dims)[1:] == [scenes.PLATE] * 2
    inner = [slice(half - 1, scenes.PLATE - half + 1)] * 3
    inner[axis] = slice(None)
    assert (ref.thickness_sq[tuple(inner)] == (half * half if half * half <= scenes.SLAB_R2 else scenes.SLAB_R2 + 1)).all()


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def test_the_rib_reads_its_width_and_the_body_the_cap():
    ref = reference("rib")
    assert (ref.thickness_sq[5:7, 2:10, 12:16] == 1).all()                           # the rib, 2 wide, above its root
    assert (ref.thickness_sq[14:22, 2:10, 0:2] == 1).all()                           # the floor, 2 thick
    assert (ref.thickness_sq[3:9, 3:9, 3:7] == 5).all() and ref.min_sq == [1] and ref.capped_counts[0] > 500
    assert reference("rib_r25").thickness_sq[6, 6, 5] == 26 and (reference("cuboid_5_r0").thickness_sq == 1).all()


def test_the_wedge_reads_its_steps():
    ref = reference("wedge")
    middle = ref.thickness_sq[:, 6, :]
    assert middle[3, 1] == 1 and middle[4, 5] == 4 and middle[2, 9] == 9 and middle[4, 14] == 10
    assert set(numpy.unique(ref.thickness_sq).tolist()) >= {0, 1, 4, 9, 10}


def test_the_ball_meets_every_kernel_and_ownership_decides():
    assert math.isqrt(BY_NAME["ball_r16"].r2) == 4 and math.isqrt(BY_NAME["ball_r81"].r2) == 9 and math.isqrt(BY_NAME["ball_r144"].r2) == 12
    assert reference("ball_r81").capped_counts[0] > 0 and reference("ball_r144").capped_counts == [0]
    assert reference("ball_r144").thickness_sq.max() > 81
    solid, plate, block = reference("glued_solid"), reference("glued_plate"), reference("glued_block")
    assert plate.min_sq == [1, None] and solid.min_sq[0] > 1 and block.min_sq[0] is None and block.min_sq[1] == solid.min_sq[1]
    pin, bored = reference("pressed_pin"), reference("pressed_block")
    assert pin.min_sq == [1, None] and pin.capped_counts == [0, 0] and bored.min_sq[1] < 5 and bored.capped_counts[1] > 0
    dims = [int(d) for d in scene("ragged")[5]]
    assert dims == [13, 9, 11] and av.volume_shape(dims, 2 ** 32)[2] == 16 > dims[2]
    assert reference("ragged_r400").capped_counts == [0] and reference("ragged_r1024").thickness_sq.max() < 100
    assert numpy.array_equal(reference("ragged_r400").thickness_sq, reference("ragged_r1024").thickness_sq)


def test_the_raw_cases_hold_their_edges():
    by = scenes.RAW_BY_NAME
    assert {math.isqrt(c.r2) for c in by.values()} >= {0, 1, 2, 4, 9, 10, 12, 32}
    assert by["narrow_r1024"].ids.shape == (5, 20, 7) and max(by["narrow_r1024"].ids.shape) < 32
    for axis, sides in ((0, (7, 8, 9, 63, 64, 65)), (1, (7, 8, 9, 63, 64, 65)), (2, (15, 16, 17, 63, 64, 65))):
        assert set(sides) <= {c.ids.shape[axis] for c in by.values()}
    assert {c.of for c in by.values()} == {SOLID, 0, 3}
    for name in scenes.RAW_NAMES:
        c = by[name]
        out, keys, counts = scenes.raw_reference(name)
        s = thin.in_set_of(c.ids, c.of)
        counted = numpy.where(s, c.field, 0)
        assert (out >= counted).all() and (out[counted == 0] == 0).all() and out.max() <= c.r2 + 1
        ids, field, pz = scenes.raw_buffers(c)
        assert pz % 16 == 0 and (field[:, :, :c.ids.shape[2]][~s] == c.r2 + 1).all() and (field[:, :, c.ids.shape[2]:] == c.r2 + 1).all()
        assert thin.in_set_of(ids[:, :, c.ids.shape[2]:], c.of).all()
        if not name.startswith(("one_sample", "all_cap", "ties")) and c.r2 > 0:
            assert (out > counted).any(), name                                     # some ball reaches a neighbour
    out, keys, counts = scenes.raw_reference("ball_on_a_corner")
    x, y, z = numpy.indices(out.shape)
    assert numpy.array_equal(out == 50, (x - 8) ** 2 + (y - 8) ** 2 + (z - 16) ** 2 < 50) and (out[out != 50] == 1).all()
    assert (out[:8, :8, :16] == 50).any() and (out[8:, 8:, 16:] == 50).any() and int((out == 50).sum()) > 1000
    assert int(keys[0]) == 1 << 48 and int(keys[1]) == scenes.NO_KEY                 # the first sample out of the ball: (0, 0, 0)
    base = scenes.raw_reference("low_r9")
    assert int(scenes.RAW_BY_NAME["low_r9"].field.max()) == 10
    for name in scenes.LOW_NAMES:
        assert numpy.array_equal(scenes.raw_reference(name)[0], base[0]) and numpy.array_equal(scenes.raw_reference(name)[1], base[1])
        assert (sum(scenes.raw_reference(name)[2]) > 0) == (name == "low_r9")
    out, keys, counts = scenes.raw_reference("all_cap_r400")
    assert (out == 401).all() and sum(counts) == out.size
    out, keys, counts = scenes.raw_reference("ties")
    ids = by["ties"].ids
    for p in range(3):
        first = numpy.argwhere(ids == p)[0]
        assert int(keys[p]) == 1 << 48 | int(first[0]) << 32 | int(first[1]) << 16 | int(first[2]) and (ids == p).sum() > 1
    assert (out == 1).all() and scenes.raw_reference("one_sample_empty")[0][0, 0, 0] == 0
    assert scenes.raw_reference("one_sample_cap")[2][0] == 1 and scenes.raw_reference("one_sample_low")[2][0] == 0


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_the_radius_rule():
    step = numpy.float32(1 / 16)
    assert wt.radius(step, 0.25) == 4 == tw.radii(step, 0.25)[0] and wt.radius(step, 0.3) == 5 and wt.radius(step, 0) == 0
    assert wt.radius(step, radius_sq=1024) == 1024 and wt.radius(step, 4.0) == 1024 and wt.radius(step, None, numpy.int64(7)) == 7
    for v in (0.1, 0.37, 1.0, 2.5, 3, numpy.float32(0.7), True):                     # the rule of thin_walls.radii, value for value
        assert wt.radius(step, v) == tw.radii(step, v, cover_sq=tw.MAX_COVER_SQ)[0]
    for bad in (-1, float("nan"), float("inf"), None, "1"):                          # ... and its refusals
        with pytest.raises(ValueError):
            tw.radii(step, bad)
    for bad in (4.01, 1000.0, -1, float("nan"), float("inf"), None, "1"):
        with pytest.raises(ValueError, match="max_thickness"):
            wt.radius(step, bad)
    for bad in (1025, -1, 1.0, True, "4"):
        with pytest.raises(ValueError, match="radius_sq"):
            wt.radius(step, None, bad)


def test_refusals_and_exports():
    one = cc.assembly("one", [shapes.sphere(r=1).make_part("ball")])
    for bad in ("void", None, ac.EMPTY_SPACE, 1, -1, 64, True, 0.0):
        with pytest.raises(ValueError):
            cc.wall_thickness(one, 0.5, 1.0, of=bad)
    for kwargs in ({}, {"max_thickness": -1}, {"radius_sq": 1025}, {"max_thickness": 1000.0}):
        with pytest.raises(ValueError):
            cc.wall_thickness(one, 0.5, **kwargs)
    with pytest.raises(ValueError):
        cc.wall_thickness(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1, 0.3)
    with pytest.raises(ValueError):
        cc.wall_thickness(one, -1, 0.3)
    assert {"wall_thickness", "WallThicknessReport"} <= set(cc.__all__) and "wall_thickness(" in cc.__doc__
    assert cc.wall_thickness is wt.wall_thickness and cc.WallThicknessReport is wt.WallThicknessReport
    assert wt.SAMPLE_BYTES == 7 and wt.MAX_RADIUS_SQ == 1024 == scenes.MAX_RADIUS_SQ and wt.LDS_K == 16
    for word in ("DEPTH", "THICKNESS", "WHAT IT MEANS", "SLABS", "THE CAP", "PER PART", "OUT OF SCOPE", "not nested", "EMPTY space",
                 "retire=True", "64 instances", "several devices", "pictures", "7 bytes a sample", "ceil(w / 2)^2"):
        assert word in wt.__doc__, word


def test_no_visible_instance_gives_the_empty_report():
    ghost = shapes.box(1).make_part("ghost").hidden()
    nothing = cc.assembly("nothing", [ghost])
    report = cc.wall_thickness(nothing, 0.1, 0.3, max_bytes=7 * 16)
    assert report.traversals == 0 and report.instances == [] and report.radius_sq == 2 and report.cap == 3 and report.of == SOLID
    assert report.counts == [] == report.core_counts == report.capped_counts == report.min_sq == report.thinnest
    for volume in (report.depth_sq, report.thickness_sq):
        assert volume.shape == (1, 1, 1) and volume.dtype == numpy.uint16 and volume[0, 0, 0] == 0
    assert report.thinnest_part() is None and not report.below(2).any() and report.diameters()[0, 0, 0] == 0.0
    with pytest.raises(ValueError, match="max_bytes"):
        cc.wall_thickness(nothing, 0.1, 0.3, max_bytes=7 * 16 - 1)
    with pytest.raises(ValueError):
        cc.wall_thickness(nothing, 0.1, 0.3, of=0)


def test_the_methods_of_the_report():
    L = numpy.array([[[0, 1, 4, 5, 9, 10]]], dtype=numpy.uint16)
    report = wt.WallThicknessReport([], None, numpy.float32(0.5), (1, 1, 6), SOLID, 9, None, None, L, [3, 0, 3], [0, 0, 0], [0, 0, 1],
                                    [4, None, 1], [(0, 0, 2), None, (0, 0, 1)], 0, 0)
    assert report.cap == 10 and report.below(4).ravel().tolist() == [False, True, True, False, False, False]
    assert report.below(9).ravel().tolist() == [False, True, True, True, True, False]
    assert report.diameters().ravel().tolist() == [0.0, 1.0, 2.0, 2 * math.sqrt(5) * 0.5, 3.0, math.inf]
    assert report.thinnest_part() == 2 and report._replace(min_sq=[4, None, 4]).thinnest_part() == 0
    assert report._replace(min_sq=[None] * 3).thinnest_part() is None


def fake_device(monkeypatch, keys, counts):
    """wall_thickness() over a library that records its calls; the keys read as `keys`, the accumulators as `counts`."""
    calls = []

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x1000000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            calls.append(("read", self.device_ptr))
            out = numpy.zeros(self.shape, self.dtype)
            if self.dtype == numpy.uint64:
                out[...] = keys if len(self.shape) == 1 else counts
            else:
                out[...] = self.device_ptr >> 24
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
    for module in (av, wt):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


@pytest.mark.parametrize("lds", [True, False])
def test_the_driver_runs_transform_1_then_the_gather_and_reads_back_once(monkeypatch, lds):
    asm, resolution = scene("plate_on_block")[:2]
    keys = numpy.full(64, scenes.NO_KEY, dtype=numpy.uint64)
    keys[0] = 3 << 48 | 1 << 32 | 2 << 16 | 11
    counts = numpy.arange(100, 228, dtype=numpy.uint64).reshape(2, 64)
    calls = fake_device(monkeypatch, keys, counts)
    report = cc.wall_thickness(asm, resolution, of=1, radius_sq=5, lds=lds, initial_capacity=7, max_bytes=7 * 12 * 12 * 16)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names == ["buffer", "hu_memset", "traverse", "read",                       # the ids, as assembly_voxels() leaves them
                     "buffer", "buffer", "buffer", "buffer", "buffer", "hu_memset", "hu_memset",      # one memset each: keys, counts
                     "hu_thickness_pass_z", "hu_thickness_pass_axis", "hu_thickness_pass_axis", "hu_thickness_local",
                     "read", "read", "read", "read",                                  # one read-back, after the last launch
                     "release", "release", "release", "release", "release", "release"]
    assert "hu_stream_synchronize" not in names and calls[2][1:] == (7, 1)          # retire=True, the cell lists' capacity
    ids, depth, other, out, key_buffer, acc = (0x1000000 * k for k in (1, 2, 3, 4, 5, 6))
    u16, u64, shape = numpy.dtype(numpy.uint16), numpy.dtype(numpy.uint64), (12, 12, 16)
    assert [c[1:] for c in calls if c[0] == "buffer"] == [(numpy.dtype(numpy.uint8), shape), (u16, shape), (u16, shape), (u16, shape),
                                                          (u64, (64,)), (u64, (2, 64))]
    assert calls[9][1] == (key_buffer, 0xff, 512, 0x99) and calls[10][1] == (acc, 0, 1024, 0x99)
    flag = int(lds)
    z1, y1, x1, local = (calls[k][1] for k in (11, 12, 13, 14))
    assert (z1[:3], list(z1[3]), z1[4:]) == ((ids, None, depth), [12, 12, 12], (16, 1, 5, 2, 6, flag, 0x99))
    tile = (252, 1) if lds else (64, 0)
    #            in, out, ids, thin, counts | pitch, axis, of, K, cap, outside, finish, tile, lds, stream
    assert y1[:5] + y1[6:] == (depth, other, None, None, None, 16, 1, 1, 2, 6, 0, 0) + tile + (0x99,)
    assert x1[:5] + x1[6:] == (other, depth, ids, None, acc, 16, 0, 1, 2, 6, 0, 1) + tile + (0x99,)
    #            depth, ids, out, keys, counts | pitch, of, radius_sq, lds, stream
    assert local[:5] + local[6:] == (depth, ids, out, key_buffer, acc + 512, 16, 1, 5, flag, 0x99)
    assert all(list(c[5]) == [12, 12, 12] for c in (y1, x1, local))
    assert [c[1] for c in calls[15:19]] == [depth, out, key_buffer, acc]
    assert sorted(c[1] for c in calls[19:]) == [ids, depth, other, out, key_buffer, acc]
    assert (report.of, report.radius_sq, report.cap) == (1, 5, 6) and report.counts == [5, 6]
    assert report.core_counts == [100, 101] and report.capped_counts == [164, 165] and report.min_sq == [3, None]
    assert report.thinnest == [(1, 2, 11), None] and report.thinnest_part() == 0
    assert all(type(v) is int for v in report.core_counts + report.capped_counts + [report.min_sq[0]] + list(report.thinnest[0]))
    for volume, value, dtype in ((report.depth_sq, 2, numpy.uint16), (report.thickness_sq, 4, numpy.uint16), (report.part_ids, 1, numpy.uint8)):
        assert volume.shape == (12, 12, 12) and (volume == value).all() and volume.dtype == dtype
    assert report.depth_sq.flags.c_contiguous and report.thickness_sq.flags.c_contiguous
    assert report.traversals == 2 and report.samples_evaluated == 77


def test_max_bytes_counts_seven_bytes_a_sample_before_any_launch(monkeypatch):
    asm, resolution = scene("ragged")[:2]
    calls = fake_device(monkeypatch, 0, 0)
    with pytest.raises(ValueError, match="max_bytes"):
        cc.wall_thickness(asm, resolution, 0.25, max_bytes=7 * 13 * 9 * 16 - 1)
    with pytest.raises(ValueError):
        cc.wall_thickness(asm, resolution, 0.25, of=1)
    with pytest.raises(ValueError):
        cc.wall_thickness(asm, resolution, radius_sq=1025)
    assert calls == []
    cc.wall_thickness(asm, resolution, radius_sq=400, max_bytes=7 * 13 * 9 * 16)
    monkeypatch.undo()
    launched = [c for c in calls if c[0].startswith("hu_thickness")]
    assert [c[0] for c in launched] == ["hu_thickness_pass_z", "hu_thickness_pass_axis", "hu_thickness_pass_axis", "hu_thickness_local"]
    assert launched[0][1][5:10] == (255, 400, 20, 401, 1) and launched[3][1][7:10] == (255, 400, 1)      # SOLID, R2, K, cap


# ---- the C ABI, the entry point's refusals and the kernels' resources -------------------------------------------------

def test_abi_of_the_new_entry_point():
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    name = "hu_thickness_local"
    args = ["const void* depth_dev", "const void* ids_dev", "void* out_dev", "uint64_t* keys_dev", "uint64_t* counts_dev",
            "const uint32_t dims[3]", "uint32_t pitch", "uint32_t of", "uint32_t radius_sq", "int lds", "void* stream"]
    assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    assert [" ".join(a.split()) for a in proto.split(",")] == args and len(_lib.PROTOTYPES[name]) == len(args)
    assert ("int %s(" % name) in integration
    assert sorted(_lib.PROTOTYPES) == _lib.header_symbols()
    constant = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))   # noqa: E731
    assert constant("HU_LOCAL_MAX_RADIUS_SQ") == wt.MAX_RADIUS_SQ == 1024 and constant("HU_LOCAL_LDS_K") == wt.LDS_K
    tile = tuple(constant("HU_COMPONENTS_TILE_" + a) for a in "XYZ")
    assert tile == scenes.TILE
    halo = constant("HU_LOCAL_LDS_K")
    assert constant("HU_LOCAL_LDS_BYTES") == 2 * math.prod(t + 2 * halo for t in tile) + 4 * 16 <= 160 * 1024
    assert constant("HU_THICKNESS_SOLID") == av._SOLID_CODE == EMPTY
    assert constant("HU_ABI_VERSION") == 3 == lib.hu_abi_version()                    # additive: the version stayed


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def local(depth=p, ids=p + 0x1000, out=p + 0x2000, keys=p + 0x3000, counts=p + 0x4000, dims=d(4, 4, 4), pitch=16, of=255, r2=4, lds=1):
        return lib.hu_thickness_local(depth, ids, out, keys, counts, dims, pitch, of, r2, lds, None)

    refused = [local(depth=None), local(ids=None), local(out=None), local(keys=None), local(counts=None), local(dims=None),
               local(pitch=24), local(pitch=0), local(pitch=8), local(dims=d(4, 4, 17)), local(dims=d(0, 4, 4)), local(dims=d(4, 0, 4)),
               local(dims=d(4, 4, 0)), local(dims=d(65537, 4, 4)), local(of=64), local(of=254), local(of=256), local(r2=1025),
               local(r2=2 ** 31), local(depth=p + 1), local(out=p + 0x2001), local(keys=p + 0x3004), local(counts=p + 0x4004),
               local(keys=p + 0x3001), local(out=p), local(lds=0, r2=1025)]
    assert refused == [-3] * len(refused)
    assert local(r2=1025) == -3 and b"radius_sq" in lib.hu_last_error() and b"1024" in lib.hu_last_error()
    assert local(pitch=24) == -3 and b"16" in lib.hu_last_error() and b"pitch" in lib.hu_last_error()
    assert local(keys=p + 0x3004) == -3 and b"keys" in lib.hu_last_error() and b"aligned" in lib.hu_last_error()
    assert local(counts=p + 0x4004) == -3 and b"counts" in lib.hu_last_error()
    assert local(depth=p + 1) == -3 and b"aligned to 2" in lib.hu_last_error()
    assert local(out=p) == -3 and b"overlap" in lib.hu_last_error()
    assert local(ids=None) == -3 and b"NULL" in lib.hu_last_error()
    assert local(of=64) == -3 and b"HU_THICKNESS_SOLID" in lib.hu_last_error()
    assert local(dims=d(4, 4, 0)) == -3 and b"dims" in lib.hu_last_error()


def documented_resources():
    """{kernel: (VGPRs, LDS bytes)} as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    found = {}
    for name in KERNELS:
        m = re.search(r"`%s` (\d+) VGPRs and (\d+) B of LDS" % re.escape(name), text)
        assert m, "DESIGN.md section 9.5 states the VGPRs and the LDS of " + name
        found[name] = (int(m.group(1)), int(m.group(2)))
    return found


def test_the_kernels_use_no_scratch_and_the_lds_the_header_states(tmp_path):
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, the LDS of a window of
    the kernel's halo (none in the comparison arm) plus a word a wavefront, HU_LOCAL_LDS_BYTES at the most, and the VGPR counts
    and LDS written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_local.hip" in builder.SOURCES and "instance_local.hip" not in builder.FLAGGED_SOURCES
    with open(os.path.join(builder.CSRC, "instance_local.hip")) as f:
        source = f.read()
    assert '#include "id_volume.hpp"' in source
    for helper in ("in_set(", "lattice_of(", "check_of(", "__ballot(", "HU_COMPONENTS_TILE_X"):
        assert helper in source, helper
    with open(_lib.HEADER) as f:
        stated = int(re.search(r"#define HU_LOCAL_LDS_BYTES (\d+)", f.read()).group(1))
    documented = documented_resources()
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_local.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_local.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"13k_thick_localILj(\d+)ELj(\d+)EEEvNS_9LocalArgsE", name)
        assert m, name
        kernel = "k_thick_local<%s, %s>" % m.groups()
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[kernel] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)))
        assert int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", block).group(1)) == int(m.group(2))
    assert found == documented and set(found) == set(KERNELS)
    for kernel, halo in KERNELS.items():
        threads = int(kernel.split(", ")[1][:-1])
        window = 2 * math.prod(t + 2 * halo for t in scenes.TILE) if halo else 0
        assert found[kernel][1] == window + 4 * threads // 64, kernel
    assert max(lds for _, lds in found.values()) == stated
