"""The references and the scenarios of test_gpu_flow_length.py and test_gpu_geodesic_raw.py, and the host side of flow_length(),
checked without a device.

flow_length_scenes.reference_steps is written from the definition, frontier by frontier; reference_rounds emulates the device's
rounds of sweeps.  That both give the same field on every scenario and on seeded random volumes is the first test; what follows
from the definition is the second."""
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

import assembly_components_scenes as comp
import islands_scenes as isl
import flow_length_scenes as scenes
from flow_length_scenes import NAMES, BY_NAME, NONE, SOLID, EMPTY_SPACE, EMPTY, reference, scene

fl = sys.modules["codecad_amd.flow_length"]            # (the package's attribute of that name is the function)
av = sys.modules["codecad_amd.assembly_voxels"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_geo_seed", "k_geo_seed_list", "k_geo_sweep_lines", "k_geo_sweep_columns", "k_geo_stats")


def report_of(ids, of, d, n, step=0.5, source=None):
    """A FlowLengthReport over a field computed on the host."""
    st = scenes.stats(ids, of, d, n)
    return fl.FlowLengthReport([], None, numpy.float32(step), ids.shape, of, source, ids, d, [int((ids == k).sum()) for k in range(n)],
                               st.reached_counts, st.unreached_counts, st.sum_steps, st.farthest, 0, 0, 0, 0)


def consequences(ids, of, seeds, d, n):
    """What the definition implies, on one volume."""
    s = scenes.in_set_of(ids, of)
    seeds = seeds & s
    assert d.dtype == numpy.uint32 and (d[~s] == NONE).all() and numpy.array_equal(d == 0, seeds)
    reached = d != NONE
    for axis in range(3):                                                             # neighbours in S: both reached or neither, a step apart at most
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        both = s[lo] & s[hi]
        assert numpy.array_equal(reached[lo][both], reached[hi][both])
        pair = both & reached[lo]
        assert (numpy.abs(d[lo][pair].astype(numpy.int64) - d[hi][pair].astype(numpy.int64)) <= 1).all()
    labels = comp.flood_labels(s)                                                     # the components of S that hold a seed
    assert numpy.array_equal(reached, s & numpy.isin(labels, numpy.unique(labels[seeds])))
    manhattan = scenes.reference_steps(numpy.ones(s.shape, dtype=bool), seeds)        # in the whole cuboid every way is straight
    assert (d[reached] >= manhattan[reached]).all()
    st = scenes.stats(ids, of, d, n)
    if of != EMPTY_SPACE:
        assert sum(st.reached_counts) == int(reached.sum()) and sum(st.unreached_counts) == int((s & ~reached).sum())
        for k, far in enumerate(st.farthest):
            assert (far is None) == (st.reached_counts[k] == 0)
            if far is not None:
                assert ids[far[1]] == k and d[far[1]] == far[0] == d[(ids == k) & reached].max()
    return st


# ---- the references ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_the_references_agree_and_the_consequences_hold_on_every_scenario(name):
    c, ref = BY_NAME[name], reference(name)
    fields, rounds = scenes.reference_rounds(ref.in_set, ref.seeds)
    assert numpy.array_equal(fields[-1], ref.steps) and rounds == ref.rounds == len(fields) >= 1
    assert all((a >= b).all() for a, b in zip(fields, fields[1:]))                    # values only fall
    if rounds > 1:                                                                    # the last round changed nothing, every other one did
        assert numpy.array_equal(fields[-2], fields[-1]) and all(not numpy.array_equal(a, b) for a, b in zip(fields[:-1], fields[1:-1]))
    consequences(ref.ids, c.of, ref.seeds, ref.steps, len(scene(c.scene)[2]))
    assert max(ref.ids.shape) <= 70 and ref.seeds.any()


@pytest.mark.parametrize("seed", range(60))
def test_random_volumes(seed):
    ids, of, seeds = scenes.random_volume(seed)
    s = scenes.in_set_of(ids, of)
    d = scenes.reference_steps(s, seeds)
    fields, rounds = scenes.reference_rounds(s, seeds)
    assert numpy.array_equal(fields[-1], d) and rounds == len(fields)
    consequences(ids, of, seeds, d, 3)


@pytest.mark.parametrize("shape,density", [((9, 10, 70), 0.7), ((17, 5, 130), 0.6), ((12, 12, 12), 0.5)])
def test_random_volumes_across_words_from_a_plane(shape, density):
    rng = numpy.random.default_rng(sum(shape))
    s = rng.random(shape) < density
    seeds = scenes.layer_of(shape, 0, 0) & s
    d = scenes.reference_steps(s, seeds)
    fields, rounds = scenes.reference_rounds(s, seeds)
    print(shape, "rounds", rounds, "greatest d", int(d[d != NONE].max()), "unreached", int((s & (d == NONE)).sum()))
    assert numpy.array_equal(fields[-1], d) and rounds > 2 and (s & (d == NONE)).any()
    consequences(numpy.where(s, 0, EMPTY).astype(numpy.uint8), SOLID, seeds, d, 1)


def test_the_serpentine_takes_twelve_rounds_and_779_steps():
    ids, seeds = scenes.serpentine()
    s = scenes.in_set_of(ids, SOLID)
    d = scenes.reference_steps(s, seeds)
    fields, rounds = scenes.reference_rounds(s, seeds)
    assert rounds == 12 and int(d[s].max()) == 779 and (d[s] != NONE).all() and numpy.array_equal(fields[-1], d)
    assert scenes.farthest_of(d, s) == (779, (20, 0, 69))
    reached = [int((f != NONE).sum()) for f in fields]
    assert reached == sorted(reached) and reached[0] < reached[-2] == reached[-1]     # a turn costs about a round


def test_in_a_cuboid_the_distance_is_the_manhattan_distance():
    shape = (5, 7, 9)
    s = numpy.ones(shape, dtype=bool)
    points = [(0, 0, 0), (4, 3, 8), (2, 6, 1)]
    d = scenes.reference_steps(s, scenes.listed(shape, points))
    at = numpy.stack(numpy.indices(shape), axis=-1)
    want = numpy.min([numpy.abs(at - numpy.array(p)).sum(axis=-1) for p in points], axis=0)
    assert numpy.array_equal(d, want)
    fields, rounds = scenes.reference_rounds(s, scenes.listed(shape, points))
    assert numpy.array_equal(fields[0], want) and rounds == 2                         # straight ways: the first round finds them all


def test_values_by_hand():
    # a U-channel in a plane: down one leg, across, up the other
    ids = numpy.full((5, 1, 4), EMPTY, dtype=numpy.uint8)
    ids[0, 0, :] = ids[4, 0, :] = ids[:, 0, 0] = 0
    d = scenes.reference_steps(ids != EMPTY, scenes.listed(ids.shape, [(0, 0, 3)]))
    assert d[0, 0].tolist() == [3, 2, 1, 0] and d[:, 0, 0].tolist() == [3, 4, 5, 6, 7] and d[4, 0].tolist() == [7, 8, 9, 10]
    assert (d[1:4, 0, 1:] == NONE).all() and scenes.reference_rounds(ids != EMPTY, scenes.listed(ids.shape, [(0, 0, 3)]))[1] == 3
    # an L of two parts: of = 0 stops at the corner
    ell = numpy.full((3, 3, 1), EMPTY, dtype=numpy.uint8)
    ell[0, :, 0], ell[1:, 2, 0] = 0, 1
    seeds = scenes.listed(ell.shape, [(0, 0, 0)])
    assert scenes.reference_steps(ell != EMPTY, seeds)[:, :, 0].tolist() == [[0, 1, 2], [NONE, NONE, 3], [NONE, NONE, 4]]
    assert scenes.reference_steps(ell == 0, seeds)[:, :, 0].tolist() == [[0, 1, 2], [NONE] * 3, [NONE] * 3]
    st = scenes.stats(ell, SOLID, scenes.reference_steps(ell != EMPTY, seeds), 2)
    assert st == ([3, 2], [0, 0], [3, 7], [(2, (0, 2, 0)), (4, (2, 2, 0))])
    # two gates at the ends of a line meet halfway
    line = numpy.zeros((1, 1, 9), dtype=numpy.uint8)
    d = scenes.reference_steps(line == 0, scenes.listed(line.shape, [(0, 0, 0), (0, 0, 8)]))
    assert d.ravel().tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0] and scenes.farthest_of(d, line == 0) == (4, (0, 0, 4))
    line = numpy.zeros((1, 1, 8), dtype=numpy.uint8)
    d = scenes.reference_steps(line == 0, scenes.listed(line.shape, [(0, 0, 0), (0, 0, 7)]))
    assert d.ravel().tolist() == [0, 1, 2, 3, 3, 2, 1, 0] and scenes.farthest_of(d, line == 0) == (3, (0, 0, 3))      # the first of two


def test_a_sweep_by_hand_carries_through_runs_only_and_saturates():
    s = numpy.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=bool).reshape(1, 1, 8)
    field = numpy.array([5, NONE, NONE, 0, NONE, 2 ** 31, NONE, NONE - 1], dtype=numpy.uint32).reshape(1, 1, 8)
    out, lowered = scenes.swept(field, s, 2)
    assert out.ravel().tolist() == [5, 6, 7, 0, 2 ** 31 + 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 2] and lowered
    out, lowered = scenes.swept(numpy.array([NONE - 1, NONE, 7, NONE], dtype=numpy.uint32).reshape(1, 1, 4), numpy.array([1, 1, 0, 1], dtype=bool).reshape(1, 1, 4), 2)
    assert out.ravel().tolist() == [NONE - 1, NONE, 7, NONE] and not lowered        # NONE - 1 + 1 is NONE: nothing falls, nothing wraps
    again, lowered = scenes.swept(scenes.swept(field, s, 2)[0], s, 2)
    assert not lowered                                                                # a line is final after one sweep of it


def test_the_scenarios_hold_what_they_are_for():
    bend = reference("ubend_gate")
    assert bend.stats.farthest[0][0] > sum(bend.ids.shape) - 3 and bend.rounds == 3 and bend.stats.unreached_counts == [0]   # longer than any straight way
    solid, left, right = reference("pair_solid"), reference("pair_left"), reference("pair_right_unseeded_side")
    assert solid.stats.reached_counts == [288, 288] and left.stats.reached_counts == [288, 0] and left.stats.farthest[1] is None
    assert (left.steps[left.ids == 1] == NONE).all() and right.stats.reached_counts == [0, 288]
    void = reference("shell_void")
    cavity = comp.reference("shell", EMPTY_SPACE)
    sealed = numpy.zeros(void.ids.shape, dtype=bool)
    for c in cavity.components:
        if not c.touches_border:
            sealed |= cavity.labels == c.label
    assert sealed.any() and numpy.array_equal(void.in_set & (void.steps == NONE), sealed) and void.stats.unreached_counts == int(sealed.sum())
    assert numpy.array_equal(part_ids_of("shell_void"), comp.part_ids("shell"))
    up, down = reference("table_up"), reference("table_down")
    assert int(up.seeds.sum()) == 24 and int(down.seeds.sum()) == 128 and up.stats.farthest[0][0] > down.stats.farthest[0][0]
    for name, axis, direction in (("table_up", 2, True), ("table_down", 2, False), ("table_x", 0, True), ("tower_plate", 2, False)):
        ref = reference(name)
        assert numpy.array_equal(ref.seeds, isl.seeds(ref.in_set, axis, direction))   # the first layer of the islands reference
    tower = reference("tower_two_seeds")
    assert tower.ids.shape == (5, 4, 70) and int(tower.seeds.sum()) == 2 and not tower.in_set[2:, :, 62:66].any() and tower.in_set[0, 0, 63:65].all()
    assert reference("nothing_void").ids.shape == (1, 1, 1) and reference("nothing_void").steps[0, 0, 0] == 0


def part_ids_of(name):
    return reference(name).ids


# ---- the report's methods ---------------------------------------------------------------------------------------------

def test_the_methods_of_the_report():
    ids = numpy.full((5, 1, 4), EMPTY, dtype=numpy.uint8)
    ids[0, 0, :] = ids[:, 0, 0] = 0
    ids[4, 0, :] = 1
    ids[2, 0, 3] = 1                                                                  # of S, and no way to it
    seeds = scenes.listed(ids.shape, [(0, 0, 3)])
    d = scenes.reference_steps(ids != EMPTY, seeds)
    report = report_of(ids, SOLID, d, 2)
    assert report.unreached().sum() == 1 and report.unreached()[2, 0, 3] and report.unreached_counts == [0, 1]
    lengths = report.lengths()
    assert lengths[0, 0].tolist() == [1.5, 1.0, 0.5, 0.0] and lengths[2, 0, 3] == math.inf and math.isnan(lengths[1, 0, 1])
    assert report.farthest == [(6, (3, 0, 0)), (10, (4, 0, 3))] and report.last_to_fill() == (10, (4, 0, 3)) and report.last_to_fill(0) == (6, (3, 0, 0))
    assert report._replace(farthest=[None, None]).last_to_fill() is None and report._replace(farthest=[(3, (1, 0, 0)), (3, (0, 0, 2))]).last_to_fill() == (3, (0, 0, 2))
    way = report.path((4, 0, 3))
    assert way == [(4, 0, 3), (4, 0, 2), (4, 0, 1), (4, 0, 0), (3, 0, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3)]
    assert report.path((0, 0, 3)) == [(0, 0, 3)] and report.path(numpy.array([0, 0, 2])) == [(0, 0, 2), (0, 0, 3)]
    for bad in ((2, 0, 3), (1, 0, 1), (5, 0, 0), (0, 0, -1), (0, 0), "abc", None, (0.0, 0, 0)):
        with pytest.raises(ValueError):
            report.path(bad)
    L = numpy.where(ids != EMPTY, 4, 0).astype(numpy.uint16)
    ratio = report.ratio(L)
    assert ratio[4, 0, 3] == 10 / 4 and ratio[0, 0, 3] == 0 and ratio[2, 0, 3] == math.inf and math.isnan(ratio[1, 0, 1])
    with pytest.raises(ValueError):
        report.ratio(L[:, :, :2])
    void = report_of(ids, EMPTY_SPACE, scenes.reference_steps(ids == EMPTY, scenes.border_of(ids.shape) & (ids == EMPTY)), 2)
    assert void.reached_counts == 8 and void.unreached_counts == 0 and void.last_to_fill() == void.farthest == (0, (1, 0, 1))


@pytest.mark.parametrize("seed", range(12))
def test_a_path_descends_by_one_stays_in_the_set_and_follows_the_tie_order(seed):
    ids, of, seeds = scenes.random_volume(seed, shape=(6, 5, 7), density=0.8)
    s = scenes.in_set_of(ids, of)
    d = scenes.reference_steps(s, seeds)
    report = report_of(ids, of, d, 3)
    order = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    for p in numpy.argwhere(s & (d != NONE))[::7]:
        way = report.path(tuple(p))
        assert len(way) == int(d[tuple(p)]) + 1 and way[0] == tuple(p) and seeds[way[-1]]
        for a, b in zip(way, way[1:]):
            assert s[b] and int(d[b]) == int(d[a]) - 1
            step = tuple(int(v - u) for u, v in zip(a, b))
            for earlier in order[:order.index(step)]:                                 # no earlier neighbour would have done
                q = tuple(u + v for u, v in zip(a, earlier))
                assert not (all(0 <= v < n for v, n in zip(q, s.shape)) and s[q] and int(d[q]) == int(d[a]) - 1)


# ---- the seeds, on the host -------------------------------------------------------------------------------------------

def test_gates_map_to_the_nearest_sample_and_a_tie_to_the_lower_index():
    corner, step, dims = numpy.array([-1.0, 0.5, 2.0], dtype=numpy.float32), numpy.float32(0.25), (4, 3, 9)
    assert fl.positions(corner, step, 4, 0).tolist() == [-1.0, -0.75, -0.5, -0.25]
    got = fl.nearest_samples([[-1.0, 0.5, 2.0], [-0.26, 0.99, 4.0], [-0.875, 0.625, 3.125], [-1.125, 1.125, 4.125], [-0.62, 0.63, 2.124]], corner, step, dims)
    assert got.tolist() == [[0, 0, 0], [3, 2, 8], [0, 0, 4], [0, 2, 8], [2, 1, 0]]                 # the third and fourth: ties, the lower index / the rim
    for outside in ([-1.126, 0.5, 2.0], [-1.0, 1.13, 2.0], [-1.0, 0.5, 4.2], [-1.0, 0.5, 1.8]):
        with pytest.raises(ValueError, match="outside the lattice"):
            fl.nearest_samples([outside], corner, step, dims)
    for bad in ([[0.0, 0.0]], [0.0, 0.0, 0.0], [[math.nan, 0.5, 2.0]], [[math.inf, 0.5, 2.0]]):
        with pytest.raises(ValueError):
            fl.nearest_samples(bad, corner, step, dims)
    # float32 positions: a step that is no binary fraction
    corner, step = numpy.array([0.1, 0.1, 0.1], dtype=numpy.float32), numpy.float32(0.1)
    at = fl.positions(corner, step, 50, 2)
    assert at[37] == float(numpy.float32(0.1) + numpy.float32(0.1) * numpy.float32(37)) and at.dtype == numpy.float64
    assert fl.nearest_samples([[0.1, 0.1, at[37]]], corner, step, (1, 1, 50)).tolist() == [[0, 0, 37]]


def test_the_seeds_of_every_source():
    ids = numpy.full((4, 3, 5), EMPTY, dtype=numpy.uint8)
    ids[1:3, :, 1:4] = 0
    ids[3, 1, 4] = 1
    corner, step = numpy.zeros(3, dtype=numpy.float32), numpy.float32(1)
    assert fl.seeds_of(fl.BORDER, ids, SOLID, corner, step) == (0, 0, 0, None, 13)    # the faces y = 0 and y = 2 of part 0, and part 1
    assert fl.seeds_of(fl.BORDER, ids, EMPTY_SPACE, corner, step)[4] == 60 - 18 - 1                 # every empty sample lies on the rim
    assert fl.seeds_of(fl.Plate(), ids, SOLID, corner, step) == (1, 2, 1, None, 6)
    assert fl.seeds_of(fl.Plate(2, False), ids, SOLID, corner, step) == (1, 2, 4, None, 1)
    assert fl.seeds_of(fl.Plate(0, False), ids, 0, corner, step) == (1, 0, 2, None, 9)
    assert fl.seeds_of(fl.Plate(1, True), ids, 1, corner, step) == (1, 1, 1, None, 1)
    assert fl.seeds_of(fl.Plate(1), numpy.zeros((2, 2, 2), numpy.uint8), EMPTY_SPACE, corner, step) == (1, 1, 0, None, 0)      # S is empty
    mode, axis, layer, rows, count = fl.seeds_of(fl.Samples([(1, 0, 1), (2, 2, 3), (1, 0, 1)]), ids, SOLID, corner, step)
    assert (mode, count) == (2, 2) and rows.dtype == numpy.uint32 and rows.tolist() == [[1, 0, 1], [2, 2, 3], [1, 0, 1]] and rows.flags.c_contiguous
    mode, axis, layer, rows, count = fl.seeds_of(fl.Gates([(1.2, 0.4, 0.6), (3.4, 1.0, 4.0)]), ids, SOLID, corner, step)
    assert (mode, count) == (2, 2) and rows.tolist() == [[1, 0, 1], [3, 1, 4]]
    for bad in (fl.Samples([(0, 0, 0)]), fl.Samples([(1, 0, 0)]), fl.Samples([(4, 0, 0)]), fl.Samples([(0, 0, -1)]), fl.Samples([]),
                fl.Samples([(1.0, 0.0, 1.0)]), fl.Samples([1, 0, 1]), fl.Samples(numpy.zeros((65537, 3), dtype=numpy.int64) + 1),
                fl.Gates([(0.0, 0.0, 0.0)]), fl.Gates([(9.0, 0.0, 0.0)]), fl.Gates([]), fl.Plate(3), fl.Plate(True), "rim", None, 7):
        with pytest.raises(ValueError):
            fl.seeds_of(bad, ids, SOLID, corner, step)
    with pytest.raises(ValueError, match="not in the set"):
        fl.seeds_of(fl.Samples([(3, 1, 4)]), ids, 0, corner, step)                    # of part 1, and S is part 0
    assert fl.seeds_of(fl.Samples(numpy.zeros((65536, 3), dtype=numpy.int64) + 1), ids, SOLID, corner, step)[4] == 1


def test_refusals_and_exports():
    one = cc.assembly("one", [shapes.sphere(r=1).make_part("ball")])
    for bad in ("void", None, 1, -1, 64, True, 0.0):
        with pytest.raises(ValueError):
            cc.flow_length(one, 0.5, cc.BORDER, of=bad)
    with pytest.raises(ValueError):
        cc.flow_length(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1, cc.BORDER)
    with pytest.raises(ValueError):
        cc.flow_length(one, -1, cc.BORDER)
    with pytest.raises(ValueError, match="2\\^31"):
        fl._check_entries((2048, 2048, 513))
    fl._check_entries((2048, 2048, 512))
    assert {"flow_length", "FlowLengthReport", "Gates", "Samples", "Plate", "BORDER"} <= set(cc.__all__) and "flow_length(" in cc.__doc__
    assert cc.flow_length is fl.flow_length and cc.FlowLengthReport is fl.FlowLengthReport and cc.Plate() == (2, True) and cc.Gates is fl.Gates
    assert fl.SAMPLE_BYTES == 5 and fl.NONE == NONE == comp.NONE and fl.MAX_SEEDS == 65536 and fl.EMPTY_SPACE == cc.EMPTY_SPACE
    for word in ("THE SET S", "SEEDS", "STEPS", "PER PART", "OUT OF SCOPE", "retire=True", "64 instances", "several devices", "pictures",
                 "5 bytes a sample", "2^31", "Euclidean", "weld lines", "passable by a sphere", "a tie going to the lower index", "L/t"):
        assert word in fl.__doc__, word


def test_no_visible_instance_gives_the_empty_report_without_a_launch():
    nothing = scenes.scene("nothing")[0]
    report = cc.flow_length(nothing, 0.1, cc.Plate(), max_bytes=5 * 16)
    assert report.traversals == 0 and report.instances == [] and report.rounds == 0 and report.seed_count == 0 and report.of == SOLID
    assert report.counts == [] == report.reached_counts == report.unreached_counts == report.sum_steps == report.farthest
    assert report.steps.shape == (1, 1, 1) and report.steps.dtype == numpy.uint32 and report.steps[0, 0, 0] == NONE
    assert report.last_to_fill() is None and not report.unreached().any() and math.isnan(report.lengths()[0, 0, 0])
    assert cc.flow_length(nothing, 0.1, cc.BORDER).seed_count == 0
    with pytest.raises(ValueError, match="max_bytes"):
        cc.flow_length(nothing, 0.1, cc.Plate(), max_bytes=5 * 16 - 1)
    with pytest.raises(ValueError):
        cc.flow_length(nothing, 0.1, cc.Plate(), of=0)
    with pytest.raises(ValueError, match="not in the set"):
        cc.flow_length(nothing, 0.1, cc.Samples([(0, 0, 0)]))                         # S is empty: no sample can seed it


# ---- the driver, on the host ------------------------------------------------------------------------------------------

def fake_device(monkeypatch, keys, counts, words):
    """flow_length() over a library that records its calls; the keys read as `keys`, the accumulators as `counts`, the word of
    round k as words[k]."""
    calls, left = [], list(words)

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
            elif self.shape == (1,):
                out[0] = left.pop(0)
            else:
                out[...] = self.device_ptr >> 24
            return out

        def enqueue_write(self, a):
            calls.append(("write", self.device_ptr, numpy.array(a)))

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
    for module in (av, fl):
        monkeypatch.setattr(module, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


def test_the_driver_seeds_runs_rounds_until_a_word_stays_zero_and_reads_back_once(monkeypatch):
    asm, resolution = scene("pair")[:2]
    keys = numpy.zeros(65, dtype=numpy.uint64)
    keys[1] = (7 + 1) << 32 | (0xffffffff - ((3 * 6 + 2) * 16 + 5))
    counts = numpy.arange(100, 295, dtype=numpy.uint64).reshape(3, 65)
    calls = fake_device(monkeypatch, keys, counts, [1, 1, 0])
    # the ids read as 1 everywhere: the samples must be of part 1
    report = cc.flow_length(asm, resolution, cc.Samples([(1, 2, 3), (4, 5, 0)]), of=1, initial_capacity=7, max_bytes=5 * 16 * 6 * 16)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    round_ = ["hu_memset", "hu_geodesic_sweep", "hu_geodesic_sweep", "hu_geodesic_sweep", "read"]
    assert names == (["buffer", "hu_memset", "traverse", "read",                      # the ids, as assembly_voxels() leaves them
                      "buffer", "buffer", "buffer", "buffer", "hu_memset", "hu_memset", "buffer", "write", "hu_geodesic_seed"]
                     + round_ * 3 + ["hu_geodesic_stats", "read", "read", "read"] + ["release"] * 6)
    assert "hu_stream_synchronize" not in names and calls[2][1:] == (7, 1)          # retire=True, the cell lists' capacity
    ids, dist, key_buffer, acc, word, samples = (0x1000000 * k for k in (1, 2, 3, 4, 5, 6))
    u32, u64, shape = numpy.dtype(numpy.uint32), numpy.dtype(numpy.uint64), (16, 6, 16)
    assert [c[1:] for c in calls if c[0] == "buffer"] == [(numpy.dtype(numpy.uint8), shape), (u32, shape), (u64, (65,)), (u64, (3, 65)),
                                                          (u32, (1,)), (u32, (2, 3))]
    assert calls[8][1] == (key_buffer, 0, 520, 0x99) and calls[9][1] == (acc, 0, 1560, 0x99)
    assert calls[11][1] == samples and calls[11][2].tolist() == [[1, 2, 3], [4, 5, 0]] and calls[11][2].dtype == numpy.uint32
    seed = calls[12][1]
    #            ids, dist | pitch, of, mode, axis, layer, samples, n, stream
    assert seed[:2] + seed[3:] == (ids, dist, 16, 1, 2, 0, 0, samples, 2, 0x99) and list(seed[2]) == [16, 6, 6]
    for k in range(3):
        memset, z, y, x, read = calls[13 + 5 * k:18 + 5 * k]
        assert memset[1] == (word, 0, 4, 0x99) and read[1] == word
        for sweep, axis in ((z, 2), (y, 1), (x, 0)):
            #                      ids, dist, word | pitch, axis, of, stream
            assert sweep[1][:3] + sweep[1][4:] == (ids, dist, word, 16, axis, 1, 0x99) and list(sweep[1][3]) == [16, 6, 6]
    stats = calls[28][1]
    assert stats[:4] + stats[5:] == (ids, dist, key_buffer, acc, 16, 1, 0x99) and list(stats[4]) == [16, 6, 6]
    assert [c[1] for c in calls[29:32]] == [dist, key_buffer, acc] and sorted(c[1] for c in calls[32:]) == [ids, dist, key_buffer, acc, word, samples]
    assert (report.of, report.rounds, report.seed_count) == (1, 3, 2) and report.counts == [5, 6] and report.source == cc.Samples([(1, 2, 3), (4, 5, 0)])
    assert report.reached_counts == [100, 101] and report.unreached_counts == [165, 166] and report.sum_steps == [230, 231]
    assert report.farthest == [None, (7, (3, 2, 5))] and report.last_to_fill() == (7, (3, 2, 5))
    assert all(type(v) is int for v in report.reached_counts + report.unreached_counts + report.sum_steps + list(report.farthest[1][1]) + [report.farthest[1][0]])
    assert report.steps.shape == (16, 6, 6) and (report.steps == 2).all() and report.steps.dtype == numpy.uint32 and report.steps.flags.c_contiguous
    assert report.traversals == 2 and report.samples_evaluated == 77


def test_every_source_and_set_reaches_the_seed_launch_as_its_mode(monkeypatch):
    asm, resolution = scene("pair")[:2]
    calls = fake_device(monkeypatch, 0, 0, [0] * 8)
    cc.flow_length(asm, resolution, cc.BORDER, of=1)                                  # (the ids read as 1 everywhere)
    cc.flow_length(asm, resolution, cc.Plate(0, False), of=SOLID)
    with pytest.raises(ValueError, match="not in the set"):
        cc.flow_length(asm, resolution, cc.Samples([(0, 0, 0)]), of=EMPTY_SPACE)
    monkeypatch.undo()
    seeds = [c[1] for c in calls if c[0] == "hu_geodesic_seed"]
    assert [s[3:10] for s in seeds] == [(16, 1, 0, 0, 0, None, 0), (16, 255, 1, 0, 15, None, 0)]
    assert [c[0] for c in calls].count("hu_geodesic_stats") == 2 and [c[0] for c in calls].count("hu_geodesic_sweep") == 6
    assert [c[0] for c in calls].count("buffer") == [c[0] for c in calls].count("release")    # a refused seed releases the ids


def test_max_bytes_and_the_seeds_are_refused_before_any_launch(monkeypatch):
    asm, resolution = scene("pair")[:2]
    calls = fake_device(monkeypatch, 0, 0, [0])
    with pytest.raises(ValueError, match="max_bytes"):
        cc.flow_length(asm, resolution, cc.BORDER, max_bytes=5 * 16 * 6 * 16 - 1)
    with pytest.raises(ValueError):
        cc.flow_length(asm, resolution, cc.BORDER, of=2)
    monkeypatch.setattr(fl, "_check_entries", lambda dims: (_ for _ in ()).throw(ValueError("2^31")))
    with pytest.raises(ValueError, match="2\\^31"):
        cc.flow_length(asm, resolution, cc.BORDER)
    assert calls == []
    monkeypatch.undo()


def test_empty_space_of_nothing_visible_runs_on_a_volume_of_255s(monkeypatch):
    calls = fake_device(monkeypatch, 0, 0, [0])
    report = cc.flow_length(scenes.scene("nothing")[0], 0.1, cc.BORDER, of=EMPTY_SPACE)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names[:2] == ["buffer", "hu_memset"] and calls[0][1:] == (numpy.dtype(numpy.uint8), (1, 1, 16)) and calls[1][1][1:3] == (255, 16)
    assert "traverse" not in names and names.count("hu_geodesic_seed") == 1 and names.count("hu_geodesic_sweep") == 3
    seed = [c[1] for c in calls if c[0] == "hu_geodesic_seed"][0]
    assert seed[3:8] == (16, 254, 0, 0, 0) and report.rounds == 1 and report.seed_count == 1 and report.traversals == 0
    assert report.reached_counts == 0 and report.farthest is None                     # single values: what the fake device read back


# ---- the C ABI, the entry points' refusals and the kernels' resources -------------------------------------------------

ARGS = {
    "hu_geodesic_seed": ["const void* ids_dev", "void* dist_dev", "const uint32_t dims[3]", "uint32_t pitch", "uint32_t of", "int mode", "int axis",
                         "uint32_t layer", "const uint32_t* samples_dev", "uint32_t n_samples", "void* stream"],
    "hu_geodesic_sweep": ["const void* ids_dev", "void* dist_dev", "uint32_t* word_dev", "const uint32_t dims[3]", "uint32_t pitch", "int axis",
                          "uint32_t of", "void* stream"],
    "hu_geodesic_stats": ["const void* ids_dev", "const void* dist_dev", "uint64_t* keys_dev", "uint64_t* counts_dev", "const uint32_t dims[3]",
                          "uint32_t pitch", "uint32_t of", "void* stream"],
}


def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    for name, args in ARGS.items():
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == args and len(_lib.PROTOTYPES[name]) == len(args)
        assert ("int %s(" % name) in integration
    assert sorted(_lib.PROTOTYPES) == _lib.header_symbols()
    constant = lambda name: int(re.search(r"#define %s (\w+)" % name, header).group(1).rstrip("u"), 0)   # noqa: E731
    assert constant("HU_GEODESIC_SOLID") == av._SOLID_CODE == EMPTY == constant("HU_THICKNESS_SOLID")
    assert constant("HU_GEODESIC_EMPTY") == fl._EMPTY_CODE == scenes.VOID_CODE == 254 and constant("HU_GEODESIC_NONE") == fl.NONE
    assert (constant("HU_GEODESIC_BORDER"), constant("HU_GEODESIC_LAYER"), constant("HU_GEODESIC_LIST")) == (fl._MODE_BORDER, fl._MODE_LAYER, fl._MODE_LIST)
    assert (scenes.MODE_BORDER, scenes.MODE_LAYER, scenes.MODE_LIST) == (0, 1, 2) == (fl._MODE_BORDER, fl._MODE_LAYER, fl._MODE_LIST)
    assert constant("HU_GEODESIC_MAX_SAMPLES") == fl.MAX_SEEDS and constant("HU_GEODESIC_SLOTS") == fl._SLOTS == scenes.SLOTS == 65
    assert constant("HU_ABI_VERSION") == 3 == lib.hu_abi_version()                    # additive: the version stayed


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    d = lambda *v: (ctypes.c_uint32 * 3)(*v)                                          # noqa: E731
    p = 0x1000                                                                        # never dereferenced: every call is refused

    def seed(ids=p, dist=p + 0x1000, dims=d(4, 4, 4), pitch=16, of=255, mode=0, axis=0, layer=0, samples=None, n=0):
        return lib.hu_geodesic_seed(ids, dist, dims, pitch, of, mode, axis, layer, samples, n, None)

    def sweep(ids=p, dist=p + 0x1000, word=p + 0x2000, dims=d(4, 4, 4), pitch=16, axis=2, of=255):
        return lib.hu_geodesic_sweep(ids, dist, word, dims, pitch, axis, of, None)

    def stats(ids=p, dist=p + 0x1000, keys=p + 0x2000, counts=p + 0x3000, dims=d(4, 4, 4), pitch=16, of=255):
        return lib.hu_geodesic_stats(ids, dist, keys, counts, dims, pitch, of, None)

    for call in (seed, sweep, stats):                                                 # what all three take
        refused = [call(ids=None), call(dist=None), call(dims=None), call(pitch=24), call(pitch=0), call(pitch=8), call(dims=d(4, 4, 17)),
                   call(dims=d(0, 4, 4)), call(dims=d(4, 0, 4)), call(dims=d(4, 4, 0)), call(dims=d(65537, 4, 4)), call(of=64), call(of=253),
                   call(of=256), call(dist=p + 0x1002), call(dist=p + 0x1001), call(dims=d(32768, 65536, 1), pitch=16),
                   call(dims=d(65536, 32768, 2), pitch=16)]
        assert refused == [-3] * len(refused), call.__name__
        assert call(dims=d(32768, 65536, 1), pitch=16) == -3 and b"2^31" in lib.hu_last_error()
        assert call(pitch=24) == -3 and b"16" in lib.hu_last_error() and b"pitch" in lib.hu_last_error()
        assert call(of=64) == -3 and b"HU_GEODESIC_SOLID" in lib.hu_last_error() and b"HU_GEODESIC_EMPTY" in lib.hu_last_error()
        assert call(dist=p + 0x1002) == -3 and b"aligned to 4" in lib.hu_last_error()
        assert call(ids=None) == -3 and b"NULL" in lib.hu_last_error()
        assert call(dims=d(4, 4, 0)) == -3 and b"dims" in lib.hu_last_error()
    refused = [seed(mode=3), seed(mode=-1), seed(mode=1, axis=3), seed(mode=1, axis=-1), seed(mode=1, axis=2, layer=4), seed(mode=1, axis=0, layer=2 ** 31),
               seed(mode=2), seed(mode=2, samples=p + 0x4000, n=0), seed(mode=2, samples=p + 0x4000, n=65537), seed(mode=2, samples=p + 0x4002, n=1),
               seed(mode=2, samples=None, n=1)]
    assert refused == [-3] * len(refused)
    assert seed(mode=3) == -3 and b"mode" in lib.hu_last_error()
    assert seed(mode=1, axis=2, layer=4) == -3 and b"layer" in lib.hu_last_error()
    assert seed(mode=2, samples=p + 0x4000, n=65537) == -3 and b"65536" in lib.hu_last_error() and b"n_samples" in lib.hu_last_error()
    assert seed(mode=2, samples=p + 0x4002, n=1) == -3 and b"samples" in lib.hu_last_error() and b"aligned" in lib.hu_last_error()
    refused = [sweep(word=None), sweep(word=p + 0x2002), sweep(axis=3), sweep(axis=-1)]
    assert refused == [-3] * len(refused)
    assert sweep(word=p + 0x2002) == -3 and b"word" in lib.hu_last_error() and sweep(axis=3) == -3 and b"axis" in lib.hu_last_error()
    refused = [stats(keys=None), stats(counts=None), stats(keys=p + 0x2004), stats(counts=p + 0x3004), stats(keys=p + 0x2001)]
    assert refused == [-3] * len(refused)
    assert stats(keys=p + 0x2004) == -3 and b"keys" in lib.hu_last_error() and stats(counts=p + 0x3004) == -3 and b"counts" in lib.hu_last_error()


def documented_resources():
    """{kernel: (VGPRs, LDS bytes)} as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    found = {}
    for name in KERNELS:
        m = re.search(r"`%s` (\d+) VGPRs and (\d+) B of LDS" % re.escape(name), text)
        assert m, "DESIGN.md section 9.7 states the VGPRs and the LDS of " + name
        found[name] = (int(m.group(1)), int(m.group(2)))
    return found


def test_the_kernels_use_no_scratch_and_no_lds(tmp_path):
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, no LDS, and the VGPR
    counts written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_geodesic.hip" in builder.SOURCES and "instance_geodesic.hip" not in builder.FLAGGED_SOURCES
    with open(os.path.join(builder.CSRC, "instance_geodesic.hip")) as f:
        source = f.read()
    assert '#include "id_volume.hpp"' in source
    for helper in ("in_set(", "lattice_of(", "lattice_axis(", "check_of(", "column_unit(", "line_unit<", "HU_FOR_UNITS(", "walking_blocks(",
                   "gather_counts(", "__ballot(", "kBatch"):
        assert helper in source, helper
    with open(os.path.join(builder.CSRC, "id_volume.hpp")) as f:
        assert "return of == kSolid ? id != kEmpty : id == of;" in f.read()               # in_set is as it was
    documented = documented_resources()
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_geodesic.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_geodesic.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"\d+(k_geo_\w+?)ENS_7GeoArgsE", name)
        assert m, name
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", block).group(1)) == 256
        found[m.group(1)] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                             int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)))
    assert found == documented and set(found) == set(KERNELS)
    assert all(lds == 0 for _, lds in found.values())
