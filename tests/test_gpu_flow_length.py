"""flow_length() on the device against reference A of flow_length_scenes.py, written from the definition frontier by frontier, on
the reference part ids: the part ids, the steps, the per-part counts, sums and farthest samples and the number of seeds are
EQUAL to the reference, entry for entry, `rounds` is the number of rounds of reference B, the NumPy emulation of the device's
sweeps, and a second call gives the same bytes."""
import math

import numpy
import pytest

import codecad_amd as cc

import flow_length_scenes as scenes
from flow_length_scenes import NAMES, BY_NAME, NONE, SOLID, EMPTY_SPACE, reference, scene

pytestmark = pytest.mark.gpu


def run(name, **kwargs):
    c = BY_NAME[name]
    asm, resolution, instances, corner, step, dims = scene(c.scene)
    report = cc.flow_length(asm, resolution, c.source(), of=c.of, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert report.of == c.of and report.source == c.source() and len(report.instances) == len(instances)
    return report


def check_against_reference(report, ref):
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    got, want = report.steps, ref.steps
    assert got.dtype == numpy.uint32 and got.flags.c_contiguous and got.shape == want.shape
    wrong = numpy.argwhere(got != want)
    assert len(wrong) == 0, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]]
    assert report.reached_counts == ref.stats.reached_counts and report.unreached_counts == ref.stats.unreached_counts
    assert report.sum_steps == ref.stats.sum_steps and report.farthest == ref.stats.farthest
    assert report.seed_count == int(ref.seeds.sum()) and report.rounds == ref.rounds
    assert numpy.array_equal(report.unreached(), ref.in_set & (ref.steps == NONE))


@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name):
    ref = reference(name)
    report = run(name)
    print(name, ref.ids.shape, "rounds", report.rounds, "reference", ref.rounds, "farthest", report.farthest, "reference", ref.stats.farthest,
          "reached", report.reached_counts, "unreached", report.unreached_counts, "seeds", report.seed_count)
    check_against_reference(report, ref)
    assert report.traversals == (0 if name.startswith("nothing") else 1)
    again = run(name)                                                # a second call: nothing is left over from the first
    check_against_reference(again, ref)
    assert again.steps.tobytes() == report.steps.tobytes() and again.rounds == report.rounds


def test_the_way_over_the_bend_and_the_methods_follow_the_map(hip):
    report, ref = run("ubend_gate"), reference("ubend_gate")
    far, where = report.last_to_fill()
    assert (far, where) == ref.stats.farthest[0] and far > sum(ref.ids.shape) - 3
    way = report.path(where)
    assert len(way) == far + 1 and way[0] == where and ref.seeds[way[-1]] and all(ref.in_set[p] for p in way)
    assert [int(report.steps[p]) for p in way] == list(range(far, -1, -1))
    lengths = report.lengths()
    assert lengths[where] == far * float(report.step) and numpy.isnan(lengths[~ref.in_set]).all()
    thick = cc.wall_thickness(scene("ubend")[0], scene("ubend")[1], radius_sq=16)
    ratio = report.ratio(thick.thickness_sq)
    assert numpy.array_equal(thick.part_ids, report.part_ids) and ratio[where] == far / (2 * math.sqrt(int(thick.thickness_sq[where])))


def test_of_decides_where_the_way_ends(hip):
    solid, left = run("pair_solid"), run("pair_left")
    assert solid.reached_counts == [288, 288] and left.reached_counts == [288, 0] and left.farthest[1] is None
    assert (left.steps[left.part_ids == 1] == NONE).all() and solid.last_to_fill() == solid.farthest[1]
    void = run("shell_void")
    assert void.unreached_counts == reference("shell_void").stats.unreached_counts > 0 and isinstance(void.reached_counts, int)
    up, down = run("table_up"), run("table_down")
    assert up.seed_count == 24 and down.seed_count == 128 and up.farthest[0][0] > down.farthest[0][0]


def test_an_assembly_with_nothing_visible(hip):
    nothing = scene("nothing")[0]
    report = cc.flow_length(nothing, 0.1, cc.Plate())
    assert report.traversals == 0 and report.rounds == 0 and report.counts == [] == report.reached_counts == report.farthest
    assert (report.steps == NONE).all() and report.last_to_fill() is None
    void = cc.flow_length(nothing, 0.1, cc.BORDER, of=EMPTY_SPACE)   # every sample is empty: it runs on a volume of 255s
    assert void.steps.shape == (1, 1, 1) and void.steps[0, 0, 0] == 0 and void.rounds == 1 and void.seed_count == 1
    assert (void.reached_counts, void.unreached_counts, void.sum_steps, void.farthest) == (1, 0, 0, (0, (0, 0, 0)))
