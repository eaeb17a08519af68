"""section() on the device against the reference section of test_section_host.py: every instance evaluated by the oracle at
every sample, then the map rules.  Every comparison is exact: numpy.array_equal for every map, field for field for the
accumulators; no case is excluded."""
import numpy
import pytest

import codecad_amd as cc
from codecad_amd import rendering
from codecad_amd.section import Plane
from codecad_amd.rendering import assembly_section, assembly_picture

from test_section_host import scenario, device_accumulators, boxes_and_ball, RANDOM

pytestmark = pytest.mark.gpu


def check(cut, ref, distance):
    assert cut.dims == tuple(int(d) for d in ref.dims) and cut.step == ref.step
    assert cut.corner.tobytes() == ref.corner.tobytes()
    assert cut.part_ids.dtype == numpy.int32 and cut.inside_count.dtype == numpy.uint8
    assert numpy.array_equal(cut.part_ids, ref.part_ids)
    assert numpy.array_equal(cut.inside_count, ref.inside_count)
    if distance:
        assert cut.distance.dtype == numpy.float32 and cut.nearest.dtype == numpy.int32
        assert numpy.array_equal(cut.distance, ref.distance)
        assert numpy.array_equal(cut.nearest, ref.nearest)
    else:
        assert cut.distance is None and cut.nearest is None
    assert device_accumulators(cut) == ref.acc
    assert [c.i for c in cut.parts] == sorted(k for k, j in ref.acc if k == j) and all(c.i == c.j for c in cut.parts)
    assert [(c.i, c.j) for c in cut.overlaps] == sorted(k for k in ref.acc if k[0] != k[1])
    assert [i.instance.transform for i in cut.instances] == [i.transform for i in ref.instances]


def run(name, **kwargs):
    asm, plane, resolution, ref = scenario(name)
    cut = cc.section(asm, plane, resolution, **kwargs)
    check(cut, ref, kwargs.get("distance", False))
    return cut, ref


def all_ways(name):
    """cull and distance, both ways -> the culled cut without distance"""
    run(name, cull=False, distance=True)
    run(name, cull=False)
    run(name, distance=True)
    return run(name)


def test_two_boxes_closed_form(hip):
    cut, ref = all_ways("two_boxes")
    assert [(c.i, c.count) for c in cut.parts] == [(0, 32 * 32), (1, 32 * 16)]
    assert [(c.i, c.j, c.count) for c in cut.overlaps] == [(0, 1, 8 * 16)]
    assert (cut.part_ids[cut.inside_count == 2] == 0).all()          # the lower index owns the overlap
    o = cut.overlaps[0]
    assert o.area == pytest.approx(0.5 * 1.0) and tuple(o.centroid) == pytest.approx((0.75, 0.25, 0.03125), abs=1e-9)
    assert o.index_box == ((24, 12), (31, 27)) and o.bounding_box == ((0.53125, -0.21875), (0.96875, 0.71875))
    assert tuple(cut.position(24, 12)) == (0.53125, -0.21875, 0.03125)
    assert cut.part_at(0, 0).name == "a" and cut.part_at(55, 0) is None and cut.part_at(55, 20).name == "b"
    assert cut.runs == 1 and cut.evaluations > 0


def test_shaft_in_bore(hip):
    tight, ref = all_ways("shaft_tight")
    assert len(tight.overlaps) == 1 and (tight.inside_count == 2).sum() == tight.overlaps[0].count > 0
    clear, _ = all_ways("shaft_clear")
    assert clear.overlaps == [] and clear.inside_count.max() == 1


@pytest.mark.parametrize("name", ["gears_mid", "gears_oblique"])
def test_gear_train(hip, name):
    cut, ref = all_ways(name)
    assert len(cut.instances) == 8 and cut.overlaps
    samples = cut.dims[0] * cut.dims[1] * len(cut.instances)
    assert cut.evaluations < samples                                 # the tiles did cull


@pytest.mark.parametrize("kind", ["named", "oblique", "missing"])
@pytest.mark.parametrize("seed,k,blended", RANDOM)
def test_random_assemblies(hip, seed, k, blended, kind):
    cut, ref = all_ways("random_%d_%s" % (seed, kind))
    assert len(cut.instances) == k
    if kind == "missing":
        assert cut.runs == 0 and cut.parts == []                     # nothing is a candidate: nothing is launched


def test_64_instances_use_both_words_of_the_mask(hip):
    cut, ref = all_ways("grid_64")
    assert len(cut.instances) == 64 and max(c.i for c in cut.parts) >= 32 > min(c.i for c in cut.parts)
    assert cut.evaluations < cut.dims[0] * cut.dims[1] * 64 * 0.25


@pytest.mark.parametrize("name", ["one_sample", "nine_by_65"])
def test_dims_that_are_no_multiple_of_a_tile(hip, name):
    cut, ref = all_ways(name)
    assert cut.dims == {"one_sample": (1, 1), "nine_by_65": (9, 65)}[name]
    assert cut.parts[0].count == cut.dims[0] * cut.dims[1]


def test_overflowing_lists_are_regrown(hip):
    first = run("gears_mid")[0]
    small = run("gears_mid", initial_capacity=1)[0]
    assert first.runs == 1 and small.runs > 1
    assert small.parts == first.parts and small.overlaps == first.overlaps and small.evaluations == first.evaluations
    with_distance = run("gears_oblique", initial_capacity=1, distance=True)[0]
    assert with_distance.runs > 1


def test_coincident_instances_go_to_the_lower_index(hip):
    cut, ref = all_ways("coincident")
    full = run("coincident", distance=True)[0]
    assert set(full.nearest.ravel().tolist()) == {0, 2} and set(cut.part_ids.ravel().tolist()) == {-1, 0, 2}
    assert cut.parts[0].count == cut.parts[1].count == cut.overlaps[0].count


def test_sections_add_up_to_interference(hip):
    asm = boxes_and_ball()
    resolution = 0.125
    r = cc.interference(asm, resolution)
    assert 1 < r.dims[2] <= 48 and len(r.pairs) == 3
    counts, sums = {}, {}
    for k in range(int(r.dims[2])):
        cut = cc.section(asm, Plane.xy(float(r.corner[2] + r.step * numpy.float32(k))), resolution)
        assert cut.corner.tobytes() == numpy.array([r.corner[0], r.corner[1], r.corner[2] + r.step * numpy.float32(k)], numpy.float32).tobytes()
        assert cut.dims == (int(r.dims[0]), int(r.dims[1])) and cut.step == r.step
        for o in cut.overlaps:
            key = (o.i, o.j)
            counts[key] = counts.get(key, 0) + o.count
            sums[key] = tuple(a + b for a, b in zip(sums.get(key, (0, 0, 0)), o.index_sums + (k * o.count,)))
    assert counts == {(p.i, p.j): p.count for p in r.pairs}
    assert sums == {(p.i, p.j): p.index_sums for p in r.pairs}


def test_far_from_the_origin(hip):
    all_ways("far")


def test_the_picture_is_the_colouring_of_the_maps(hip):
    asm, plane, resolution, ref = scenario("gears_mid")
    pixels, cut = rendering.render_assembly_section_pixels(asm, plane, resolution)
    check(cut, ref, False)
    hues = assembly_picture.part_colors(ref.instances, "parts")
    assert pixels.shape == (ref.dims[1], ref.dims[0], 3) and pixels.dtype == numpy.uint8
    assert numpy.array_equal(pixels, assembly_section.section_colors(ref.part_ids, ref.inside_count, hues))
    assert (pixels == numpy.array([255, 0, 0], numpy.uint8)).all(axis=-1).sum() > 0       # the pins in the planets, marked
    plain, _ = rendering.render_assembly_section_pixels(asm, plane, resolution, colors=None, overlap_color=(0, 0, 1), background=(0, 0, 0),
                                                        outline=False)
    hues = assembly_picture.part_colors(ref.instances, None)
    assert numpy.array_equal(plain, assembly_section.section_colors(ref.part_ids, ref.inside_count, hues, (0, 0, 1), (0, 0, 0), False))

