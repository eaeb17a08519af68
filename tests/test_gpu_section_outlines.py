"""section_outlines() on the device against the reference outlines of test_section_outlines_host.py: every instance
evaluated by the oracle at every ringed sample, crossings in NumPy float32, the segments of a square derived from its
crossed edges.  Every comparison is exact: the sorted records byte for byte, the counts and the evaluations as integers."""
import xml.etree.ElementTree

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import rendering
from codecad_amd.section import Plane
from codecad_amd.section_outlines import SEGMENT, stitch

from test_section_outlines_host import scenario, traversal, check_raster_property, outlines_of

pytestmark = pytest.mark.gpu


def check(o, ref, evaluations=None):
    assert o.dims == tuple(int(d) for d in ref.dims) and o.step == ref.step and o.corner.tobytes() == ref.corner.tobytes()
    assert o.segments.dtype == SEGMENT and o.segments.tobytes() == ref.segments.tobytes()
    assert o.counts.tolist() == ref.counts.tolist() and len(o.loops) == len(ref.instances)
    assert [i.instance.transform for i in o.instances] == [i.transform for i in ref.instances]
    if evaluations is not None:
        assert o.evaluations == evaluations


def run(name, cull=True, **kwargs):
    asm, plane, resolution, ref = scenario(name)
    o = cc.section_outlines(asm, plane, resolution, cull=cull, **kwargs)
    check(o, ref, traversal(name, cull).evaluations)
    return o, ref


def test_two_boxes(hip):
    o, ref = run("two_boxes")
    assert o.runs == 1 and [len(l) for l in o.loops] == [1, 1] and all(l.closed and l.area > 0 for l in sum(o.loops, []))
    assert o.loops[0][0].area == pytest.approx(4.0 - 4 * 0.0625 ** 2 / 8) and o.loops[1][0].area == pytest.approx(2.0 - 4 * 0.0625 ** 2 / 8)
    want = outlines_of(ref, o.plane)
    assert all(numpy.array_equal(a.points, b.points) for a, b in zip(sum(o.loops, []), sum(want.loops, [])))
    assert o.points3d(o.loops[0][0])[:, 2].tolist() == [0.03125] * len(o.loops[0][0].points)


def test_boxes_and_ball_on_an_oblique_plane(hip):
    o, ref = run("boxes_and_ball")
    assert o.runs == 1 and all(len(l) == 1 and l[0].closed for l in o.loops)


def test_coincident_instances_give_identical_segments(hip):
    o, ref = run("coincident")
    a, b = o.segments[o.segments["k"] == 0].copy(), o.segments[o.segments["k"] == 1].copy()
    b["k"] = 0
    assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_both_saddles(hip):
    o, ref = run("diagonal")
    assert len(o.loops[0]) == 3 and all(l.closed and l.area > 0 for l in o.loops[0])


def test_a_tile_with_a_single_live_column(hip):
    o, ref = run("bar_64_9")
    assert o.dims == (64, 9) and o.segments["a"].max() == 64 and len(o.loops[0]) == 1 and o.loops[0][0].closed


def test_a_part_smaller_than_a_step(hip):
    o, ref = run("speck")
    assert o.dims == (1, 1) and len(o.segments) == 4 and len(o.loops[0][0].points) == 4


def test_64_instances_without_the_hidden_ones(hip):
    o, ref = run("grid_64")
    assert len(o.instances) == 64 and (o.counts > 0).sum() > 30
    assert o.segments["k"].min() < 32 <= o.segments["k"].max()      # both words of the mask; bit 63 is evaluated (the evaluations)


def test_far_from_the_origin(hip):
    run("far")


def test_a_plane_that_misses_every_part(hip):
    o, ref = run("missing")
    assert o.runs == 0 and len(o.segments) == 0 and o.loops == [[], []]


def test_overflowing_lists_and_segment_buffers_are_regrown(hip):
    first = run("boxes_and_ball")[0]
    small = run("boxes_and_ball", initial_capacity=1)[0]
    few = run("boxes_and_ball", segment_capacity=1)[0]
    both = run("boxes_and_ball", initial_capacity=1, segment_capacity=1)[0]
    assert first.runs == 1 and small.runs > 1 and few.runs == 2 and both.runs > small.runs


@pytest.mark.parametrize("name", ["boxes_and_ball", "grid_64"])
def test_dense_gives_what_culled_gives(hip, name):
    dense, culled = run(name, cull=False)[0], run(name)[0]
    assert dense.segments.tobytes() == culled.segments.tobytes() and dense.evaluations > culled.evaluations and dense.runs == 1


def test_a_random_assembly(hip):
    o, ref = run("random_2_named")
    assert len(o.instances) == 9


def test_the_fill_of_the_device_loops_is_the_inside_map(hip):
    o, ref = run("gear_train")
    assert max(o.dims) <= 96 and len(o.instances) == 8
    loops = check_raster_property(o.segments, ref.w, float(o.step))
    for a, b in zip(sum(loops, []), sum(o.loops, [])):
        assert numpy.array_equal(b.points, ref.first + float(ref.step) * a.points) and a.closed and b.closed
    cut = [bool((w < 0).any()) for w in ref.w]                 # (the plane goes through the sun, one planet with its pin, the carrier)
    assert [len(l) >= 1 for l in o.loops] == cut and sum(cut) >= 4         # every part the plane cuts is a closed outline


def test_the_svg_of_a_cut(hip, tmp_path):
    asm, plane, resolution, ref = scenario("gear_train")
    o = rendering.render_assembly_section_svg(asm, str(tmp_path / "cut.svg"), plane, resolution)
    check(o, ref)
    root = xml.etree.ElementTree.parse(str(tmp_path / "cut.svg")).getroot()
    paths = [e for e in root if e.tag.endswith("path")]
    assert len(paths) == sum(1 for l in o.loops if l) >= 4 and all(p.get("fill-rule") == "evenodd" for p in paths)
    assert [p.get("d").count("Z") for p in paths] == [len(l) for l in o.loops if l]
    assert root.get("viewBox") and root.get("width").endswith("mm")
