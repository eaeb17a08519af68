"""wall_thickness() on the device against reference 1 of wall_thickness_scenes.py, written from the definition offset by
offset: the part ids, depth_sq, thickness_sq, the counts, the least thickness of every part and where it is are EQUAL to the
reference, entry for entry, for of=SOLID and of=k, with the LDS staging and without it, and on a second call."""
import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes

import wall_thickness_scenes as scenes
from wall_thickness_scenes import NAMES, BY_NAME, reference, scene, SOLID

pytestmark = pytest.mark.gpu


def run(name, **kwargs):
    c = BY_NAME[name]
    asm, resolution, instances, corner, step, dims = scene(c.scene)
    report = cc.wall_thickness(asm, resolution, of=c.of, radius_sq=c.r2, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert report.of == c.of and report.radius_sq == c.r2 and report.cap == c.r2 + 1 and len(report.instances) == len(instances)
    return report


def check_against_reference(report, ref):
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    for got, want in ((report.depth_sq, ref.depth_sq), (report.thickness_sq, ref.thickness_sq)):
        assert got.dtype == numpy.uint16 and got.flags.c_contiguous and got.shape == want.shape
        wrong = numpy.argwhere(got != want)
        assert len(wrong) == 0, [(tuple(k), int(got[tuple(k)]), int(want[tuple(k)])) for k in wrong[:8]]
    assert report.counts == ref.counts and report.core_counts == ref.core_counts and report.capped_counts == ref.capped_counts
    assert report.min_sq == ref.min_sq and report.thinnest == ref.thinnest
    assert all(type(v) is int for v in report.counts + report.core_counts + report.capped_counts)
    assert all(v is None or type(v) is int for v in report.min_sq)


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name, lds):
    ref = reference(name)
    report = run(name, lds=lds)
    print(name, "lds" if lds else "global", "min", report.min_sq, "reference", ref.min_sq, "at", report.thinnest, "reference", ref.thinnest,
          "capped", report.capped_counts, "reference", ref.capped_counts, "core", report.core_counts, "reference", ref.core_counts)
    check_against_reference(report, ref)
    assert report.traversals == 1
    again = run(name, lds=lds)                                       # a second call: nothing is left over from the first
    check_against_reference(again, ref)
    assert again.thickness_sq.tobytes() == report.thickness_sq.tobytes()


def test_max_thickness_gives_the_radius_and_the_methods_follow_the_map(hip):
    asm, resolution = scene("rib")[:2]
    report = cc.wall_thickness(asm, resolution, 0.25)                # 0.25 / (2 / 16) = 2 steps: R2 = 4, the case `rib`
    assert report.radius_sq == 4
    ref = reference("rib")
    check_against_reference(report, ref)
    assert numpy.array_equal(report.below(4), (ref.thickness_sq > 0) & (ref.thickness_sq <= 4)) and report.thinnest_part() == 0
    widths = report.diameters()
    assert numpy.isinf(widths[ref.thickness_sq == 5]).all() and (widths[ref.thickness_sq == 1] == 2 * float(report.step)).all()


def test_an_assembly_with_nothing_visible_launches_nothing(hip):
    ghost = shapes.box(1).make_part("ghost").hidden()
    report = cc.wall_thickness(cc.assembly("nothing", [ghost]), 0.1, 0.3)
    assert report.traversals == 0 and report.counts == [] == report.min_sq == report.thinnest == report.capped_counts
    assert not report.thickness_sq.any() and not report.depth_sq.any() and report.thinnest_part() is None


def test_of_decides_who_is_thin(hip):
    solid, plate = run("glued_solid"), run("glued_plate")
    assert solid.min_sq[0] > 1 and plate.min_sq == [1, None] and plate.thinnest == [(0, 0, 0), None]     # 2 samples wide: D = 1
    assert SOLID == solid.of and plate.of == 0 and solid.min_sq == reference("glued_solid").min_sq
