"""overhangs() on the device against the reference of overhangs_scenes.py, which is written from the definitions: the part ids,
overhang_ids, support_ids, landing_ids, every count, the plate landings, the first layer, the labels and every field of every
support structure are EQUAL to the reference, in every direction a scenario is registered for, whatever the support table's
first capacity and the voxel traversal's top level were."""
import numpy
import pytest

import codecad_amd as cc
from codecad_amd import _instance_cells

import overhangs_scenes as scenes
from overhangs_scenes import NAMES, BY_NAME, reference, scene, NONE, EMPTY

pytestmark = pytest.mark.gpu


def run(name, **kwargs):
    c = BY_NAME[name]
    asm, resolution, instances, corner, step, dims = scene(c.scene)
    report = cc.overhangs(asm, resolution, axis=c.axis, up=c.up, reach_sq=c.reach_sq, of=c.of, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert (report.of, report.axis, report.up, report.reach_sq) == (c.of, c.axis, c.up, c.reach_sq)
    assert len(report.instances) == len(instances)
    return report


def check_against_reference(report, ref):
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    for got, want in ((report.overhang_ids, ref.overhang_ids), (report.support_ids, ref.support_ids), (report.landing_ids, ref.landing_ids)):
        assert got.dtype == numpy.uint8 and got.flags.c_contiguous and numpy.array_equal(got, want)
    assert report.first_layer == ref.first_layer and type(report.first_layer) is int
    assert report.counts == [int((ref.ids == k).sum()) for k in range(len(report.instances))]
    assert report.overhang_counts == ref.overhang_counts and report.support_counts == ref.support_counts
    assert report.landing_counts == ref.landing_counts and report.plate_landings == ref.plate_landings
    assert all(type(v) is int for v in report.counts + report.overhang_counts + report.support_counts + report.landing_counts
               + [report.plate_landings])
    assert sum(report.overhang_counts) == sum(report.landing_counts) + report.plate_landings
    assert report.labels.dtype == numpy.uint32 and report.labels.flags.c_contiguous and numpy.array_equal(report.labels, ref.labels)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in report.supports]
    assert got == [tuple(r) for r in ref.supports]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for r in report.supports:
        assert r.volume == r.count * step ** 3
        assert tuple(r.centroid) == tuple(corner[k] + step * r.index_sums[k] / r.count for k in range(3))
        assert report.mask(r).sum() == r.count and (report.support_ids[report.mask(r)] != EMPTY).all()
    assert ((report.labels == NONE) == (report.support_ids == EMPTY)).all()
    assert report.support_volume() == sum(ref.support_counts) * step ** 3 and report.overhang_area() == sum(ref.overhang_counts) * step ** 2
    assert report.self_supporting == (sum(ref.overhang_counts) == 0)


@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name):
    report = run(name)
    ref = reference(name)
    print(name, "first layer", report.first_layer, "reference", ref.first_layer, "overhangs", report.overhang_counts, "reference",
          ref.overhang_counts, "supports", report.support_counts, "reference", ref.support_counts, "landings", report.landing_counts,
          "reference", ref.landing_counts, "plate", report.plate_landings, "reference", ref.plate_landings, "structures",
          len(report.supports), "reference", len(ref.supports))
    check_against_reference(report, ref)
    assert report.traversals == 1 and report.component_capacity_runs == 1


def test_the_support_table_regrows_and_only_the_statistics_run_again(hip):
    ref = reference("ball_z+_r1")
    assert len(ref.supports) == 19
    small = run("ball_z+_r1", initial_components=1)
    check_against_reference(small, ref)
    assert small.component_capacity_runs == 2 and small.traversals == 1


def test_a_traversal_of_several_levels_changes_nothing(hip, monkeypatch):
    dims = scene("words")[5]
    normal = _instance_cells.top_side(dims)
    monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.comp.mass.forced_top_cells(dims, 64))
    assert _instance_cells.top_side(dims) == 64 != normal           # three top cells: levels of 64, 16 and 4 samples
    report = run("words_z+_r1")
    monkeypatch.undo()
    assert _instance_cells.top_side(dims) == normal == 16
    check_against_reference(report, reference("words_z+_r1"))


def test_an_overflowing_cell_list_changes_nothing(hip):
    small = run("six_x-_r1", initial_capacity=8)                     # a cell list that overflows repeats the traversal
    assert small.traversals > 1
    check_against_reference(small, reference("six_x-_r1"))


def test_one_part_alone_on_the_two_part_scene(hip):
    for name in ("six_z+_r1_of1", "six_x-_r1_of0"):
        report = run(name)
        ref = reference(name)
        check_against_reference(report, ref)
        other = 1 - BY_NAME[name].of
        assert report.overhang_counts[other] == report.support_counts[other] == report.landing_counts[other] == 0
        assert not numpy.array_equal(report.support_ids, reference(name.rsplit("_of", 1)[0]).support_ids)
