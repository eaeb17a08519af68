"""tool_access() on the device against reference 1 of tool_access_scenes.py, which is written from the definitions: the part
ids, the tops, the tips, the cut, the crowd, rest_ids, both count vectors, the labels and every field of every pocket are EQUAL
to the reference, in every direction a scenario is registered for, whatever the pocket table's first capacity and the voxel
traversal's cell lists were."""
import numpy
import pytest

import codecad_amd as cc

import tool_access_scenes as scenes
from tool_access_scenes import NAMES, BY_NAME, reference, scene, NONE, EMPTY

pytestmark = pytest.mark.gpu


def run(name, **kwargs):
    c = BY_NAME[name]
    asm, resolution, instances, corner, step, dims = scene(c.scene)
    report = cc.tool_access(asm, resolution, axis=c.axis, up=c.up, tool=c.tool, of=c.of, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert (report.of, report.axis, report.up, report.tool) == (c.of, c.axis, c.up, c.tool)
    assert len(report.instances) == len(instances)
    return report


def check_against_reference(report, ref):
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    for name, got, want in (("tops", report.tops, ref.tops), ("tips", report.tips, ref.tips), ("cut", report.cut, ref.cut)):
        assert got.dtype == numpy.int32 and got.shape == want.shape and numpy.array_equal(got, want), name
    assert report.crowd.dtype == numpy.uint8 and numpy.array_equal(report.crowd, ref.crowd)
    assert report.rest_ids.dtype == numpy.uint8 and report.rest_ids.flags.c_contiguous and numpy.array_equal(report.rest_ids, ref.rest_ids)
    assert report.counts == [int((ref.ids == k).sum()) for k in range(len(report.instances))]
    assert report.undercut_counts == ref.undercut_counts and report.tight_counts == ref.tight_counts
    assert all(type(v) is int for v in report.counts + report.undercut_counts + report.tight_counts)
    assert numpy.array_equal(report.undercut_mask(), ref.undercut) and numpy.array_equal(report.tight_mask(), ref.tight)
    assert report.labels.dtype == numpy.uint32 and report.labels.flags.c_contiguous and numpy.array_equal(report.labels, ref.labels)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in report.pockets]
    assert got == [tuple(r) for r in ref.pockets]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for r in report.pockets:
        assert r.volume == r.count * step ** 3
        assert tuple(r.centroid) == tuple(corner[k] + step * r.index_sums[k] / r.count for k in range(3))
        assert report.mask(r).sum() == r.count and (report.rest_ids[report.mask(r)] != EMPTY).all()
    assert ((report.labels == NONE) == (report.rest_ids == EMPTY)).all()
    rest = sum(ref.undercut_counts) + sum(ref.tight_counts)
    assert report.rest_volume() == rest * step ** 3 and report.machinable == (rest == 0)


@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name):
    report = run(name)
    ref = reference(name)
    print(name, "undercut", report.undercut_counts, "reference", ref.undercut_counts, "tight", report.tight_counts, "reference",
          ref.tight_counts, "pockets", len(report.pockets), "reference", len(ref.pockets), "highest cut", int(report.cut.max()),
          "reference", int(ref.cut.max()))
    check_against_reference(report, ref)
    assert report.traversals == 1 and report.component_capacity_runs == 1


def test_the_pocket_table_regrows_and_only_the_statistics_run_again(hip):
    ref = reference("pocket_z+_flat4")
    assert len(ref.pockets) == 4
    small = run("pocket_z+_flat4", initial_components=1)                           # a pocket table of one row
    check_against_reference(small, ref)
    assert small.component_capacity_runs == 2 and small.traversals == 1


def test_an_overflowing_cell_list_changes_nothing(hip):
    small = run("two_x-_flat4", initial_capacity=8)                                  # a cell list that overflows repeats the traversal
    assert small.traversals > 1
    check_against_reference(small, reference("two_x-_flat4"))


def test_one_part_alone_on_the_two_part_scene(hip):
    for name in ("two_z+_flat4_of0", "two_z+_flat4_of1"):
        report = run(name)
        check_against_reference(report, reference(name))
        other = 1 - BY_NAME[name].of
        assert report.undercut_counts[other] == report.tight_counts[other] == 0
        assert not numpy.array_equal(report.rest_ids, reference("two_z+_flat4").rest_ids)


def test_a_second_call_gives_the_same_bytes(hip):
    first, second = run("two_y-_flat4"), run("two_y-_flat4")
    for a, b in zip(first, second):
        if isinstance(a, numpy.ndarray):
            assert a.tobytes() == b.tobytes()
    assert (first.undercut_counts, first.tight_counts) == (second.undercut_counts, second.tight_counts)
    assert [tuple(p) for p in first.pockets] == [tuple(p) for p in second.pockets]
