"""thin_walls() on the device against the offset-by-offset reference of thin_walls_scenes.py: the part ids, depth_sq, thin_ids,
the counts per part and every field of every region are EQUAL to the reference, with the LDS staging and without it,
whatever the region table's first capacity and the voxel traversal's top level were."""
import numpy
import pytest

import codecad_amd as cc
from codecad_amd import _instance_cells

import thin_walls_scenes as scenes
from thin_walls_scenes import NAMES, BY_NAME, reference, scene, NONE, EMPTY

pytestmark = pytest.mark.gpu


def run(name, **kwargs):
    c = BY_NAME[name]
    asm, resolution, instances, corner, step, dims = scene(c.scene)
    report = cc.thin_walls(asm, resolution, of=c.of, radius_sq=c.r2, cover_sq=c.c2, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert report.of == c.of and (report.radius_sq, report.cover_sq) == (c.r2, c.c2) and len(report.instances) == len(instances)
    return report


def check_against_reference(report, ref):
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    assert report.depth_sq.dtype == numpy.uint16 and report.depth_sq.flags.c_contiguous
    assert numpy.array_equal(report.depth_sq, ref.depth_sq)
    assert report.thin_ids.dtype == numpy.uint8 and report.thin_ids.flags.c_contiguous
    assert numpy.array_equal(report.thin_ids, ref.thin_ids)
    assert report.counts == [int((ref.ids == k).sum()) for k in range(len(report.instances))]
    assert report.core_counts == ref.core_counts and report.thin_counts == ref.thin_counts
    assert all(type(v) is int for v in report.counts + report.core_counts + report.thin_counts)
    assert report.labels.dtype == numpy.uint32 and numpy.array_equal(report.labels, ref.labels)
    got = [(r.label, r.count, r.box, r.index_sums, r.touches_border, r.parts) for r in report.regions]
    assert got == [tuple(r) for r in ref.regions]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for r in report.regions:
        assert r.volume == r.count * step ** 3
        assert tuple(r.centroid) == tuple(corner[k] + step * r.index_sums[k] / r.count for k in range(3))
        assert report.mask(r).sum() == r.count and (report.thin_ids[report.mask(r)] != EMPTY).all()
    assert ((report.labels == NONE) == (report.thin_ids == EMPTY)).all()


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name, lds):
    report = run(name, lds=lds)
    ref = reference(name)
    print(name, "lds" if lds else "global", "thin", report.thin_counts, "reference", ref.thin_counts, "core", report.core_counts,
          "reference", ref.core_counts, "regions", len(report.regions), "reference", len(ref.regions))
    check_against_reference(report, ref)
    assert report.traversals == 1 and report.component_capacity_runs == 1


def test_min_thickness_gives_the_default_radii(hip):
    asm, resolution = scene("rib")[:2]
    report = cc.thin_walls(asm, resolution, 0.25)                    # 0.25 / (2 / 16) = 2 steps: R2 = 4, C2 = 12, the case `rib`
    assert (report.radius_sq, report.cover_sq) == (4, 12)
    check_against_reference(report, reference("rib"))


@pytest.mark.parametrize("lds", [True, False])
def test_the_region_table_regrows_and_only_the_statistics_run_again(hip, lds):
    ref = reference("bars_r2_c2")
    assert len(ref.regions) == 9
    small = run("bars_r2_c2", lds=lds, initial_components=1)
    check_against_reference(small, ref)
    assert small.component_capacity_runs == 2 and small.traversals == 1


def test_a_traversal_of_several_levels_changes_nothing(hip, monkeypatch):
    dims = scene("shell")[5]
    monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.comp.mass.forced_top_cells(dims, 64))
    assert _instance_cells.top_side(dims) == 64                      # one top cell: levels of 64, 16 and 4 samples
    report = run("shell")
    monkeypatch.undo()
    assert _instance_cells.top_side(dims) == 16
    check_against_reference(report, reference("shell"))
    small = run("rib", initial_capacity=8)                           # ... and a cell list that overflows repeats the traversal
    assert small.traversals > 1
    check_against_reference(small, reference("rib"))
