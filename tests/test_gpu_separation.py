"""separation() on the device against the CPU reference of separation_scenes.py: the float32 bits of every pair's
separation and its witness against the dense definition, the evaluations and the rows of every level against the
reference traversal -- on every scenario, under forced top sides, through overflow and regrowth, on a lattice far too
fine to evaluate densely, and against interference() for the sign."""
import math
import sys

import numpy
import pytest

import codecad_amd as cc
import separation_scenes as scenes

sep = sys.modules["codecad_amd.separation"]            # (the package's attribute of that name is the function)

pytestmark = pytest.mark.gpu


def check(report, dense, traversal):
    keys, witness = scenes.report_keys(report)
    n = len(report.instances)
    assert [(p.i, p.j) for p in report.pairs] == [(i, j) for i in range(n) for j in range(i + 1, n)]      # every pair
    if dense is not None:
        assert numpy.array_equal(keys, dense.keys) and witness == dense.witness
    assert numpy.array_equal(keys, traversal.keys) and witness == traversal.witness
    assert report.samples_evaluated == traversal.evaluations
    assert report.level_rows == traversal.level_rows
    for p in report.pairs:
        if p.separation is not None:
            assert p.witness_point == cc._instance_cells.index_position(report.corner, report.step, p.witness)
            assert p.gap_bounds == (2.0 * float(p.separation) - float(report.step) * math.sqrt(3), 2.0 * float(p.separation))


@pytest.mark.parametrize("name", scenes.NAMES)
def test_every_scenario_matches_the_reference(hip, name):
    """solids64 among them: 64 instances, 2016 pairs, the whole [instance][lane] block of LDS, at whatever workgroup
    shape the launch picks for it."""
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    report = cc.separation(asm, resolution)
    assert report.traversals == 1 and numpy.array_equal(report.dims, dims)
    check(report, scenes.dense_reference(name), scenes.traversal_reference(name))


@pytest.mark.parametrize("side", (16, 64, 256))
@pytest.mark.parametrize("name", scenes.FORCED)
def test_forced_top_sides(hip, name, side):
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    report = sep._separation(asm, resolution, side=side)
    check(report, scenes.dense_reference(name), scenes.traversal_reference(name, side))
    assert len(report.level_rows) == {16: 1, 64: 2, 256: 3}[side]


@pytest.mark.parametrize("name", ("gears", "random_2"))
def test_overflow_and_regrowth_give_the_same_report(hip, name):
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    first = cc.separation(asm, resolution)
    again = cc.separation(asm, resolution, initial_capacity=1)
    assert again.traversals > 1 and first.traversals == 1
    assert again.pairs == first.pairs and again.samples_evaluated == first.samples_evaluated and again.level_rows == first.level_rows
    check(again, scenes.dense_reference(name), scenes.traversal_reference(name))


def test_the_fine_two_sphere_lattice(hip):
    """About 4000 x 1861 x 1861 samples, 1.4e10: the device against the reference traversal and the closed-form gap."""
    asm, resolution, dims, traversal = scenes.fine_spheres()
    report = cc.separation(asm, resolution)
    assert numpy.array_equal(report.dims, dims) and dims.max() >= 4000
    check(report, None, traversal)
    lo, hi = report.pairs[0].gap_bounds
    assert lo - 1e-5 <= scenes.SPHERES_GAP <= hi + 1e-5
    assert report.samples_evaluated <= 1e-3 * float(numpy.prod(dims)) * 2


@pytest.mark.parametrize("name", ("lens", "gears", "random_5", "solids64"))
def test_negative_exactly_for_the_pairs_interference_reports(hip, name):
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    report = cc.separation(asm, resolution)
    overlapping = {(p.i, p.j) for p in cc.interference(asm, resolution).pairs}
    assert {(p.i, p.j) for p in report.pairs if p.separation is not None and p.separation < 0} == overlapping
    if name != "random_5":
        assert overlapping
