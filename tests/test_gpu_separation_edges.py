"""separation() on the device at the edges of its branch and bound, against the CPU references of separation_scenes.py through
the `check` of test_gpu_separation.py -- float32 bits, witnesses, evaluations and the rows of every level, no tolerance:
forced top sides up to 65536 (seven levels, every key array of the layout), 65536 samples on each axis in turn (indices
above 32767 in rows and witnesses), a pair whose v(q) - U_l equals r and one four ulps above it, both zeros tied for the
least key, assemblies far from the origin, and parts whose field is a NaN at some samples or at all of them.
test_separation_edges_host.py proves that every scenario holds its edge."""
import numpy
import pytest

import codecad_amd as cc
import separation_scenes as scenes
from test_gpu_separation import check, sep

pytestmark = pytest.mark.gpu


def run(name):
    asm, resolution, instances, corner, step, dims = scenes.edge_scene(name)
    side = scenes.EDGES[name].side
    report = cc.separation(asm, resolution) if side is None else sep._separation(asm, resolution, side=side)
    assert report.traversals == 1 and numpy.array_equal(report.dims, dims)
    check(report, *scenes.edge_reference(name))
    return report


@pytest.mark.parametrize("side, levels", zip(scenes.DEEP_SIDES, (4, 5, 7)))
@pytest.mark.parametrize("name", ("spheres", "rims"))
def test_forced_deep_sides(hip, name, side, levels):
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    report = sep._separation(asm, resolution, side=side)
    check(report, scenes.dense_reference(name), scenes.traversal_reference(name, side))
    assert len(report.level_rows) == levels


@pytest.mark.parametrize("side", (32, 48, 100, 128, 262144))
def test_a_side_that_is_no_16_times_a_power_of_4_is_refused_cleanly(hip, side):
    asm, resolution, instances, corner, step, dims = scenes.scene("spheres")
    with pytest.raises(RuntimeError, match="top_side"):
        sep._separation(asm, resolution, side=side)
    check(cc.separation(asm, resolution), scenes.dense_reference("spheres"), scenes.traversal_reference("spheres"))


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_65536_samples_on_one_axis(hip, axis):
    report = run("long_" + "xyz"[axis])
    assert report.dims[axis] == 65536 and report.pairs[0].witness[axis] > 32767


def test_a_pair_at_r_is_kept_and_one_just_above_it_dropped(hip):
    kept, dropped = run("near_r_equal"), run("near_r_dropped")
    assert kept.level_rows == (36, 40) and dropped.level_rows == (36, 39)


def test_both_zeros_give_plus_zero_and_the_first_tied_sample(hip):
    report = run("touching")
    pair = report.pairs[0]
    assert numpy.float32(pair.separation).view(numpy.uint32) == 0 and pair.witness == (16, 0, 0)


@pytest.mark.parametrize("name", ("nans", "nans_64"))
def test_nans_take_no_part_and_keep_their_pairs(hip, name):
    """`speck` is a NaN on three planes and +inf elsewhere, `ghost` a NaN everywhere: pairs with numbers at only some samples,
    pairs with none (all four fields None) and an ordinary pair, from one level and from two."""
    report = run(name)
    by_pair = {(p.i, p.j): p for p in report.pairs}
    for pair in ((0, 2), (1, 2), (2, 3)):
        assert by_pair[pair][2:] == (None, None, None, None)
    for pair in ((0, 1), (1, 3)):
        assert by_pair[pair].separation == numpy.inf and by_pair[pair].witness == (0, 0, 0)
    assert 0 < by_pair[(0, 3)].separation < 0.25


@pytest.mark.parametrize("name", ("far_boxes", "far_random_2"))
def test_far_from_the_origin(hip, name):
    report = run(name)
    assert abs(float(report.corner[1])) > 1999
