"""The edge scenarios of separation_scenes.py, inspected without a device: each one holds the edge test_gpu_separation_edges.py
runs it for -- seven levels of key arrays, indices above 32767 in the rows and the witness of every axis, a pair whose
v(q) - U_l equals r (and one four ulps above it), -0.0 and +0.0 tied for the least key, coordinates where a binary32 ulp is
a visible part of the step, NaNs in the fields and pairs the NaN rule keeps, both kernel variants -- and the reference
traversal still gives the dense minimum and witness wherever the lattice can be evaluated densely.  A scenario that loses its edge fails here."""
import sys

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import _instance_cells

import heavy_instances as hi
import separation_scenes as scenes

sep = sys.modules["codecad_amd.separation"]


def same(dense, traversal):
    return numpy.array_equal(dense.keys, traversal.keys) and dense.witness == traversal.witness


def same_traversal(a, b):
    return same(a, b) and a[2:] == b[2:]                   # evaluations, level_rows, side


# ---- depth ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("spheres", "rims"))
def test_forced_deep_sides_use_every_key_array(name):
    dense = scenes.dense_reference(name)
    for side, levels in zip(scenes.DEEP_SIDES, (4, 5, 7)):
        traversal = scenes.traversal_reference(name, side)
        assert traversal.side == side and len(traversal.level_rows) == levels == len(_instance_cells.levels(side, 1, None)[0])
        assert same(dense, traversal) and all(rows > 0 for rows in traversal.level_rows)
        assert traversal.level_rows[-1] == scenes.traversal_reference(name, 256).level_rows[-1]       # the same finest cells
    assert len(sep.top_rows(2, scenes.scene(name)[5], 65536)) == 1
    # seven levels read U_0 .. U_6 and write U_1 .. U_7, the leaf the final array U_8: nine arrays, the most the layout takes
    assert scenes.DEEP_SIDES[-1] == 16 * 4 ** 6


# ---- indices --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a_long_axis_has_65536_samples_and_indices_above_32767_at_every_level(axis):
    """The reference evaluates 190,640 samples (2 x 1024 children of side 64, then what the bound keeps) of 2 x 7.6e7."""
    name = "long_" + "xyz"[axis]
    asm, resolution, instances, corner, step, dims = scenes.edge_scene(name)
    assert dims[axis] == 65536 and all(16 < dims[k] < 64 for k in range(3) if k != axis)
    listed = []
    traversal = scenes.traverse(scenes.edge_values(name), 2, dims, step, listed=listed)
    assert same_traversal(traversal, scenes.edge_reference(name)[1])
    assert traversal.side == 256 and len(traversal.level_rows) == 3 and traversal.evaluations <= 200000
    assert [len(rows) for rows in listed] == list(traversal.level_rows)
    assert all((rows[:, axis] > 32767).any() for rows in listed)                    # in the rows every level lists
    assert (sep.top_rows(2, dims, 256)[:, 1 if axis == 2 else 0] >> (16 if axis == 1 else 0) & 0xffff).max() == 65536 - 256
    witness = traversal.witness[(0, 1)]
    assert witness[axis] > 32767 and all(witness[k] < 34 for k in range(3) if k != axis)
    # not tied across the middle: on the line through the witness along the long axis, 4096 samples to either side (the
    # middle of the lattice, 32767.5, among them), the witness alone has the least key, and the keys rise away from it
    values = scenes.edge_values(name)
    line = numpy.repeat(numpy.array([witness], dtype=numpy.int64), 8193, axis=0)
    line[:, axis] += numpy.arange(-4096, 4097)
    keys = scenes.order_keys(scenes.pair_value(values(0, line), values(1, line))).astype(numpy.int64)
    assert keys[4096] == traversal.keys[0, 1] and (numpy.delete(keys, 4096) > keys[4096]).all()
    assert (numpy.diff(keys[:4097]) < 0).all() and (numpy.diff(keys[4096:]) > 0).all()
    # the larger ball first: 2 * separation is the gap of the two balls to within a step's diagonal
    lo, hi_ = sep.gap_bounds(scenes.key_value(traversal.keys[0, 1]), step)
    assert lo <= scenes.LONG_DISTANCE - sum(scenes.LONG_RADII) <= hi_ + 1e-3      # (binary32 at 512: an ulp of 6e-5)


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_one_sample_more_on_the_long_axis_is_refused(axis):
    asm = scenes._long(axis, scenes.LONG_RESOLUTION)
    instances = _instance_cells.visible(asm, scenes.LONG_RESOLUTION)
    assert _instance_cells.lattice(instances, scenes.LONG_RESOLUTION)[2][axis] == 65537
    with pytest.raises(ValueError, match="65536"):
        cc.separation(asm, scenes.LONG_RESOLUTION)


# ---- the drop rule at r ---------------------------------------------------------------------------------------------------

def ulps_from_r(name, dropped=numpy.greater):
    """[(ulps of (v(q) - U_l) above r, level, child's first index)] of every live child of every level that knows a bound,
    measured on the float32 operands, and the Traversal."""
    asm, resolution, instances, corner, step, dims = scenes.edge_scene(name)
    seen = []

    def watch(level, i, j, first, at, v, bound, difference, r):
        if numpy.isnan(bound):
            return
        again = (v - bound).astype(numpy.float32)
        assert numpy.array_equal(again.view(numpy.uint32)[at], difference.view(numpy.uint32)[at])
        ulps = difference.view(numpy.int32).astype(numpy.int64) - int(r.view(numpy.int32))      # both positive: bits order as values
        for c, lane in numpy.argwhere(at & (difference > 0)):
            seen.append((int(ulps[c, lane]), level, tuple(int(x) for x in first[c, lane])))

    traversal = scenes.traverse(scenes.edge_values(name), len(instances), dims, step, scenes.NEAR_R_SIDE, dropped=dropped, watch=watch)
    return seen, traversal


def test_a_pair_exactly_at_r_is_kept_and_one_four_ulps_above_it_is_dropped():
    """The bisection reached equality: at NEAR_R_EQUAL the child at (36, 28, 16) of the second level has v(q) - U_1 == r,
    0 ulps, kept; at the binary32 number before it, 4 ulps above r (v(q) lies in [0.25, 0.5) and moves by two ulps of r,
    U_1 moves with it), dropped.  Both are conditions on the inputs, measured here from the operands."""
    for name in ("near_r_equal", "near_r_dropped"):
        assert scenes.EDGES[name].side == scenes.NEAR_R_SIDE and scenes.edge_scene(name)[5].tolist() == [61, 40, 40]
    assert numpy.float32(scenes.NEAR_R_EQUAL) == scenes.NEAR_R_EQUAL
    assert numpy.nextafter(numpy.float32(scenes.NEAR_R_EQUAL), numpy.float32(0)) == numpy.float32(scenes.NEAR_R_DROPPED) == scenes.NEAR_R_DROPPED
    equal, kept = ulps_from_r("near_r_equal")
    above, dropped = ulps_from_r("near_r_dropped")
    assert same_traversal(kept, scenes.edge_reference("near_r_equal")[1]) and same_traversal(dropped, scenes.edge_reference("near_r_dropped")[1])
    at = (1, (36, 28, 16))
    assert [u for u, *where in equal if tuple(where) == at] == [0]
    assert [u for u, *where in above if tuple(where) == at] == [4]
    assert min(u for u, *_ in above if u > 0) == 4 and max(u for u, *_ in equal if u <= 0) == 0
    # the child is listed in the one and not in the other: 40 and 39 rows of the finest level
    assert kept.level_rows == (36, 40) and dropped.level_rows == (36, 39)
    assert kept.evaluations == 13512 and dropped.evaluations == 13256
    for name, traversal in (("near_r_equal", kept), ("near_r_dropped", dropped)):
        assert same(scenes.edge_reference(name)[0], traversal)


def test_a_drop_rule_that_is_not_strict_lists_other_rows():
    strict = scenes.edge_reference("near_r_equal")[1]
    loose = ulps_from_r("near_r_equal", dropped=numpy.greater_equal)[1]
    assert loose.level_rows == (36, 39) != strict.level_rows and loose.evaluations != strict.evaluations
    # ... and only there: four ulps above r both rules drop
    assert same_traversal(ulps_from_r("near_r_dropped", dropped=numpy.greater_equal)[1], scenes.edge_reference("near_r_dropped")[1])


# ---- zeros ----------------------------------------------------------------------------------------------------------------

def test_both_zeros_tie_for_the_least_key_on_the_shared_plane():
    asm, resolution, instances, corner, step, dims = scenes.edge_scene("touching")
    assert float(corner[0]) == -1.0 and float(step) == 2.0 ** -4 and dims.tolist() == [33, 16, 16]
    w = scenes.edge_fields("touching")
    dense, traversal = scenes.edge_reference("touching")
    assert same(dense, traversal)
    v = scenes.pair_value(w[0], w[1])
    keys = scenes.order_keys(v)
    tied = keys == dense.keys[0, 1]
    assert dense.keys[0, 1] == 0x80000000 and tied.sum() == 256 and (numpy.argwhere(tied)[:, 0] == 16).all()      # the plane x = 0
    assert (v[tied] == 0).all() and numpy.signbit(v[tied]).sum() == 128 and (~numpy.signbit(v[tied])).sum() == 128
    assert dense.witness[(0, 1)] == (16, 0, 0) and numpy.signbit(v[16, 0, 0])      # the first of them is a -0.0
    assert not numpy.signbit(scenes.key_value(dense.keys[0, 1])) and not numpy.signbit(sep.key_to_float(int(dense.keys[0, 1])))


# ---- far from the origin --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, near", (("far_boxes", "boxes"), ("far_random_2", "random_2")))
def test_far_from_the_origin_an_ulp_is_a_visible_part_of_the_step(name, near):
    asm, resolution, instances, corner, step, dims = scenes.edge_scene(name)
    assert numpy.array_equal(dims, scenes.scene(near)[5]) and resolution == scenes.scene(near)[1]
    assert abs(float(corner[1])) > 1999
    assert numpy.spacing(numpy.float32(abs(corner[1]))) / step > 2.0 ** -11            # 1 / 410 of the boxes' step, 1 / 1166 of random_2's
    dense, traversal = scenes.edge_reference(name)
    assert same(dense, traversal) and len(dense.witness) == len(instances) * (len(instances) - 1) // 2
    assert any(not numpy.array_equal(a, b) for a, b in zip(scenes.edge_fields(name), scenes.fields(near)))     # the rounding is in the values


# ---- NaN ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("nans", "nans_64"))
def test_nans_take_no_part_and_keep_their_pairs(name):
    """visible() and checked_lattice() accept the assembly, which is all separation() asks.  `speck` (1) is a NaN on the
    planes through the origin and +inf elsewhere, `ghost` (2) a NaN everywhere."""
    asm, resolution, instances, corner, step, dims = scenes.edge_scene(name)
    assert [i.name for i in instances] == ["ball", "speck", "ghost", "bead"]
    assert corner.tolist() == [-0.875] * 3 and float(step) == 2.0 ** -4 and dims.tolist() == [52, 32, 32]
    assert numpy.float32(scenes.NAN_SCALES[0]) > 0 and numpy.float32(scenes.NAN_SCALES[1]) == 0
    w = scenes.edge_fields(name)
    nans = [numpy.isnan(f) for f in w]
    assert [int(m.sum()) for m in nans] == [0, 52 * 32 * 32 - 51 * 31 * 31, 52 * 32 * 32, 0]
    on_a_plane = numpy.zeros(tuple(dims), dtype=bool)
    on_a_plane[14], on_a_plane[:, 14], on_a_plane[:, :, 14] = True, True, True
    assert numpy.array_equal(nans[1], on_a_plane) and numpy.isposinf(w[1][~on_a_plane]).all()
    dense, traversal = scenes.edge_reference(name)
    assert same(dense, traversal)
    # numbers at only some samples: +inf, first at (0, 0, 0); at no sample: no key and no witness; an ordinary pair
    plus_inf = scenes.order_keys(numpy.float32(numpy.inf))
    assert dense.keys[0, 1] == dense.keys[1, 3] == plus_inf == 0xff800000 and dense.witness[(0, 1)] == dense.witness[(1, 3)] == (0, 0, 0)
    assert dense.keys[0, 2] == dense.keys[1, 2] == dense.keys[2, 3] == scenes.NOTHING
    assert set(dense.witness) == {(0, 1), (0, 3), (1, 3)}
    assert scenes.key_value(dense.keys[0, 3]) < 0.25 and dense.witness[(0, 3)][0] > 14
    # in the traversal: v(q) is a NaN in live children; the bound is a NaN (nothing known, or no number at any q), +inf
    # (inf - inf is a NaN again) or a number -- and each of them keeps its pair
    seen = {}

    def watch(level, i, j, first, at, v, bound, difference, r):
        kept_by_nan = at & numpy.isnan(difference)
        seen[(level, i, j)] = (int((at & numpy.isnan(v)).sum()), float(bound), int(kept_by_nan.sum()), int((at & (difference > r)).sum()))

    again = scenes.traverse(scenes.edge_values(name), 4, dims, step, scenes.EDGES[name].side, watch=watch)
    assert same_traversal(again, traversal)
    last = len(traversal.level_rows) - 1
    assert len(traversal.level_rows) == (2 if name == "nans_64" else 1)
    for pair in ((0, 2), (1, 2), (2, 3)):                       # every live child: v is a NaN, and so is the bound, at every level
        for level in range(last + 1):
            nan_v, bound, kept, dropped = seen[(level,) + pair]
            assert nan_v == kept > 0 and numpy.isnan(bound) and dropped == 0
    nan_v, bound, kept, dropped = seen[(last, 0, 1)]
    assert nan_v > 0 and kept > 0 and dropped == 0
    if name == "nans_64":
        # a NaN v(q) against a bound that is a number, and inf - inf: every live child is kept by a NaN for (ball, speck), and listed
        assert bound == numpy.inf and kept == traversal.level_rows[1] == 832 > nan_v
        assert seen[(1, 0, 3)][3] > 0 and not numpy.isnan(seen[(1, 0, 3)][1])       # while the ordinary pair is pruned
    else:
        assert numpy.isnan(bound)


# ---- both kernel variants ---------------------------------------------------------------------------------------------------

def test_the_edge_scenarios_run_both_kernel_variants():
    figures = {name: hi.table_figures(scenes.edge_scene(name)[2])[0] for name in scenes.EDGES}
    assert figures == {"long_x": 1, "long_y": 1, "long_z": 1, "near_r_equal": 1, "near_r_dropped": 1, "touching": 1,
                       "far_boxes": 1, "far_random_2": 0, "nans": 1, "nans_64": 1}
    assert hi.table_figures(scenes.scene("spheres")[2])[0] == hi.table_figures(scenes.scene("rims")[2])[0] == 1
    assert hi.table_figures(scenes.scene("random_5")[2])[0] == 0
