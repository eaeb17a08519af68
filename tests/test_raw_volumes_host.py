"""The raw volumes of raw_volume_scenes.py hold the edges they are named for: checked on the CPU, as numbers, so that the device
tests over them (test_gpu_thickness_passes.py, test_gpu_blocking_raw.py, test_gpu_overhang_raw.py,
test_gpu_components_raw.py) cannot pass for want of a hard case."""
import numpy
import pytest

import raw_volume_scenes as raw
import thin_walls_scenes as thin
import disassembly_scenes as dis
import overhangs_scenes as over
import assembly_components_scenes as comp
from raw_volume_scenes import SOLID, EMPTY, NONE


def as_data(buffer):
    """The whole device buffer read as a lattice: what a kernel that took the padding for samples would see."""
    return numpy.ascontiguousarray(buffer)


# ---- padded, padded16 --------------------------------------------------------------------------------------------------------

def test_the_padding_holds_the_poison_and_nothing_else_changes():
    ids = raw.block_small_ids()
    buffer, pz = raw.padded(ids, raw.BLOCK_POISON)
    assert pz == 144 and buffer.dtype == numpy.uint8 and buffer.shape == (5, 7, 144) and numpy.array_equal(buffer[:, :, :130], ids)
    assert buffer[0, 0, 130] == 0 and buffer[0, 0, 131] == 1 and buffer[1, 0, 130] == 1 and buffer[0, 1, 130] == 1
    wide, pz = raw.padded16(raw.axis_input("x300"), raw.constant(0))
    assert pz == 32 and wide.dtype == numpy.uint16 and (wide[:, :, 21:] == 0).all() and numpy.array_equal(wide[:, :, :21], raw.axis_input("x300"))
    same, pz = raw.padded(raw.z_ids("2x3x64"), raw.constant(7))
    assert pz == 64 and numpy.array_equal(same, raw.z_ids("2x3x64"))                 # no padding at all
    assert [raw.ceil16(v) for v in (1, 16, 17, 130)] == [16, 16, 32, 144]
    assert {name: pz for name, (_, pz) in raw.Z_LATTICES.items()} == {"3x5x130": 144, "2x3x64": 64, "2x3x65": 80, "1x1x1": 16}
    assert all(raw.ceil16(shape[2]) == pz for shape, pz in list(raw.Z_LATTICES.values()) + list(raw.OVER_VOLUMES.values())
               + list(raw.COMP_VOLUMES.values()))
    assert all(raw.ceil16(v.shape[2]) == v.pitch for v in raw.AXIS_VOLUMES.values())


# ---- the z pass ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("of", raw.Z_OFS)
def test_the_tall_lattice_needs_taps_from_another_segment(of):
    ids = raw.z_ids("3x5x130")
    s = thin.in_set_of(ids, of)
    assert 0.9 < (ids != EMPTY).mean() < 0.995 and set(numpy.unique(ids).tolist()) == set(range(64)) | {EMPTY}
    d = thin.min_plus_1d(raw.z_input_1(ids, of, 65535), 2, 255, 65535, 0)
    far, edge = raw.Z_FAR[of], raw.Z_EDGE[of]
    assert s[far].all() and d[far][64] == 65 * 65 == d.max()                         # more than 64 samples to the nearest background
    assert not s[edge][0] and s[edge][1:].all()
    assert d[edge][64] == 64 * 64 and d[edge][65] == 65 * 65                         # from the tap at z = 0, a segment below
    for K, cap in raw.Z_PARAMS:
        out = thin.min_plus_1d(raw.z_input_1(ids, of, cap), 2, K, cap, 0)
        assert out.min() == 0 and out.max() == min(cap, 4225)
        if K >= 64:                                                                  # the tap that crosses 64 samples decides
            less = thin.min_plus_1d(raw.z_input_1(ids, of, cap), 2, 63, cap, 0)
            assert out[edge][64] == 4096 < less[edge][64] == cap
        if K >= 65:
            assert out[far][64] == 4225 < cap


@pytest.mark.parametrize("of", raw.Z_OFS)
@pytest.mark.parametrize("name", ["3x5x130", "2x3x65"])
def test_the_id_padding_read_as_data_changes_the_z_pass(name, of):
    ids = raw.z_ids(name)
    buffer, pz = raw.padded(ids, raw.z_ids_poison(of))
    nz = ids.shape[2]
    assert pz > nz and (buffer[:, :, nz:] == 0).any()
    changed = False
    for K, cap in raw.Z_PARAMS[1:]:
        want = thin.min_plus_1d(raw.z_input_1(ids, of, cap), 2, K, cap, 0)
        wrong = thin.min_plus_1d(raw.z_input_1(as_data(buffer), of, cap), 2, K, cap, 0)[:, :, :nz]
        changed |= not numpy.array_equal(want, wrong)
    assert changed


@pytest.mark.parametrize("name", list(raw.Z_LATTICES))
def test_the_depth_volumes_hold_both_sides_of_the_radius(name):
    depth = raw.z_depth(name)
    assert depth.dtype == numpy.uint16
    if depth.size > 1:
        assert (depth > raw.RADIUS_SQ).any() and (depth <= raw.RADIUS_SQ).any()
        assert (depth == raw.RADIUS_SQ).any() and (depth == raw.RADIUS_SQ + 1).any()
    else:
        assert depth[0, 0, 0] == raw.RADIUS_SQ + 1
    buffer, pz = raw.padded16(depth, raw.Z_DEPTH_POISON)
    nz = depth.shape[2]
    if pz > nz and depth.size > 1:                                                   # the padding read as data: a core next to z = nz - 1
        assert (buffer[:, :, nz:] == 0).any() and (buffer[:, :, nz:] == 65535).any()
        K, cap = 8, 70
        want = thin.min_plus_1d(raw.z_input_2(depth, cap), 2, K, cap, cap)
        wrong = thin.min_plus_1d(raw.z_input_2(as_data(buffer), cap), 2, K, cap, cap)[:, :, :nz]
        assert not numpy.array_equal(want, wrong)
    if name == "3x5x130":
        for K, cap in raw.Z_PARAMS:
            out = thin.min_plus_1d(raw.z_input_2(depth, cap), 2, K, cap, cap)
            assert (out[1, 2] == cap).all()                                          # no core in the column, none outside
            if K >= 64:
                assert out[0, 1, 64] == 4096 < cap                                   # the core at z = 0, a segment below


# ---- the y and x passes -------------------------------------------------------------------------------------------------------

def test_the_axis_volumes_are_longer_than_a_tile_and_end_ragged():
    v = raw.AXIS_VOLUMES
    assert v["y300"] == ((3, 300, 21), 32, 1) and v["x300"] == ((300, 5, 21), 32, 0) and v["x130"] == ((130, 3, 16), 16, 0)
    assert 5 * 32 == 160 and 160 % 64 == 32                                          # x300: the last column block is half empty
    assert -(-300 // 64) == 5 and 300 - 4 * 64 == 44                                 # five tiles, the last one ragged
    params = set(raw.AXIS_PARAMS)
    assert {(0, 256, 1), (96, 64, 1), (97, 64, 0), (10, 236, 1), (10, 5, 1)} <= {(K, tile, lds) for K, cap, tile, lds in params}
    assert {tile for K, cap, tile, lds in params if K == 255 and lds == 0} == {1, 7, 64, 300, 4096}
    assert all(tile + 2 * K <= 256 for K, cap, tile, lds in params if lds) and 64 + 2 * 97 > 256 and 64 + 2 * 96 == 256
    assert all(cap <= 65535 and K * K < cap for K, cap, tile, lds in params)
    for name in v:
        values = raw.axis_input(name)
        small = (values < raw.TOP).mean()
        assert values.dtype == numpy.uint16 and 0.01 <= small <= 0.03 and values.max() == 65535 and raw.TOP > 255 * 255
        assert int(values.astype(numpy.int64).max()) + 255 * 255 > 65535             # the sum leaves uint16 before the cap is applied


@pytest.mark.parametrize("which", raw.OUTSIDES)
@pytest.mark.parametrize("params", raw.AXIS_PARAMS, ids=str)
@pytest.mark.parametrize("name", list(raw.AXIS_VOLUMES))
def test_far_taps_and_taps_from_another_tile_decide(name, params, which):
    K, cap, tile, lds = params
    v = raw.AXIS_VOLUMES[name]
    values = raw.axis_input(name)
    n, outside = v.shape[v.axis], raw.outside_of(which, cap)
    want = thin.min_plus_1d(values, v.axis, K, cap, outside)
    own, other = raw.own_and_other_tile(values, v.axis, K, cap, outside, tile)
    assert numpy.array_equal(numpy.minimum(cap, numpy.minimum(own, other)), want)     # the two ways agree
    assert (want < cap).any() and (which != "cap" or cap >= raw.TOP or (want == cap).any())
    if K >= 1:
        assert (values.astype(numpy.int64) + K * K > 65535).any()
        nearer = thin.min_plus_1d(values, v.axis, K - 1, cap, outside)
        assert raw.planted_far_tap(n, K, cap, cap) == (K < n - 2)                    # with outside = cap wherever a tap of K is inside
        if raw.planted_far_tap(n, K, cap, outside):
            assert not numpy.array_equal(want, nearer)                               # the farthest tap matters
    if K >= 1 and tile < n:
        assert ((other < own) & (other < cap)).any()                                 # an output below the cap from another tile


@pytest.mark.parametrize("of", raw.FINISH_OFS)
@pytest.mark.parametrize("params", raw.FINISH_PARAMS, ids=str)
def test_the_finishing_passes_count_many_parts_on_both_sides_of_the_cap(params, of):
    K, cap, tile, lds = params
    ids = raw.finish_ids()
    assert set(numpy.unique(ids).tolist()) == set(range(64)) | {EMPTY}
    out, core_counts, thin_ids, thin_counts = raw.finish_reference(K, cap, cap, of)
    assert (out == cap).any() and (out < cap).any()
    assert sum(c > 0 for c in core_counts) == 64                                     # every accumulator is used
    assert ((out == cap) & (ids == EMPTY)).any()                                     # an empty sample at the cap: nobody's count
    assert sum(core_counts) == int(((out == cap) & (ids != EMPTY)).sum())
    assert sum(thin_counts) == int((thin_ids != EMPTY).sum()) > 0 and (thin_ids == EMPTY).any()
    assert sum(c > 0 for c in thin_counts) == (64 if of == SOLID else 1)


# ---- hu_blocking_lines --------------------------------------------------------------------------------------------------------

def test_the_small_blocking_volume_and_its_padding():
    ids = raw.block_small_ids()
    assert ids.shape == (5, 7, 130) and set(numpy.unique(ids).tolist()) == set(range(64)) | {EMPTY}
    distance, witness = raw.block_small_reference(64)
    again = dis.running_blocking(ids, 64)
    assert numpy.array_equal(distance, again[0]) and numpy.array_equal(witness, again[1])   # the walk equals the definition
    assert (distance != dis.NEVER).sum() > 2000 and (distance == dis.NEVER).any()
    buffer, pz = raw.padded(ids, raw.BLOCK_POISON)
    wrong = dis.running_blocking(as_data(buffer), 64)
    for axis in range(3):                                                            # pairs along x and y, shorter distances along z
        assert not numpy.array_equal(wrong[0][axis], distance[axis])
    cut, cut_witness = raw.block_small_reference(40)
    # a part between two others hides neither: with ids 40..63 empty the first 40 parts keep their distances, and an id from
    # n up may do nothing but end a run
    assert cut.shape == (3, 40, 40) and numpy.array_equal(cut, distance[:, :40, :40])
    assert (ids >= 40).sum() > 1000
    walked = dis.running_blocking(numpy.where(ids < 40, ids, EMPTY).astype(numpy.uint8), 40)
    assert numpy.array_equal(cut, walked[0]) and numpy.array_equal(cut_witness, walked[1])


@pytest.mark.parametrize("na", raw.WIDE_NA)
@pytest.mark.parametrize("axis", [0, 1])
def test_a_second_unit_would_give_wrong_keys_from_stale_last_indices(axis, na):
    ids = raw.wide_ids(axis, na)
    assert ids.shape == raw.wide_shape(axis, na) and ids.shape[axis] == na and ids.shape[1 - axis] == 5000
    units, segments = raw.wide_units(axis, na)
    assert units == 10000 > raw.GRID_WAVEFRONTS == 8192 and units - raw.GRID_WAVEFRONTS == 1808    # wavefronts with two units
    first, second = (ids[:, :4096], ids[:, 4096:]) if axis == 0 else (ids[:4096], ids[4096:])
    assert set(numpy.unique(first).tolist()) == {0, 1, EMPTY} and set(numpy.unique(second).tolist()) == {2, 3, EMPTY}
    distance, witness = raw.wide_reference(axis, na)
    good = raw.walked_keys(ids, axis, 4, stale=False)
    stale = raw.walked_keys(ids, axis, 4, stale=True)
    ones = numpy.uint64(0xffffffffffffffff)
    field = lambda keys, shift: ((keys >> numpy.uint64(shift)) & numpy.uint64(0xffff)).astype(numpy.int64)      # noqa: E731
    assert numpy.array_equal(numpy.where(good == ones, dis.NEVER, field(good, 48)), distance[axis])             # the walk is the definition
    for k, shift in enumerate((32, 16, 0)):
        assert numpy.array_equal(numpy.where(good == ones, -1, field(good, shift)), witness[axis, :, :, k])
    for i in (0, 1):
        for j in (2, 3):                                                             # no line holds both: never, unless `last` is stale
            assert distance[axis, i, j] == dis.NEVER and distance[axis, j, i] == dis.NEVER
            assert stale[i, j] != ones and good[i, j] == ones
    if na >= 3:
        assert (distance[axis][:2, :2] != dis.NEVER).sum() == 2 and (distance[axis][2:, 2:] != dis.NEVER).sum() == 2
    else:
        assert (distance[axis] == dis.NEVER).all()                                   # one sample a line: nothing lies beyond anything
    assert {1, 3, 8, 9, 17} == set(raw.WIDE_NA)                                       # less than a batch, a batch, a batch and one, two and one


# ---- the overhang kernels -----------------------------------------------------------------------------------------------------

def test_the_overhang_volumes():
    ids = raw.over_ids("noise")
    assert ids.shape == (5, 7, 130) and 0.4 < (ids != EMPTY).mean() < 0.5 and set(numpy.unique(ids).tolist()) == set(range(64)) | {EMPTY}
    assert (raw.over_ids("empty") == EMPTY).all() and raw.over_ids("line64").shape == (1, 1, 64)
    ref = raw.over_reference("empty", 2, True, 1, SOLID)
    assert ref.first_layer == 130 and (ref.overhang_ids == EMPTY).all() and (ref.support_ids == EMPTY).all() and ref.plate_landings == 0
    line = raw.over_reference("line64", 2, True, 0, SOLID)
    assert sum(line.overhang_counts) > 5 and sum(line.support_counts) > 5 and sum(line.landing_counts) > 5
    for of in raw.OVER_OFS:
        for axis, up in dis.DIRECTIONS:
            ref = raw.over_reference("noise", axis, up, 1, of)
            assert sum(ref.overhang_counts) > 0 and sum(ref.support_counts) > 0 and sum(ref.overhang_counts) == sum(ref.landing_counts) + ref.plate_landings
    counts = [sum(raw.over_reference("noise", 2, True, r, SOLID).overhang_counts) for r in raw.OVER_REACH]
    assert counts == sorted(counts, reverse=True) and len(set(counts)) == len(counts)      # every reach is another answer


@pytest.mark.parametrize("of", [SOLID, 63])
@pytest.mark.parametrize("axis,up,reach_sq", [(2, False, 0), (0, True, 1), (1, False, 1)])
def test_the_overhang_padding_read_as_data_would_change_the_top_layer(axis, up, reach_sq, of):
    ids = raw.over_ids("noise")
    buffer, pz = raw.padded(ids, raw.OVER_POISON)
    assert pz == 144 and set(numpy.unique(buffer[:, :, 130:]).tolist()) == {63, EMPTY}
    want = over.reference_overhangs(ids, axis, up, reach_sq, of, 64)
    wrong = over.reference_overhangs(as_data(buffer), axis, up, reach_sq, of, 64)
    top = (slice(None), slice(None), 129)
    # along x and y an overhang at z = nz - 1 is supported from the padding; downwards along z that layer is the plate no more
    assert not numpy.array_equal(want.overhang_ids[top], wrong.overhang_ids[top])
    assert ((want.overhang_ids[top] != EMPTY).sum() > (wrong.overhang_ids[top] != EMPTY).sum()) == (axis != 2)
    if axis != 2:
        assert numpy.array_equal(want.overhang_ids[:, :, :129], wrong.overhang_ids[:, :, :129])


# ---- the component kernels ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solid", [0, 1])
@pytest.mark.parametrize("name", list(raw.COMP_VOLUMES))
def test_the_component_volumes(name, solid):
    ids = raw.comp_ids(name)
    shape, pz = raw.COMP_VOLUMES[name]
    assert ids.shape == shape and 0.4 < (ids != EMPTY).mean() < 0.6
    ref = raw.comp_reference(name, solid)
    assert numpy.array_equal(ref.labels, comp.propagated_labels((ids != EMPTY) == bool(solid)))
    assert len(ref.components) > (50 if name == "noise" else 20)                     # far more than a first table of one row
    assert any(63 in c.parts for c in ref.components) and any(0 in c.parts for c in ref.components)   # bit 63 of `parts`, and bit 0
    assert any(c.touches_border for c in ref.components) and (name != "noise" or any(not c.touches_border for c in ref.components))
    if name == "noise":
        assert all(d % t for d, t in zip(shape, comp.TILE)) and max(c.count for c in ref.components) > 500
    buffer, pz = raw.padded(ids, raw.COMP_POISON)
    assert set(numpy.unique(buffer[:, :, shape[2]:]).tolist()) == {63, EMPTY}          # it would join S under either `solid`
    wrong = comp.reference_components(as_data(buffer), SOLID if solid else comp.EMPTY_SPACE)
    counts = lambda r: sorted(c.count for c in r.components)                         # noqa: E731
    assert counts(wrong) != counts(ref)
