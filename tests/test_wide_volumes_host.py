"""The wide cases of wide_volume_scenes.py, on the CPU: every case has more units than the grid has wavefronts; every walk emulated
as written EQUALS the reference, and emulated with its state carried from a wavefront's first unit into its second it DIFFERS,
so the device tests over these cases cannot pass for want of a hard case; and the cheap references of the cases that decompose
are the definitions' on a small twin of the same construction and on a crop of the wide volume."""
import numpy
import pytest

import raw_volume_scenes as raw
import wide_volume_scenes as wide
import drainage_scenes as drain
import islands_scenes as isl
import flow_length_scenes as flow
from raw_volume_scenes import GRID_WAVEFRONTS, WIDE_NA, SOLID, EMPTY, NONE

DIRECTIONS = (True, False)


# ---- the arithmetic -------------------------------------------------------------------------------------------------------

def test_every_wide_case_has_more_units_than_the_grid_has_wavefronts():
    assert GRID_WAVEFRONTS == 4 * 2048
    columns = {name: shape[0] * shape[1] for name, shape in wide.REACH_SHAPES.items()}
    assert columns == {"100x100x70": 10000, "129x128x70": 16512, "91x91x128": 8281}
    assert all(n > GRID_WAVEFRONTS for n in columns.values())
    assert wide.walked(10000) == (1808, 0)                                          # a minority of the wavefronts
    assert wide.walked(16512) == (8192, 128)                                        # all of them, and 128 a third
    assert wide.walked(8281) == (89, 0)
    # k_geo_seed and k_geo_stats take four units a wavefront at the least: their cap is past 4 x the grid
    segments = -(-70 // 64)
    assert 16512 * segments == 33024 > 4 * GRID_WAVEFRONTS and wide.walked(33024) == (8192, 8192)
    assert 10000 * segments < 4 * GRID_WAVEFRONTS                                   # (the smaller shape does not reach it)
    for axis in (0, 1):
        for na in WIDE_NA:
            units, segments = raw.wide_units(axis, na)
            assert units == 10000 > GRID_WAVEFRONTS and wide.walked(units) == (1808, 0)
            assert wide.tool_ids(axis, na).shape == raw.wide_shape(axis, na) == wide.seed_lines(axis, na)[0].shape
    first = GRID_WAVEFRONTS // segments                                             # the lines a wavefront walks first
    assert wide.line_kinds().tolist() == [0] * first + [1] * (raw.WIDE_LINES - first)


# ---- the decomposed references ----------------------------------------------------------------------------------------------

def linear(labels, r, pitch):
    """The linear indices of own_labels' buffer indices."""
    nz = r.shape[2]
    q = labels[:, :, :nz].astype(numpy.int64)
    return numpy.where(r, q - (q // pitch) * (pitch - nz), NONE).astype(numpy.uint32)


def pieces():
    """(ids, r, flags) of the small twins and of crops of the wide volumes, per member."""
    for member in ("empty", "solid"):
        for shape in (wide.TWIN, wide.TWIN_FULL):
            yield member, wide.reach_case(shape, member, wide.TWIN_GRID)
        c = wide.reach_case(wide.REACH_SHAPES["100x100x70"], member)
        x = GRID_WAVEFRONTS // 100                                                   # the row of columns in which kind 1 begins
        at = (slice(x - 3, x + 5), slice(0, 100, 9), slice(None))                   # both kinds
        assert len(set(wide.kinds(10000).reshape(100, 100)[at[:2]].ravel().tolist())) == 2
        yield member, wide.Reach(*(numpy.ascontiguousarray(a[at]) for a in c))


def test_a_layer_component_of_a_reach_case_is_one_sample():
    for member, c in pieces():
        r = wide.members(c.ids, member)
        assert numpy.array_equal(r, c.r) and r.any() and not r.all()
        labels = wide.own_labels(r, raw.ceil16(r.shape[2]) + 16)
        assert numpy.array_equal(linear(labels, r, raw.ceil16(r.shape[2]) + 16), drain.layer_labels(r, 2))
        assert (labels[:, :, r.shape[2]:] == NONE).all()
    for shape in wide.REACH_SHAPES.values():                                        # at full size: no two lateral neighbours
        for member in ("empty", "solid"):
            r = wide.reach_case(shape, member).r
            assert not (r[1:] & r[:-1]).any() and not (r[:, 1:] & r[:, :-1]).any()


def test_the_references_of_the_reach_cases_are_the_definitions():
    for member, c in pieces():
        for up in DIRECTIONS:
            if member == "empty":
                ref = drain.reference_of(c.ids, 64, 2, up)
                x = wide.risen(c.r, drain.seeds(c.r, 2, up), 2, up)
                assert numpy.array_equal(x, ref.escapes) and numpy.array_equal(x, drain.layered_escape(c.r, 2, up))
                trapped, counts = wide.trapped_of(c.ids, x, 2, up)
                assert numpy.array_equal(trapped, ref.trapped_ids) and counts == ref.trapped_counts
            else:
                for of in (SOLID, 63):
                    s = isl.in_set_of(c.ids, of)
                    ref = isl.reference_of(c.ids, 64, 2, up, of)
                    g = wide.risen(s, isl.seeds(s, 2, up), 2, up)
                    assert numpy.array_equal(g, ref.grounded)
                    (floating, fc), (start, _), (join, _) = wide.marks_of(c.ids, s, g, 2, up)
                    assert numpy.array_equal(floating, ref.floating_ids) and numpy.array_equal(start, ref.start_ids)
                    assert numpy.array_equal(join, ref.join_ids) and fc == list(ref.floating_counts)


def test_a_layer_component_of_a_seed_case_is_a_line():
    for axis in (0, 1):
        ids, r = wide.seed_lines(axis, 3)
        first = GRID_WAVEFRONTS // -(-raw.WIDE_NZ // 64)                             # the first line of kind 1
        at = (slice(None), slice(first - 6, first + 6)) if axis == 0 else (slice(first - 6, first + 6), slice(None))
        piece = numpy.ascontiguousarray(r[at])
        pitch = 96
        assert numpy.array_equal(linear(wide.line_labels(piece, pitch), piece, pitch), isl.layer_labels(piece, axis))
        s = isl.in_set_of(numpy.ascontiguousarray(ids[at]), SOLID)
        assert numpy.array_equal(s, piece)
        for up in DIRECTIONS:
            h0 = isl.first_layer(s, axis, up)
            layer = h0 if up else piece.shape[axis] - 1 - h0
            assert numpy.array_equal(wide.seeded_lines(piece, axis, layer, False), isl.seeds(s, axis, up))


# ---- the cases bite ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(wide.REACH_SHAPES))
def test_the_reach_walks_equal_their_references_and_a_stale_state_shows(name):
    shape = wide.REACH_SHAPES[name]
    full = shape[2] % 64 == 0
    for up in DIRECTIONS:
        c = wide.reach_case(shape, "empty")
        want = wide.risen(c.r, c.flags, 2, up)
        assert numpy.array_equal(wide.rise(c.r, c.flags, up, False), want) and (want & ~c.flags).any()
        assert numpy.array_equal(wide.rise(c.r, c.flags, up, True), want) != full    # (ragged: the carry cannot leave a column)
        trapped = wide.trapped_of(c.ids, c.flags, 2, up)[0]
        assert numpy.array_equal(wide.floor(c.ids, c.flags, up, False), trapped)
        stale = wide.floor(c.ids, c.flags, up, True)
        wrong = stale != trapped
        assert wrong.any() and (trapped[wrong] == EMPTY).all() and (stale[wrong] < 64).all()     # a floor where the column has none yet
        c = wide.reach_case(shape, "solid")
        for of in (SOLID, 63):
            s = isl.in_set_of(c.ids, of)
            g = c.flags & s
            start = wide.marks_of(c.ids, s, g, 2, up)[1][0]
            assert numpy.array_equal(wide.mark_starts(c.ids, s, g, up, False), start)
            assert numpy.array_equal(wide.mark_starts(c.ids, s, g, up, True), start)    # (the step beyond the last word clears the carry)


@pytest.mark.parametrize("name", list(wide.COLUMN_SHAPES))
def test_the_column_sweep_equals_swept_and_a_stale_carry_shows(name):
    shape = wide.COLUMN_SHAPES[name]
    for of in wide.GEO_OFS:
        s = flow.in_set_of(wide.geo_ids(shape), of)
        field = wide.geo_field(shape, of)
        want, lowered = flow.swept(field, s, 2)
        assert lowered and numpy.array_equal(wide.geo_sweep(field, s, False), want)
        stale = wide.geo_sweep(field, s, True)
        assert (stale != want).any() and numpy.array_equal(stale[~s], want[~s])
        assert set(numpy.argwhere(stale != want)[:, 0].tolist()) >= {shape[0] - 1}  # (the last columns are second or third units)


@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("na", WIDE_NA)
def test_the_line_walks_equal_the_tool_reference_and_a_stale_state_shows(axis, na):
    ids = wide.tool_ids(axis, na)
    for up in DIRECTIONS:
        for of in wide.TOOL_OFS:
            ref = wide.tool_reference(axis, na, up, of)
            keys = wide.keys_of(ref)
            assert numpy.array_equal(wide.line_keys(ids, axis, up, of, False), keys)
            stale = wide.line_keys(ids, axis, up, of, True)
            wrong = stale != keys
            first = GRID_WAVEFRONTS // -(-raw.WIDE_NZ // 64)
            assert (wrong & (keys == 0)).any() and not wrong[:first].any()           # a key where the line holds no sample of S
            cut = ref.cut * 256 + ref.crowd
            assert numpy.array_equal(wide.line_rest(ids, axis, up, of, keys, cut, False)[0], ref.rest_ids)
            assert (wide.line_rest(ids, axis, up, of, keys, cut, True)[0] != ref.rest_ids).any()


@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("na", WIDE_NA)
def test_a_second_unit_of_the_seeds_has_lines_of_its_own_to_flag(axis, na):
    ids, r = wide.seed_lines(axis, na)
    for layer in sorted({0, na - 1}):
        honest, reused = wide.seeded_lines(r, axis, layer, False), wide.seeded_lines(r, axis, layer, True)
        assert honest.any() and (honest & ~reused).any() and not (reused & ~honest).any()
