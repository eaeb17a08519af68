"""The CPU proof that the cases of test_gpu_pitch_alignment.py hold their edges: the arithmetic of every placement, that the
poison over the padding bites at the wider pitches too (the reference over the padding as data differs from the true one), that
a label converted with the wrong pitch is another label, and that the helpers which now take a pitch give the bytes they gave
before when they are called without one.  No case had to be dropped: where a raw case of the suite could not meet the poison's
condition (an overhang line of one sample across, a drain over 2 x 3 samples that are all border) pitched_buffers.py takes the
first 64 layers of a larger raw case instead, and names the arms a poison cannot reach (its `arms` and `blind`)."""
import numpy
import pytest

import pitched_buffers as pb
import raw_volume_scenes as raw
import wall_thickness_scenes as wall
from pitched_buffers import EMPTY, NONE, SOLID, ceil16

WIDE = [(family, case, placement) for family, case, placement in pb.combinations() if placement != "tight"]
ALIGNMENTS = (1, 2, 4, 8, 16)


def test_the_cases_cover_the_edges_of_nz_in_every_family():
    for family, cases in pb.CASES.items():
        groups = {"thickness": ("z:", "axis:", "local:"), "reach": ("drain:", "ground:")}.get(family, ("",))
        for prefix in groups:
            nzs = [pb.ids_of(family, case).shape[2] for case in cases if case.startswith(prefix)]
            assert any(nz % 16 for nz in nzs), (family, prefix)
            assert any(nz > 64 for nz in nzs) and any(nz % 64 == 0 for nz in nzs), (family, prefix, nzs)
        assert (family, pb.CONTROL[family], "tight") in pb.combinations()
    # the line kernels: all three axes, both directions
    for family in ("overhang", "reach", "tool"):
        for case in pb.CASES[family]:
            assert {tuple(arm[:2]) for arm in pb.arms(family, case)} == {(a, u) for a in range(3) for u in (True, False)}
    # a kernel instantiation of hu_thickness_local each: K <= 4, <= 10, > 10
    ks = sorted(int(numpy.sqrt(wall.RAW_BY_NAME[name].r2)) for name in pb.LOCAL_CASES.values())
    assert ks[0] <= 4 and any(4 < k <= 10 for k in ks) and ks[-1] > 10


@pytest.mark.parametrize("family,case,placement", pb.combinations(), ids=lambda v: str(v).replace(":", "_"))
def test_the_arithmetic_of_the_placement(family, case, placement):
    place = pb.PLACEMENTS[placement]
    nz = pb.ids_of(family, case).shape[2]
    pitch = place.pitch_of(nz)
    assert pitch % 16 == 0 and nz <= pitch <= 65536
    if placement == "tight":
        assert pitch == ceil16(nz)
    if placement == "word":
        assert pitch == ceil16(nz) + 16
    if placement == "segment":
        assert pitch - nz >= 64 and pitch % 64 != 0 and pitch // 64 > -(-nz // 64)
    for base in (0, 256):
        for a in ALIGNMENTS:
            at = pb.address(base, a, place)
            assert pb.GUARD <= at - base <= pb.slack(a) - pb.GUARD                  # a guard before, and room for one after
            if place.minimal:
                assert at % (2 * a) == a
            else:
                assert at % 256 == 0
    for arm in pb.arms(family, case):                                               # the whole padding is poison
        for name, image in pb.inputs(family, case, arm, pitch).items():
            assert image.shape[2] == pitch, name


@pytest.mark.parametrize("family,case,placement", WIDE, ids=lambda v: str(v).replace(":", "_"))
def test_the_poison_bites_at_the_wider_pitch(family, case, placement):
    """The reference over the buffer with its padding AS DATA differs from the true one on the lattice, in a count or in a
    table: a kernel that read the padding would fail the device test.  A blind arm (pitched_buffers.blind) cannot differ."""
    pitch = pb.PLACEMENTS[placement].pitch_of(pb.ids_of(family, case).shape[2])
    for arm in pb.arms(family, case):
        assert pb.widened_differs(family, case, arm, pitch) != pb.blind(family, case, arm), arm
    assert not all(pb.blind(family, case, arm) for arm in pb.arms(family, case))


@pytest.mark.parametrize("family,case,placement", [c for c in WIDE if c[0] in ("components", "reach")], ids=lambda v: str(v).replace(":", "_"))
def test_a_label_converted_with_the_wrong_pitch_is_another_label(family, case, placement):
    nz = pb.ids_of(family, case).shape[2]
    pitch = pb.PLACEMENTS[placement].pitch_of(nz)
    changed = []
    for arm in pb.arms(family, case):
        kind, linear = next(v for v in pb.reference(family, case, arm).values() if v[0] == "labels")
        entries = pb.buffer_index(linear, nz, pitch)
        assert numpy.array_equal(pb.linear_index(entries, nz, pitch), linear)
        wrong = pb.linear_index(entries, nz, ceil16(nz))
        assert ((wrong == NONE) == (linear == NONE)).all(), arm
        changed.append(bool((wrong != linear).any()))
    # (line130 is one column: row 0 starts at 0 under every pitch; a solid that is one component has its one label in row 0)
    assert any(changed) != (linear.shape[0] * linear.shape[1] == 1), changed


# ---- the helpers that now take a pitch, as they were -----------------------------------------------------------------------

def _old_fill(dtype, values, poison):
    nx, ny, nz = values.shape
    pz = ceil16(nz)
    out = numpy.empty((nx, ny, pz), dtype=dtype)
    out[:, :, :nz] = values
    if pz > nz:
        x, y, z = numpy.meshgrid(numpy.arange(nx), numpy.arange(ny), numpy.arange(nz, pz), indexing="ij")
        out[:, :, nz:] = poison(x, y, z)
    return out, pz


def _old_padded_ids(ids, solid):
    """padded_ids of the drainage test (solid = 63) and of the islands test (solid = 63 or `of`), and, with the values 0 and 1
    where these have `solid` and 255, the padding of raw_call in the contacts test."""
    nx, ny, nz = ids.shape
    pz = -(-nz // 16) * 16
    out = numpy.empty((nx, ny, pz), dtype=numpy.uint8)
    out[:, :, :nz] = ids
    odd = (numpy.arange(nz, pz) + numpy.arange(nx)[:, None, None] + numpy.arange(ny)[None, :, None]) % 2
    out[:, :, nz:] = odd if solid is None else numpy.where(odd, EMPTY, solid)
    return out, pz


def _old_raw_buffers(case):
    cap = case.r2 + 1
    s = wall.in_set_of(case.ids, case.of)
    ids, pz = _old_fill(numpy.uint8, case.ids, raw.constant(0 if case.of == SOLID else case.of))
    field, _ = _old_fill(numpy.uint16, numpy.where(s, case.field, cap), raw.constant(cap))
    return ids, field, pz


def same(a, b):
    return a[1] == b[1] and a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes()


def test_the_helpers_called_without_a_pitch_give_the_bytes_they_gave_before():
    import test_gpu_contacts
    import test_gpu_drainage
    import test_gpu_islands
    import test_gpu_geodesic_raw
    for case in pb.CASES["geodesic"]:                                               # the geodesic family pads as the geodesic raw test does
        for of, in pb.arms("geodesic", case):
            ids, field = pb.geodesic_ids(case), pb.geodesic_field(case, of)
            assert same(raw.padded(ids, pb.geodesic_poison(of)), _old_fill(numpy.uint8, ids, test_gpu_geodesic_raw.ids_poison(of)))
            assert same(pb.flow.padded32(field, raw.constant(0)), _old_fill(numpy.uint32, field, raw.constant(0)))
            given = pb.inputs("geodesic", case, (of,))
            assert same((given["ids"], 0), (raw.padded(ids, pb.geodesic_poison(of))[0], 0)) and not given["dist"][:, :, ids.shape[2]:].any()
            s = pb.flow.in_set_of(ids, of)
            assert s[:, :, -1].any() and (field[:, :, -1][s[:, :, -1]] == NONE).all()     # a top in S that the padding's zeros would lower
    for name in raw.Z_LATTICES:
        for of in raw.Z_OFS:
            assert same(raw.padded(raw.z_ids(name), raw.z_ids_poison(of)), _old_fill(numpy.uint8, raw.z_ids(name), raw.z_ids_poison(of)))
        assert same(raw.padded16(raw.z_depth(name), raw.Z_DEPTH_POISON), _old_fill(numpy.uint16, raw.z_depth(name), raw.Z_DEPTH_POISON))
    for name in raw.AXIS_VOLUMES:
        assert same(raw.padded16(raw.axis_input(name), raw.constant(0)), _old_fill(numpy.uint16, raw.axis_input(name), raw.constant(0)))
    for ids, poison in ((raw.block_small_ids(), raw.BLOCK_POISON), (raw.over_ids("noise"), raw.OVER_POISON), (raw.comp_ids("noise"), raw.COMP_POISON)):
        assert same(raw.padded(ids, poison), _old_fill(numpy.uint8, ids, poison))
    for case in wall.RAW_CASES:
        new, old = wall.raw_buffers(case), _old_raw_buffers(case)
        assert new[2] == old[2] and same((new[0], 0), (old[0], 0)) and same((new[1], 0), (old[1], 0)), case.name
    for name in pb.drain.RAW_NAMES:
        assert same(test_gpu_drainage.padded_ids(pb.drain.raw_ids(name)), _old_padded_ids(pb.drain.raw_ids(name), 63)), name
    for name in pb.isl.RAW_NAMES:
        for of in (SOLID, 0, 1):
            assert same(test_gpu_islands.padded_ids(pb.isl.raw_ids(name), of), _old_padded_ids(pb.isl.raw_ids(name), 63 if of == SOLID else of)), name
    for name in pb.con.RAW_NAMES:
        assert same(raw.padded(pb.con.raw_ids(name), raw.CONTACT_POISON), _old_padded_ids(pb.con.raw_ids(name), None)), name
    assert test_gpu_contacts.raw_call.__defaults__ == (None,)                        # (raw_call pads with just that, at ceil16(nz))


def test_a_pitch_is_taken_as_it_is_given_and_refused_where_the_entry_points_would():
    ids = raw.comp_ids("noise")
    image, pz = raw.padded(ids, raw.COMP_POISON, 112)
    assert pz == 112 and image.shape == ids.shape[:2] + (112,) and numpy.array_equal(image[:, :, :33], ids)
    x, y, z = numpy.meshgrid(numpy.arange(9), numpy.arange(17), numpy.arange(33, 112), indexing="ij")
    assert numpy.array_equal(image[:, :, 33:], raw.COMP_POISON(x, y, z))             # the WHOLE padding, not its first word
    for bad in (24, 32, 65552):
        with pytest.raises(AssertionError):
            raw.padded(ids, raw.COMP_POISON, bad)
