"""The CPU reference of an assembly's picture (oracle.ray_caster_instances, sdf_oracle.c instance_field) and the scenes the
device is held to with it (assembly_picture_scenes.py), proven without a device: one instance is the single-shape
oracle byte for byte; the default hue is the single-shape colour; every tie scene contains its tie, resolved to the
lower index, and visibly so; the scene list reaches all three workgroup shapes."""
import numpy
import pytest

from codecad_amd import nodes
from codecad_amd.rendering import assembly_picture as ap
from codecad_amd.rendering.ray_caster import RenderOptions
import oracle
import assembly_picture_scenes as scenes
import test_gpu_assembly_picture as loose

SIZE = (64, 48)
OPTIONS = (RenderOptions.no_flags, RenderOptions.false_color, RenderOptions.zebra)


def _arguments(a):
    f = numpy.float32
    return ([list(a[k]) for k in ("origin", "forward", "up", "right")]
            + [f(a[k]) for k in ("pixel_tolerance", "box_radius", "min_distance", "max_distance", "floor_z")])


@pytest.mark.parametrize("name", ["csg_thing", "torus", "mirror_3d", "placed"])
def test_one_instance_is_the_single_shape_oracle(name):
    asm = loose._single(name)
    instances, hues, camera, a = ap.scene(asm, SIZE)
    assert len(instances) == 1
    tape = nodes.make_program(instances[0].shape())
    for options in OPTIONS:
        want = oracle.ray_caster(tape, *_arguments(a), int(options), SIZE, threads=scenes.THREADS)
        got = oracle.ray_caster_instances([tape], hues, *_arguments(a), int(options), SIZE, threads=scenes.THREADS)
        assert got.pixels.shape == want.shape == SIZE + (3,) and numpy.array_equal(got.pixels, want)
        assert numpy.array_equal(oracle.ray_caster_instances([tape], None, *_arguments(a), int(options), SIZE).pixels, want)
        assert got.part_ids.dtype == numpy.int32 and got.depth.dtype == numpy.float32 and got.tied.dtype == numpy.uint8
        assert set(numpy.unique(got.part_ids)) == {-1, 0}
        assert numpy.array_equal(numpy.isfinite(got.depth), got.part_ids == 0)
        assert (got.depth[got.part_ids == 0] > 0).all() and (got.depth[got.part_ids < 0] == numpy.inf).all()
        assert not got.tied.any()


def test_the_default_hue_is_the_single_shape_colour():
    asm = scenes.assembly("gear_train")
    instances, hues, camera, a = ap.scene(asm, SIZE)
    assert (hues == numpy.float32(ap.DEFAULT_HUE)).all() and len(instances) == 8
    tapes = [nodes.make_program(i.shape()) for i in instances]
    with_table = oracle.ray_caster_instances(tapes, hues, *_arguments(a), 0, SIZE, threads=scenes.THREADS)
    without = oracle.ray_caster_instances(tapes, None, *_arguments(a), 0, SIZE, threads=scenes.THREADS)
    for x, y in zip(with_table, without):
        assert numpy.array_equal(x, y)
    assert len(numpy.unique(with_table.part_ids)) >= 5
    # ... and another hue for one part changes that part's lit pixels only
    changed = hues.copy()
    changed[0] = (0.0, 0.2, 1.0)
    other = oracle.ray_caster_instances(tapes, changed, *_arguments(a), 0, SIZE, threads=scenes.THREADS)
    differs = numpy.any(other.pixels != without.pixels, axis=-1)
    assert differs.any() and not differs[without.part_ids != 0].any()
    assert numpy.array_equal(other.part_ids, without.part_ids) and numpy.array_equal(other.depth, without.depth)


def _tie_pictures(name):
    hues = [scenes.HUE_A, scenes.HUE_B, scenes.HUE_C, scenes.HUE_A, scenes.HUE_B, scenes.HUE_C][:len(ap.scene(scenes.assembly(name), (8, 8))[0])]
    return scenes.reference(name, scenes.TIE_SIZE, hues), scenes.reference(name + "_flipped", scenes.TIE_SIZE, hues)


@pytest.mark.parametrize("name, lower, higher", [("tie_pair", 0, 1), ("tie_six", 1, 4)])
def test_the_seam_of_the_two_spheres_ties_and_the_lower_index_wins(name, lower, higher):
    """The camera looks along +y from x = 0 with right = (1, 0, 0), and with an odd width the centre column has
    filmx == 0: every sample of its rays has x == 0, where the two spheres' distances are equal bit for bit and their
    directions differ in the sign of x.  The hues belong to the INDEX, so in both orders the seam has the same part id
    and hue, and what differs between the orders is the direction the lighting took: a rule that picked the other sphere
    would move those pixels."""
    for flipped in ("", "_flipped"):
        a = ap.scene(scenes.assembly(name + flipped), scenes.TIE_SIZE)[3]
        assert a["origin"].x == 0 and a["forward"].x == 0 and tuple(a["right"]) == (1, 0, 0)
    assert scenes.TIE_SIZE[0] % 2 == 1 and scenes.TIE_COLUMN == (scenes.TIE_SIZE[0] - 1) // 2
    one, other = _tie_pictures(name)
    for picture in (one, other):
        column = picture.part_ids[:, scenes.TIE_COLUMN]
        seam = numpy.isin(column, [lower, higher])
        print("%s: %d hit pixels, %d with tied == 2, %d of them in the centre column" % (
            name, (picture.part_ids >= 0).sum(), ((picture.tied == 2) & (picture.part_ids >= 0)).sum(), seam.sum()))
        assert seam.sum() >= 5
        assert (picture.tied[:, scenes.TIE_COLUMN][seam] == 2).all()
        assert (column[seam] == lower).all()
        assert not (picture.tied[:, :scenes.TIE_COLUMN] == 2).any() and not (picture.tied[:, scenes.TIE_COLUMN + 1:] == 2).any()
        assert (picture.part_ids == lower).any() and (picture.part_ids == higher).any()
    seam = numpy.isin(one.part_ids[:, scenes.TIE_COLUMN], [lower, higher])
    assert numpy.array_equal(one.part_ids[:, scenes.TIE_COLUMN], other.part_ids[:, scenes.TIE_COLUMN])
    assert numpy.array_equal(one.depth[:, scenes.TIE_COLUMN].view(numpy.uint32), other.depth[:, scenes.TIE_COLUMN].view(numpy.uint32))
    differing = numpy.any(one.pixels[:, scenes.TIE_COLUMN][seam] != other.pixels[:, scenes.TIE_COLUMN][seam], axis=-1)
    assert differing.all(), "%d of %d seam pixels are the same in both orders" % ((~differing).sum(), seam.sum())


def test_a_part_listed_three_times_is_its_lowest_index():
    """Every sample ties between the three visible copies, with equal directions: `tied` is 1 on every pixel (2 would say
    the directions differ, and they cannot).  The object has index 0 and its hue; the hidden copy takes no index."""
    instances = ap.scene(scenes.assembly("tie_triple"), scenes.TIE_SIZE)[0]
    assert len(instances) == 3 and len(list(scenes.assembly("tie_triple").all_instances())) == 4
    hues = [scenes.HUE_A, scenes.HUE_B, scenes.HUE_C]
    picture = scenes.reference("tie_triple", scenes.TIE_SIZE, hues)
    hit = picture.part_ids >= 0
    print("tie_triple: %d hit pixels, all with tied == 1" % hit.sum())
    assert hit.sum() >= 100 and (picture.tied == 1).all()
    assert set(numpy.unique(picture.part_ids)) == {-1, 0}
    # the picture is the one of a single copy with the first hue, and not with another
    tape = nodes.make_program(instances[0].shape())
    a = ap.scene(scenes.assembly("tie_triple"), scenes.TIE_SIZE)[3]
    alone = [oracle.ray_caster_instances([tape], numpy.float32([h]), *_arguments(a), 0, scenes.TIE_SIZE).pixels.transpose((1, 0, 2))
             for h in hues]
    assert numpy.array_equal(picture.pixels, alone[0])
    assert numpy.any(picture.pixels[hit] != alone[1][hit]) and numpy.any(picture.pixels[hit] != alone[2][hit])


# the workgroup shape of every scene the device tests render (test_gpu_assembly_picture_exact.py asserts the same figures
# from what the library reports on the device)
SHAPES = {"gear_train": 256, "random_4": 256, "random_9": 256, "random_12_blended": 256, "grid_64": 128, "tie_pair": 256,
          "tie_pair_flipped": 256, "tie_six": 256, "tie_six_flipped": 256, "tie_triple": 256, "heavy_64": 64, "placed_gear_train": 256}


def test_the_scenes_reach_all_three_workgroup_shapes():
    """hu_ray_caster_instances: per_lane = lane_bytes + 4 n, and the workgroup is the largest of 256 / 128 / 64 lanes with
    per_lane * lanes <= 48 KiB.  lane_bytes is 16 B per float4 slot of the largest full program (hu_instance_table),
    counted here from the library's own listing of each instance's program."""
    assert set(SHAPES) == set(scenes.SCENES)
    for name, lanes in SHAPES.items():
        asm = scenes.assembly(name)
        n, lane_bytes = len(ap.scene(asm, (8, 8))[0]), scenes.lane_bytes(asm)
        per_lane = lane_bytes + 4 * n
        want = 256 if per_lane * 256 <= 48 * 1024 else 128 if per_lane * 128 <= 48 * 1024 else 64
        print("%s: %d instances, lane_bytes %d, %d lanes" % (name, n, lane_bytes, want))
        assert scenes.workgroup_lanes(lane_bytes, n) == want == lanes, name
    assert set(SHAPES.values()) == {256, 128, 64}
    assert scenes.lane_bytes(scenes.assembly("heavy_64")) == 144 and scenes.lane_bytes(scenes.assembly("tie_pair")) == 16
    assert scenes.n_slots(nodes.make_program(scenes.knot())) == 9
