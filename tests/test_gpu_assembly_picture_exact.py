"""The picture of an assembly on the device (csrc/instance_rays.hip) against the CPU reference written from its definition
(oracle.ray_caster_instances): pixels, part ids and depth EQUAL, with skipping and without, over the scenes of
test_gpu_assembly_picture.py, exact ties, images whose rim cuts tiles, wavefronts and workgroups, all three workgroup
shapes, explicit colours and a placed assembly.  test_assembly_picture_reference_host.py proves on the CPU that the
tie scenes contain their ties and which workgroup shape each scene lands on.

The reference on 16 threads, per scene and render, programs included: gear train 0.16 s at 160 x 120 and 0.09 s at
80 x 60; random_4 0.11 / 0.05 s; random_9 0.51 / 0.20 s; random_12_blended 0.09 / 0.06 s; grid_64 0.35 / 0.35 s; the tie
scenes 0.01 - 0.04 s at 61 x 45; heavy_64 1.0 s at 45 x 37 (most of it the 64 programs, built once)."""
import numpy
import pytest

from codecad_amd import _instance_cells as cells
from codecad_amd.hip_util import manager as hip_manager
from codecad_amd.rendering import assembly_picture as ap
from codecad_amd.rendering.ray_caster import RenderOptions
import assembly_picture_scenes as scenes
from test_assembly_picture_reference_host import SHAPES

pytestmark = pytest.mark.gpu

OPTIONS = (RenderOptions.no_flags, RenderOptions.false_color, RenderOptions.zebra)
INDEX_HUES = [scenes.HUE_A, scenes.HUE_B, scenes.HUE_C, scenes.HUE_A, scenes.HUE_B, scenes.HUE_C]


def _hex(v):
    return "0x%08x" % int(numpy.float32(v).view(numpy.uint32))


def check(name, size, colors, options):
    """The device's picture of the scene, with skipping and without, equals the reference -> the reference."""
    want = scenes.reference(name, size, colors, options)
    for skip in (True, False):
        got = ap.render_assembly_pixels(scenes.assembly(name), size, colors=colors, options=options, skip=skip)
        assert got.pixels.shape == want.pixels.shape and got.part_ids.shape == want.part_ids.shape == got.depth.shape
        differs = (numpy.any(got.pixels != want.pixels, axis=-1) | (got.part_ids != want.part_ids)
                   | (got.depth.view(numpy.uint32) != want.depth.view(numpy.uint32)))
        if differs.any():
            y, x = (int(v) for v in numpy.argwhere(differs)[0])
            print("%s %s options %d skip %s: %d of %d pixels differ, the first at column %d, row %d: pixel %s / %s, id %d / %d, "
                  "depth %s / %s, tied %d (device / reference)" % (
                      name, size, int(options), skip, differs.sum(), differs.size, x, y, got.pixels[y, x].tolist(),
                      want.pixels[y, x].tolist(), got.part_ids[y, x], want.part_ids[y, x], _hex(got.depth[y, x]),
                      _hex(want.depth[y, x]), want.tied[y, x]))
        assert numpy.array_equal(got.pixels, want.pixels)
        assert numpy.array_equal(got.part_ids, want.part_ids)
        assert numpy.array_equal(got.depth.view(numpy.uint32), want.depth.view(numpy.uint32))
    return want


# ---- the scenes of the loose tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gear_train", "random_4", "random_9", "random_12_blended", "grid_64"])
def test_the_scenes_equal_the_reference(hip, name):
    want = check(name, (160, 120), "parts", RenderOptions.no_flags)
    hit = want.part_ids >= 0
    print("%s: %d pixels hit, %d parts seen, %d hit pixels with tied == 2" % (
        name, hit.sum(), len(numpy.unique(want.part_ids[hit])), ((want.tied == 2) & hit).sum()))
    assert len(numpy.unique(want.part_ids[hit])) >= 3
    check(name, (80, 60), "parts", RenderOptions.false_color)
    check(name, (80, 60), "parts", RenderOptions.zebra)


# ---- ties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, lower", [("tie_pair", 0), ("tie_pair_flipped", 0), ("tie_six", 1), ("tie_six_flipped", 1)])
def test_a_tie_goes_to_the_lower_index(hip, name, lower):
    n = len(ap.scene(scenes.assembly(name), scenes.TIE_SIZE)[0])
    for options in OPTIONS:
        want = check(name, scenes.TIE_SIZE, INDEX_HUES[:n], options)
        seam = (want.tied[:, scenes.TIE_COLUMN] == 2) & (want.part_ids[:, scenes.TIE_COLUMN] >= 0)
        assert seam.sum() >= 5 and (want.part_ids[:, scenes.TIE_COLUMN][seam] == lower).all()


def test_a_part_listed_three_times(hip):
    for options in OPTIONS:
        want = check("tie_triple", scenes.TIE_SIZE, INDEX_HUES[:3], options)
        assert (want.tied == 1).all() and set(numpy.unique(want.part_ids)) == {-1, 0}


# ---- rims ----------------------------------------------------------------------------------------------------------------
# 61 x 45: 8 x 6 tiles, the last column and row of tiles cut; 45 x 37: 6 x 5 = 30 tiles, cut the same way, and a workgroup
# of 256 lanes ends with two wavefronts past the image; 8 x 8: one tile; 3 x 5: fewer pixels than lanes
@pytest.mark.parametrize("size", [(61, 45), (45, 37), (8, 8), (3, 5)])
@pytest.mark.parametrize("name", ["gear_train", "tie_pair"])
def test_images_that_end_inside_a_tile(hip, name, size):
    assert SHAPES[name] == 256
    tiles = -(-size[0] // 8) * -(-size[1] // 8)
    assert size != (45, 37) or (tiles == 30 and tiles % 4 == 2)
    for options in OPTIONS:
        check(name, size, "parts", options)


# ---- workgroup shapes ----------------------------------------------------------------------------------------------------
def test_the_workgroup_shape_of_every_scene(hip):
    """What hu_instance_table reports on the device is what the host test counted, and with it the rule gives the shape
    stated there: 256 lanes for the small assemblies, 128 for grid_64, 64 for heavy_64."""
    for name, lanes in SHAPES.items():
        instances = ap.scene(scenes.assembly(name), (8, 8))[0]
        table, distance_only, lane_bytes = cells.device_table(instances, hip_manager.queue, full_programs=True)
        table.release()
        print("%s: %d instances, lane_bytes %d, %d lanes" % (name, len(instances), lane_bytes, lanes))
        assert distance_only == 0 and lane_bytes == scenes.lane_bytes(scenes.assembly(name))
        assert scenes.workgroup_lanes(lane_bytes, len(instances)) == lanes


def test_sixty_four_lanes(hip):
    """heavy_64: 64 instances and a register file of 144 B per lane (the knot: rounded unions nested 4 deep, each made
    symmetrical) -> 400 B per lane, workgroups of one wavefront; the bounds start at 144 * 64 B and stride 64 lanes."""
    assert SHAPES["heavy_64"] == 64 and SHAPES["grid_64"] == 128 and SHAPES["tie_pair"] == 256
    want = check("heavy_64", (45, 37), "parts", RenderOptions.no_flags)
    hit = want.part_ids >= 0
    print("heavy_64: %d pixels hit, %d parts seen" % (hit.sum(), len(numpy.unique(want.part_ids[hit]))))
    assert len(numpy.unique(want.part_ids[hit])) == 64
    check("heavy_64", (45, 37), "parts", RenderOptions.false_color)
    check("heavy_64", (45, 37), "parts", RenderOptions.zebra)


# ---- explicit colours, a placed assembly ---------------------------------------------------------------------------------
def test_explicit_colours_and_a_placed_assembly(hip):
    hues = [(0.0, 1.0, 0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.6, 0.9), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.25, 1.0, 0.0),
            (0.9, 0.1, 0.7)]
    want = check("gear_train", (80, 60), hues, RenderOptions.no_flags)
    assert len(numpy.unique(want.part_ids)) == 9                      # every part, and the background
    check("gear_train", (80, 60), {"planet": (0.0, 0.2, 1.0), "pin": (1.0, 0.0, 0.5)}, RenderOptions.no_flags)
    assert scenes.assembly("placed_gear_train").transform != scenes.assembly("gear_train").transform
    for options in OPTIONS:
        check("placed_gear_train", (80, 60), "parts", options)
    check("placed_gear_train", (80, 60), hues, RenderOptions.no_flags)
