"""Scenes and the CPU reference of the exact tests of an assembly's picture (test_assembly_picture_reference_host.py,
test_gpu_assembly_picture_exact.py): the five scenes of test_gpu_assembly_picture.py, exact ties, a part with a large
register file 64 times over, and the workgroup shape a scene lands on.  Nothing here touches a device."""
import collections
import ctypes
import re

import numpy

import codecad_amd as cc
from codecad_amd import shapes, nodes
from codecad_amd.rendering import assembly_picture as ap
from codecad_amd.hip_util import _lib
import oracle
import test_gpu_assembly_picture as loose

THREADS = 16
TIE_SIZE = (61, 45)                    # an odd width: the centre column, x = 30, has filmx == 0
TIE_COLUMN = 30
HUE_A, HUE_B, HUE_C = (1.0, 0.0, 0.25), (0.0, 0.5, 1.0), (0.5, 1.0, 0.0)


# ---- ties ----------------------------------------------------------------------------------------------------------------
def _pair(flipped):
    """Two spheres of diameter 2 at x = -0.75 and x = +0.75: on the plane x = 0 their distances are equal bit for bit
    (dx enters as dx * dx) and their directions differ in the sign of x."""
    left = shapes.sphere(2).make_part("left").translated_x(-0.75)
    right = shapes.sphere(2).make_part("right").translated_x(0.75)
    return (right, left) if flipped else (left, right)


def tie_pair(flipped=False):
    return cc.assembly("pair", list(_pair(flipped)))


def tie_six(flipped=False):
    """The pair at the visible indices 1 and 4 of six, a hidden ball that would cover both between them in the list.  The
    parts at indices 2 and 3 lie on x = 0 just above and below the lens, inside the 8 x 8 tiles of the seam: lanes of the
    seam's wavefronts come from winners 2 and 3 and evaluate those before instance 1.  Indices 0 and 5 reach x = -4.25 and
    x = +4.25: the box stays symmetric about x = 0, and so does the camera."""
    a, b = _pair(flipped)
    return cc.assembly("six", [
        shapes.box(1.5).make_part("block").translated(-3.5, 0, 0.5),
        a,
        shapes.sphere(0.6).make_part("bead").translated(0, -0.5, 1.3),
        shapes.sphere(6).make_part("cover").hidden(),
        shapes.cylinder(h=0.6, d=0.8).make_part("peg").translated(0, -0.25, -1.3),
        b,
        shapes.sphere(1).make_part("ball").translated(3.75, 0, -0.5),
    ])


def tie_triple():
    """One part three times at one placement, a hidden copy among them: every sample ties, with equal directions."""
    part = (shapes.box(2, 1, 1) + shapes.sphere(1.5).translated_x(1) - shapes.cylinder(h=4, d=0.8)).make_part("thing")
    placed = part.rotated((1, 2, 3), 35).translated(3, -1, 2)
    return cc.assembly("triple", [placed, placed.hidden(), placed, placed])


# ---- workgroup shapes ----------------------------------------------------------------------------------------------------
def knot():
    """A balanced tree of rounded unions 4 levels deep over 16 spheres, every level's union made symmetrical in x: a level
    keeps its left operand's result and its mirrored point while the right operand is evaluated, so the full program keeps
    9 float4 values live, a register file of 144 B per lane.  With 64 instances a lane needs 144 + 256 = 400 B, and
    400 B x 128 lanes is more than 48 KiB: 64 lanes."""
    def level(k):
        if k == 0:
            return shapes.sphere(0.9)
        h = 0.25 * 2 ** (k - 1)
        a = level(k - 1).rotated((1, 2, k), 10 * k).translated(h, 0.05 * k, 0)
        b = level(k - 1).rotated((k, 1, 2), -7 * k).translated(h + 0.3, 0, 0.3 * k)
        return shapes.union([a, b], r=0.1).symmetrical_x()
    return level(4).scaled(0.15)


def heavy_64():
    """The grid of 64 solids with every eighth one a knot: the register file is the largest instance's."""
    knot_part = knot().make_part("knot")
    solids = list(loose.SCENES["grid_64"]().all_instances())
    return cc.assembly("heavy", [knot_part.rotated((1, i % 3, 2), 13 * i).translated(2.5 * (i % 8), 0.3 * (i % 5), 2.5 * (i // 8))
                                 if i % 8 == 3 else solid for i, solid in enumerate(solids)])


def placed_gear_train():
    return loose.SCENES["gear_train"]().rotated((1, 2, 3), 40).translated(5, -7, 2)


SCENES = dict(loose.SCENES)
SCENES.update({
    "tie_pair": tie_pair, "tie_pair_flipped": lambda: tie_pair(True),
    "tie_six": tie_six, "tie_six_flipped": lambda: tie_six(True),
    "tie_triple": tie_triple, "heavy_64": heavy_64, "placed_gear_train": placed_gear_train,
})
_assemblies = {}


def assembly(name):
    if name not in _assemblies:
        _assemblies[name] = SCENES[name]()
    return _assemblies[name]


def n_slots(tape):
    """The float4 slots the full program of `tape` keeps live, from the library's own listing of it after renaming (no
    device): slots are packed from 0, so the highest one stored to is the last."""
    lib = _lib.load()
    t = numpy.ascontiguousarray(tape, dtype=numpy.float32)
    p = t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    needed = ctypes.c_size_t(0)
    assert lib.hu_tape_listing(p, t.size, 0, None, 0, ctypes.byref(needed)) == 0, lib.hu_last_error()
    buf = ctypes.create_string_buffer(needed.value)
    assert lib.hu_tape_listing(p, t.size, 0, buf, needed.value, ctypes.byref(needed)) == 0
    return max([-1] + [int(k) for k in re.findall(r"store (\d+)", buf.value.decode())]) + 1


def lane_bytes(asm):
    """What hu_instance_table reports for the full programs of `asm`'s visible instances: 16 B per slot of the largest, one
    slot at least."""
    return 16 * max([1] + [n_slots(nodes.make_program(i.shape())) for i in ap.scene(asm, (8, 8))[0]])


def workgroup_lanes(lane_bytes, n):
    """The rule of hu_ray_caster_instances, restated: a lane's LDS is its register file and one float per instance; the
    workgroup is the largest of 256 / 128 / 64 lanes that keeps per_lane * lanes within 48 KiB."""
    per_lane = lane_bytes + 4 * n
    for lanes in (256, 128):
        if per_lane * lanes <= 48 * 1024:
            return lanes
    return 64


# ---- the reference -------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "pixels part_ids depth tied")
_references = {}


def _key(colors):
    return tuple(sorted(colors.items())) if isinstance(colors, dict) else tuple(map(tuple, colors)) if isinstance(colors, list) else colors


def reference(name, size, colors="parts", options=0):
    """The oracle's picture of scene `name` in the layout of an AssemblyPicture (row, column), rendered once per session."""
    key = (name, tuple(size), _key(colors), int(options))
    if key not in _references:
        instances, hues, camera, a = ap.scene(assembly(name), size, None, colors)
        tapes = [nodes.make_program(i.shape()) for i in instances]
        f = numpy.float32
        got = oracle.ray_caster_instances(tapes, hues, list(a["origin"]), list(a["forward"]), list(a["up"]), list(a["right"]),
                                          f(a["pixel_tolerance"]), f(a["box_radius"]), f(a["min_distance"]), f(a["max_distance"]),
                                          f(a["floor_z"]), int(options), size, threads=THREADS)
        _references[key] = Reference(got.pixels.transpose((1, 0, 2)), got.part_ids.T, got.depth.T, got.tied.T)
        for array in _references[key]:
            array.setflags(write=False)
    return _references[key]
