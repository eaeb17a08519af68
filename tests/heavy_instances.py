"""Parts with wide register files among light ones, for the kernels over an assembly's cells (csrc/instance_cells.hpp
cells_launch): the scenes of test_cells_workgroup_shapes_host.py and test_gpu_cells_workgroup_shapes.py, the slot counts
of their programs and the workgroup a kernel lands on.  Nothing here touches a device.

`knot(level, r, axes)` generalises assembly_picture_scenes.knot(): a balanced tree of unions over 2**level spheres, every
level made symmetrical in each axis of `axes`.  Slots are counted from the library's own listing (hu_tape_listing), the
full program's float4 slots and the distance-only program's point and result slots.  Along x alone a level adds two
float4 slots to the full program: 9 at level 4, 13 at level 6 (208 B per lane), 15 at level 7.  The plain knot (r = -1)
keeps distance-only programs of 2 * level point slots and `level` result slots: 12 and 6 at level 6, 216 B per lane, the
lowest level above 192 B (level 5 has 10 and 5, 180 B).

A PART WITH 25 SLOTS exists within 5000 tape floats.  Tried, the rounded knot with every level symmetrical in: x and y
(3 slots a level: 19 at level 6, 3292 floats); x, y and z (4 a level: 21 at level 5, 25 at level 6, 4300 floats); one
axis per level in turn (2 a level, 13 at level 6); two axes per level in turn (19 at level 6).  KNOT25 is knot(6, 0.1,
"xyz"): 400 B per lane, 64 lanes in every kernel.
"""
import ctypes
import functools
import re

import numpy

import codecad_amd as cc
from codecad_amd import shapes, nodes, _instance_cells
from codecad_amd.hip_util import _lib

import assembly_picture_scenes as picture_scenes


# ---- the parts -----------------------------------------------------------------------------------------------------------
def knot(level, r, axes="x", leaf=0.9):
    """A balanced tree of unions (rounded by `r`; r = -1: plain) `level` levels deep over 2**level spheres of diameter
    `leaf`, every level's union made symmetrical in each axis of `axes`: a level keeps its left operand's result and its
    mirrored points while the right operand is evaluated."""
    def tree(k):
        if k == 0:
            return shapes.sphere(leaf)
        h = 0.25 * 2 ** (k - 1)
        a = tree(k - 1).rotated((1, 2, k), 10 * k).translated(h, 0.05 * k, 0)
        b = tree(k - 1).rotated((k, 1, 2), -7 * k).translated(h + 0.3, 0, 0.3 * k)
        out = shapes.union([a, b], r=r)
        for axis in axes:
            out = getattr(out, "symmetrical_" + axis)()
        return out
    return tree(level)


LEAF = 6.0                  # fat leaves: at the scenes' steps every sphere of a heavy part holds samples


def rounded_knot(scale=0.08):
    """13 float4 slots: 208 B per lane, above the 192 B at which a workgroup drops to 128 lanes."""
    return knot(6, 0.1, leaf=LEAF).scaled(scale)


def plain_knot(scale=0.08):
    """distance-only: 12 point slots and 6 result slots, 216 B per lane."""
    return knot(6, -1, leaf=LEAF).scaled(scale)


def knot25(scale=0.08):
    """25 float4 slots: 400 B per lane, above the 384 B at which a workgroup drops to 64 lanes."""
    return knot(6, 0.1, "xyz", leaf=LEAF).scaled(scale)


HEAVY = {"rounded": rounded_knot, "plain": plain_knot, "knot25": knot25}


# ---- slots ---------------------------------------------------------------------------------------------------------------
def listing(tape, which):
    """The library's listing of a tape's program after renaming: `which` 0 the full program, 1 the distance-only one."""
    lib = _lib.load()
    t = numpy.ascontiguousarray(tape, dtype=numpy.float32)
    p = t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    needed = ctypes.c_size_t(0)
    assert lib.hu_tape_listing(p, t.size, which, None, 0, ctypes.byref(needed)) == 0, lib.hu_last_error()
    buf = ctypes.create_string_buffer(needed.value)
    assert lib.hu_tape_listing(p, t.size, which, buf, needed.value, ctypes.byref(needed)) == 0
    return buf.value.decode()


def slots(tape):
    """(float4 slots of the full program, point slots and result slots of the distance-only program or None when the
    tape has none): slots are packed from 0, so the highest one stored to is the last."""
    def highest(pattern, text):
        return max([-1] + [int(k) for k in re.findall(pattern, text)]) + 1

    full, plain = listing(tape, 0), listing(tape, 1)
    return highest(r"store (\d+)\b(?!r)", full), (highest(r"store (\d+)\b(?!r)", plain), highest(r"store (\d+)r", plain)) if plain else None


@functools.lru_cache(maxsize=None)
def _slots_of_part(data):
    return slots(nodes.make_program(data))


def table_figures(instances):
    """(distance_only, lane_bytes) as hu_instance_table reports them for the checks over `instances`: every instance's
    distance-only program when all have one, the largest instance's slots for all."""
    counted = [_slots_of_part(i.part.data) for i in instances]       # (a placement changes no slot)
    if all(c[1] is not None for c in counted):
        return 1, 16 * max(c[1][0] for c in counted) + 4 * max(c[1][1] for c in counted)
    return 0, 16 * max(c[0] for c in counted)


# ---- the workgroup of a kernel -------------------------------------------------------------------------------------------
MAX_LDS = 160 * 1024


def cells_lanes(lane_bytes, extra_per_lane=0):
    """The rule of host.hpp hu_workgroup for cells_launch, restated: the largest of 256, 128, 64 lanes that keeps
    (lane_bytes + extra_per_lane) * lanes within 48 KiB, else 64."""
    per_lane = lane_bytes + extra_per_lane
    for lanes in (256, 128):
        if per_lane * lanes <= 48 * 1024:
            return lanes
    return 64


def cells_lds(lane_bytes, extra_per_lane=0):
    """The dynamic LDS of that workgroup: its lanes' bytes and 128 B of scratch; ValueError above 160 KiB."""
    lds = (lane_bytes + extra_per_lane) * cells_lanes(lane_bytes, extra_per_lane) + 128
    if lds > MAX_LDS:
        raise ValueError("more than 160 KiB")
    return lds


def kernel_extras(n):
    """{kernel: what it keeps per lane after the register file}, for a table of `n` instances."""
    return {
        "interference cells": 0, "interference leaf": 0, "clearance cells": 0, "clearance leaf": 4 * n, "clearance witness": 4 * n,
        "section tiles": 0, "section tiles with distance": 4 * n, "section leaf": 0, "section leaf with distance": 0,
        "outline tiles": 0, "outline leaf": 8, "layer tiles": 0, "layer leaf": 8, "mesh cells": 0, "mesh leaf": 8,
        "mass cells": 0, "mass leaf": 0, "voxel cells": 0, "voxel leaf": 0,
        "separation cells": 4 * n, "separation leaf": 4 * n, "separation witness": 4 * n,
    }


REGIMES = ["128 lanes", "64 lanes", "64 lanes above 64 KiB", "the largest LDS"]


def regimes_of(lane_bytes, extra_per_lane=0):
    """The regimes of REGIMES that a larger `lane_bytes` can still take a kernel to, from the rule: the ones its unpadded
    workgroup is not in already (256 lanes reach all four; 128 lanes, as solids64's separation has them, the last three)."""
    lanes, per_lane = cells_lanes(lane_bytes, extra_per_lane), lane_bytes + extra_per_lane
    return [regime for regime, there in zip(REGIMES, (lanes == 256, lanes > 64, per_lane * 64 + 128 <= 64 * 1024, True)) if there]


def lanes_table(instances):
    """{kernel: lanes} of the checks over `instances`."""
    lane_bytes = table_figures(instances)[1]
    return {kernel: cells_lanes(lane_bytes, extra) for kernel, extra in kernel_extras(len(instances)).items()}


# ---- the scenes ----------------------------------------------------------------------------------------------------------
def pair(kind):
    """A heavy part at index 1 of four, among light ones: it overlaps a block (0) and a ball (2), each centred deep inside
    one of its lobes; a bead (3) lies 0.2 outside it, within the gap and not overlapping (the places were read off the
    distance fields of all three heavy parts, which share them)."""
    heavy = HEAVY[kind]().make_part("knot")
    return cc.assembly("heavy_pair", [
        shapes.box(0.9, 0.8, 0.7).make_part("block").translated(1.1, 0.5, -0.2),
        heavy.rotated((1, 2, 3), 20),
        shapes.sphere(0.9).make_part("ball").translated(-1.2, 0.3, 0.5),
        shapes.sphere(0.4).make_part("bead").translated(0.0, -1.05, 0.1),
    ])


def grid_64(kind):
    """The grid of 64 solids of the picture and outline scenes with every eighth one a heavy part, at the solid's place
    and two and a half times the size of a pair's: its lobes reach the solids beside it and the heavy parts of the rows
    before and after it, and eight wavefronts of different workgroups run a heavy instance beside light ones."""
    heavy = HEAVY[kind](0.2).make_part("knot")
    solids = list(picture_scenes.SCENES["grid_64"]().all_instances())
    return cc.assembly("heavy_64", [heavy.translated(2.5 * (i % 8), 0.3 * (i % 5), 2.5 * (i // 8)) if i % 8 == 3 else solid
                                    for i, solid in enumerate(solids)])


PAIR_RESOLUTION = 0.25      # a lattice of at most 40 samples a side
PAIR_GAP = 0.5
GRID_RESOLUTION = 0.625     # a lattice of 31 x 23 x 48 samples, a section of 31 x 48
GRID_GAP = 1.25
HEAVY_INDEX = {"heavy_pair": [1], "heavy_plain": [1], "heavy_pair25": [1], "heavy_64": list(range(3, 64, 8))}

# name -> (assembly, resolution, a gap with near pairs)
SCENES = {
    "heavy_pair": lambda: (pair("rounded"), PAIR_RESOLUTION, PAIR_GAP),
    "heavy_plain": lambda: (pair("plain"), PAIR_RESOLUTION, PAIR_GAP),
    "heavy_pair25": lambda: (pair("knot25"), PAIR_RESOLUTION, PAIR_GAP),
    "heavy_64": lambda: (grid_64("rounded"), GRID_RESOLUTION, GRID_GAP),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def instances_of(name):
    asm, resolution, gap = scene(name)
    return _instance_cells.visible(asm, resolution)


# ---- the references, each family's own, computed once per session ----------------------------------------------------------
# (the family modules are imported where they are used: some of them import this one's neighbours)

def plane_of(name):
    """The plane of a scene's cut: through the block, the ball and the bead of a pair, through the grid's middle row."""
    from codecad_amd.section import Plane
    return Plane.xz(0.6) if name == "heavy_64" else Plane.xy(0.1)


def layers_of(name):
    """(base plane, three heights) of a scene's stack."""
    from codecad_amd.section import Plane
    return (Plane.xz(0), [0.0, 0.6, 1.2]) if name == "heavy_64" else (Plane.xy(0), [-0.15, 0.1, 0.35])


def without_heavy(name):
    """The scene with a ball in the place of every heavy part (what the lane table must fail on)."""
    asm, resolution, gap = scene(name)
    ball = shapes.sphere(1.0).make_part("ball")
    return cc.assembly("light", [ball._transformed(i.transform) if i.name == "knot" else i for i in asm.all_instances()])


def without_heavy_references(name):
    """What each family's reference gives for the scene without its heavy parts, by the family's own functions."""
    import assembly_voxels_scenes as avs
    import test_section_host as tsh
    import test_section_outlines_host as tso
    import layer_outlines_scenes as los
    import assembly_meshes_scenes as ams
    import assembly_mass_scenes as mass
    from test_instance_cells_reference_host import lattice_of, as_report
    from test_gpu_clearance import dense_near
    asm, (_, resolution, gap) = without_heavy(name), scene(name)
    instances, corner, step, dims, t = lattice_of(asm, resolution, gap)
    visible = _instance_cells.visible(asm, resolution)
    lattice = _instance_cells.checked_lattice(visible, resolution)
    plane, heights = layers_of(name)
    return {"near": dense_near(as_report(instances, corner, step, dims, gap)),
            "section": tsh.reference_section(asm, plane_of(name), resolution).acc,
            "outlines": tso.reference_outlines(asm, plane_of(name), resolution).counts.tolist(),
            "layers": los.reference_layers(asm, plane, resolution, heights).layer_counts.tolist(),
            "meshes": ams.reference_meshes(visible, *lattice).counts.tolist(),
            "mass": mass.reference_mass(visible, *lattice, True).sums,
            "separation": separation_of(visible, lattice[2], lattice[1], mass.dense_fields(visible, *lattice)),
            "voxels": avs.reference_voxels(visible, *lattice, True).counts}


@functools.lru_cache(maxsize=None)
def pairs_reference(name, gap):
    """(dense_pairs, dense_near) dicts of the scene at `gap` (dense_pairs only at gap 0)."""
    from test_instance_cells_reference_host import lattice_of, as_report
    from test_gpu_interference import dense_pairs
    from test_gpu_clearance import dense_near
    asm, resolution, _ = scene(name)
    instances, corner, step, dims, t = lattice_of(asm, resolution, gap)
    report = as_report(instances, corner, step, dims, gap)
    return (dense_pairs(report) if gap == 0 else None), dense_near(report), dims


def section_reference(name):
    import test_section_host as tsh
    return tsh.scenario(name)[3]


def outlines_reference(name):
    import test_section_outlines_host as tso
    return tso.scenario(name)[3]


def outlines_traversal(name, cull=True):
    import test_section_outlines_host as tso
    return tso.traversal(name, cull)


def layers_reference(name):
    import layer_outlines_scenes as los
    return los.scenario(name)[4]


def layers_traversal(name, cull=True):
    import layer_outlines_scenes as los
    return los.traversal(name, cull)


def lattice3(name):
    import assembly_mass_scenes as mass
    return mass.scene(name)[2:]


def meshes_reference(name):
    import assembly_meshes_scenes as ams
    return ams.reference(name)


def meshes_traversal(name):
    import assembly_meshes_scenes as ams
    return ams.traversal(name)


def mass_reference(name, retire=True):
    import assembly_mass_scenes as mass
    return mass.reference(name, retire)


def separation_of(instances, dims, step, w):
    """(Dense, Traversal) of separation_scenes.py over the dense fields `w`."""
    import separation_scenes as sep
    return sep.dense(w), sep.traverse(sep.field_values(w), len(instances), dims, step)


@functools.lru_cache(maxsize=None)
def separation_reference(name):
    """(Dense, Traversal) of a scene, over the fields its mass reference evaluates."""
    import assembly_mass_scenes as mass
    instances, corner, step, dims = lattice3(name)
    return separation_of(instances, dims, step, mass._fields(name))


def voxels_reference(name, retire=True):
    """The Reference of assembly_voxels_scenes.py for a scene, which registers the heavy scenes itself (through the mass
    scenes' table) and caches every reference per session: nothing is kept here."""
    import assembly_voxels_scenes as avs
    return avs.reference(name, retire)


# ---- what each family's own scenario table takes (the family modules register these entries themselves) --------------------

def mass_scenes(Scene):
    return {name: Scene(functools.partial(lambda n: scene(n)[0], name), scene(name)[1]) for name in SCENES}


def plane_scenarios():
    """name -> () -> (assembly, plane, resolution): test_section_host.py, test_section_outlines_host.py"""
    return {name: functools.partial(lambda n: (scene(n)[0], plane_of(n), scene(n)[1]), name) for name in SCENES}


def layer_scenarios():
    """name -> () -> (assembly, base plane, resolution, three heights): layer_outlines_scenes.py"""
    return {name: functools.partial(lambda n: (scene(n)[0], layers_of(n)[0], scene(n)[1], layers_of(n)[1]), name) for name in SCENES}


def pair_scenarios(Scenario):
    """name -> Scenario of test_instance_cells_reference_host.py: the gaps 0 and the scene's, a top side of 16, dense."""
    return {name: Scenario(functools.partial(lambda n, gap: scene(n)[0], name), scene(name)[1], (0.0, scene(name)[2]), 16, False)
            for name in SCENES}
