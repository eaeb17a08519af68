"""The section of an assembly (codecad_amd/section.py), the parts that need no device: planes, the lattice, windows and
top tiles, the position formula, the colouring, the C ABI and the ISA of its kernels -- and the REFERENCE SECTION that
test_gpu_section.py holds the device to, with the scenarios that file runs, each shown here to contain what it is for.

The reference: every instance's tape evaluated by the oracle at the float32 sample positions (`sample_positions`, the
formula of the module's docstring in NumPy float32), then the map rules: inside = w < 0 strictly, part_ids the lowest
index inside, inside_count their number, distance the minimum (numpy.fmin: numbers before NaNs, like the hardware's
minimum), nearest the lowest index that attains it.
"""
import collections
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, nodes, rendering, _instance_cells
from codecad_amd import section as section_function
from codecad_amd.section import Plane, Section, lattice, windows, top_tiles, sample_positions, radius
from codecad_amd.rendering import assembly_section, assembly_picture
from codecad_amd.hip_util import _lib
import oracle

from test_gpu_interference import _plate_and_shaft, _gear_train, _random_assembly
from test_gpu_assembly_picture import _grid
from test_instance_cells_reference_host import far_translation
import heavy_instances
import cells_abi


# ---- the reference ----------------------------------------------------------------------------------------------------

Reference = collections.namedtuple("Reference", "instances corner step dims w part_ids inside_count distance nearest acc")


def maps_of(w):
    """(part_ids, inside_count, distance, nearest) of the distances w[k, j, i] of every instance at every sample."""
    inside = w < 0
    count = inside.sum(axis=0)
    part_ids = numpy.where(count > 0, inside.argmax(axis=0), -1).astype(numpy.int32)
    least = numpy.fmin.reduce(w, axis=0)
    nearest = (w == least).argmax(axis=0).astype(numpy.int32)       # (all of them NaN: the first)
    return part_ids, count.astype(numpy.uint8), least.astype(numpy.float32), nearest


def accumulators_of(w):
    """{(i, j): (count, index sums (i, j), index box)} over the samples inside i (i == j) and inside both (i < j)."""
    inside = w < 0
    out = {}
    for i in range(len(w)):
        for j in range(i, len(w)):
            at = numpy.argwhere(inside[i] & inside[j])[:, ::-1]       # (index along u, along v)
            if len(at):
                out[(i, j)] = (len(at), tuple(int(v) for v in at.sum(axis=0)),
                               (tuple(int(v) for v in at.min(axis=0)), tuple(int(v) for v in at.max(axis=0))))
    return out


def reference_section(asm, plane, resolution):
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    points = sample_positions(plane, corner, step, numpy.arange(dims[0]), numpy.arange(dims[1]))
    assert points.dtype == numpy.float32 and points.shape == (dims[1], dims[0], 3)
    w = numpy.zeros((len(instances), int(dims[1]), int(dims[0])), dtype=numpy.float32)
    for k, inst in enumerate(instances):
        w[k] = oracle.evaluate_points(nodes.make_program(inst.shape()), points.reshape(-1, 3))[:, 3].reshape(w.shape[1:])
    if not len(instances):
        empty = numpy.full((1, 1), -1, numpy.int32)
        return Reference(instances, corner, step, dims, w, empty, numpy.zeros((1, 1), numpy.uint8),
                         numpy.full((1, 1), numpy.inf, numpy.float32), empty, {})
    return Reference(instances, corner, step, dims, w, *maps_of(w), accumulators_of(w))


def device_accumulators(cut):
    return {(c.i, c.j): (c.count, c.index_sums, c.index_box) for c in cut.parts + cut.overlaps}


# ---- the scenarios of test_gpu_section.py -----------------------------------------------------------------------------

def two_boxes():
    a = shapes.box(2, 2, 2).make_part("a")
    b = shapes.box(2, 1, 3).make_part("b")
    return cc.assembly("boxes", [a, b.translated(1.5, 0.25, -0.5)])


def boxes_and_ball():
    ball = shapes.sphere(0.8).make_part("ball")
    return cc.assembly("three", list(two_boxes()) + [ball.translated(0.5, 0.5, 0.2)])


def coincident():
    ball = shapes.sphere(1).make_part("ball")
    return cc.assembly("twice", [ball.translated_x(0.3), ball.translated_x(0.3), shapes.box(1, 1, 1).make_part("block").translated_x(1.2)])


def grid_64_with_hidden():
    shown = list(_grid(64))
    listed = []
    for k, inst in enumerate(shown):
        listed.append(inst)
        if k % 5 == 0:
            listed.append(inst.translated_x(0.2).hidden())
    return cc.assembly("grid", listed)


def bar(nu, nv, step):
    """A box that gives a section of nu x nv samples on Plane.xy at `step` (a power of two: the sizes are exact)."""
    return cc.assembly("bar", [shapes.box(nu * step, nv * step, 1).make_part("bar")])


def far_assembly(resolution):
    d = far_translation(resolution)
    return boxes_and_ball().rotated((1, 2, 3), 25).translated(d, -d, d)


def centre_of(asm):
    box = asm.shape().bounding_box()
    return tuple((a + b) / 2 for a, b in zip(tuple(box.a), tuple(box.b)))


RANDOM = [(1, 4, False), (2, 9, False), (4, 6, True), (5, 12, True)]


def random_case(seed, k, blended, kind):
    """(assembly, plane, resolution): a named plane and an oblique one through the centre, one that misses every part"""
    asm = _random_assembly(seed, k, blended)
    box = asm.shape().bounding_box()
    resolution = max(box.size()) / 90
    c = centre_of(asm)
    plane = {"named": Plane.xz(c[1]), "oblique": Plane(c, (1, -2, 3), (3, 1, 0.5)),
             "missing": Plane.xy(box.b[2] + 3 * resolution)}[kind]
    return asm, plane, resolution


FAR_RESOLUTION = 0.05
# name -> (assembly, plane, resolution)
SCENARIOS = {
    "two_boxes": lambda: (two_boxes(), Plane.xy(0.03125), 0.0625),
    "shaft_tight": lambda: (_plate_and_shaft(1.6), Plane.xy(0.01), 0.05),
    "shaft_clear": lambda: (_plate_and_shaft(1.0), Plane.xy(0.01), 0.05),
    "gears_mid": lambda: (_gear_train(), Plane.xy(0.05), 0.25),
    "gears_oblique": lambda: (_gear_train(), Plane((0, 0, 1), (1, 2, 3)), 0.25),
    "grid_64": lambda: (grid_64_with_hidden(), Plane.xz(0.6), 0.125),
    "one_sample": lambda: (bar(1, 1, 0.125), Plane.xy(0.1), 0.125),
    "nine_by_65": lambda: (bar(9, 65, 0.125), Plane.xy(0.1), 0.125),
    "coincident": lambda: (coincident(), Plane.xy(0.02), 0.05),
    "far": lambda: (far_assembly(FAR_RESOLUTION), Plane(centre_of(far_assembly(FAR_RESOLUTION)), (1, 1, 2)), FAR_RESOLUTION),
}
for _seed, _k, _blended in RANDOM:
    for _kind in ("named", "oblique", "missing"):
        SCENARIOS["random_%d_%s" % (_seed, _kind)] = functools.partial(random_case, _seed, _k, _blended, _kind)
SCENARIOS.update(heavy_instances.plane_scenarios())      # parts with wide register files among light ones


@functools.lru_cache(maxsize=None)
def scenario(name):
    """(assembly, plane, resolution, its reference section)"""
    asm, plane, resolution = SCENARIOS[name]()
    return asm, plane, resolution, reference_section(asm, plane, resolution)


def empty_tiles(ref):
    """How many 8 x 8 tiles of the lattice hold no sample inside any instance."""
    n = 0
    for j in range(0, ref.inside_count.shape[0], 8):
        for i in range(0, ref.inside_count.shape[1], 8):
            n += not ref.inside_count[j:j + 8, i:i + 8].any()
    return n


# ---- planes -----------------------------------------------------------------------------------------------------------

def test_exports():
    assert cc.section is section_function and cc.Plane is Plane and cc.Section is Section
    for name in ("render_assembly_section_pixels", "render_assembly_section_pil_image", "render_assembly_section_image"):
        assert getattr(rendering, name) is getattr(assembly_section, name)


def test_named_planes_are_exact():
    for plane, u, v, n, o in ((Plane.xy(0.3), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0.3)),
                              (Plane.xz(-2), (1, 0, 0), (0, 0, 1), (0, -1, 0), (0, -2, 0)),
                              (Plane.yz(7), (0, 1, 0), (0, 0, 1), (1, 0, 0), (7, 0, 0))):
        for got, want in ((plane.u, u), (plane.v, v), (plane.normal, n), (plane.origin, o)):
            assert got.dtype == numpy.float32 and got.tobytes() == numpy.array(want, dtype=numpy.float32).tobytes()
    assert Plane.xy().origin.tolist() == [0, 0, 0]


@pytest.mark.parametrize("origin,normal,u", [((1, 2, 3), (1, 1, 1), None), ((0, 0, 0), (0, 0, 2), (1, 1, 5)), ((-4, 0.5, 9), (0.3, -2, 0.1), (0, 0, 1)),
                                             ((0, 0, 0), (1e-3, 0, 1), None)])
def test_frames_are_orthonormal(origin, normal, u):
    plane = Plane(origin, normal, u)
    f = [x.astype(numpy.float64) for x in (plane.u, plane.v, plane.normal)]
    for i in range(3):
        assert all(x.dtype == numpy.float32 for x in plane)
        for j in range(3):
            assert f[i] @ f[j] == pytest.approx(1.0 if i == j else 0.0, abs=4e-7)      # a few float32 roundings
    assert numpy.cross(f[0], f[1]) == pytest.approx(f[2], abs=4e-7)
    n = numpy.array(normal, dtype=numpy.float64)
    assert f[2] == pytest.approx(n / math.sqrt(n @ n), abs=1e-7)
    if u is not None:
        assert f[0] @ numpy.array(u, dtype=numpy.float64) > 0
    assert plane.origin.tolist() == numpy.array(origin, dtype=numpy.float32).tolist()


@pytest.mark.parametrize("origin,normal,u", [((0, 0, 0), (0, 0, 0), None), ((0, 0, 0), (0, float("nan"), 1), None), ((0, 0, 0), (float("inf"), 0, 1), None),
                                             ((0, 0, 0), (0, 0, 1), (0, 0, 3)), ((0, 0, 0), (1, 1, 0), (-2, -2, 0)), ((0, 0, 0), (0, 0, 1), (0, 0, 0)),
                                             ((float("nan"), 0, 0), (0, 0, 1), None), ((0, 0, 0), (0, 0, 1), (float("nan"), 0, 0)), ((0, 0), (0, 0, 1), None)])
def test_bad_planes(origin, normal, u):
    with pytest.raises(ValueError):
        Plane(origin, normal, u)


# ---- the lattice ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axes,make", [((0, 1), Plane.xy), ((0, 2), Plane.xz), ((1, 2), Plane.yz)])
def test_axis_planes_take_the_lattice_of_interference(axes, make):
    asm = _random_assembly(2, 9, False)
    instances = _instance_cells.visible(asm, 0.07)
    corner3, step3, dims3 = _instance_cells.lattice(instances, 0.07)
    other = 3 - sum(axes)
    plane = make(0.4)
    corner, step, dims, first, projected = lattice(instances, plane, 0.07)
    assert step == step3 and step.dtype == numpy.float32 and corner.dtype == numpy.float32
    assert dims.tolist() == dims3[list(axes)].tolist()
    assert corner[list(axes)].tobytes() == corner3[list(axes)].tobytes() and corner[other] == numpy.float32(0.4)
    # and its samples are the lattice's, bit for bit
    points = sample_positions(plane, corner, step, numpy.arange(dims[0]), numpy.arange(dims[1]))
    for k, axis in enumerate(axes):
        want = corner3[axis] + step3 * numpy.arange(dims[k]).astype(numpy.float32)
        got = points[0, :, axis] if k == 0 else points[:, 0, axis]
        assert got.tobytes() == want.tobytes()
        assert (points[..., axis] == (got[None, :] if k == 0 else got[:, None])).all()
    assert (points[..., other] == numpy.float32(0.4)).all()


@pytest.mark.parametrize("plane", [Plane((0.3, -1, 2), (1, 2, 3)), Plane((0, 0, 0), (-1, 0.2, 0.1), (0, 1, 1))])
def test_an_oblique_lattice_contains_every_projected_corner(plane):
    asm = _random_assembly(4, 6, True)
    instances = _instance_cells.visible(asm, 0.11)
    corner, step, dims, first, projected = lattice(instances, plane, 0.11)
    lo, hi = first - float(step) / 2, first + float(step) * (dims - 0.5)
    o, u, v = (x.astype(numpy.float64) for x in (plane.origin, plane.u, plane.v))
    for inst in instances:
        box = inst.shape().bounding_box()
        for c in range(8):
            p = numpy.array([(tuple(box.a), tuple(box.b))[(c >> k) & 1][k] for k in range(3)]) - o
            assert lo[0] - 1e-9 <= p @ u <= hi[0] + 1e-9 and lo[1] - 1e-9 <= p @ v <= hi[1] + 1e-9
    assert ((hi - lo) - (projected[:, :, :2].max(axis=(0, 1)) - projected[:, :, :2].min(axis=(0, 1))) < float(step) + 1e-9).all()
    assert corner.tolist() == (o + u * first[0] + v * first[1]).astype(numpy.float32).tolist()


def test_what_cannot_be_cut():
    ball = shapes.sphere(1).make_part("ball")
    pair = cc.assembly("pair", [ball, ball.translated_x(3)])
    with pytest.raises(ValueError, match="assembly"):
        cc.section(shapes.sphere(1), Plane.xy(), 0.1)
    with pytest.raises(ValueError, match="3D"):
        cc.section(cc.assembly("flat", [shapes.circle(1).make_part("disc")]), Plane.xy(), 0.1)
    with pytest.raises(ValueError, match="64"):
        cc.section(cc.assembly("crowd", [ball.translated_x(3 * i) for i in range(65)]), Plane.xy(), 0.1)
    for bad in (0, -1, float("nan"), float("inf"), "fine"):
        with pytest.raises(ValueError, match="resolution"):
            cc.section(pair, Plane.xy(), bad)
    with pytest.raises(ValueError, match="Plane"):
        cc.section(pair, ((0, 0, 0), (0, 0, 1)), 0.1)
    with pytest.raises(ValueError, match="65536"):
        cc.section(pair, Plane.xy(), 4.0 / 65537)
    with pytest.raises(ValueError, match="2\\^28"):
        cc.section(cc.assembly("wide", [ball, ball.translated(30, 30, 0)]), Plane.xy(), 32.0 / 17000)
    with pytest.raises(ValueError, match="finite"):
        cc.section(cc.assembly("endless", [ball, shapes.half_space().make_part("half")]), Plane.xy(), 0.1)


def test_an_assembly_with_nothing_to_show_gives_one_empty_sample():
    ball = shapes.sphere(1).make_part("ball")
    cut = cc.section(cc.assembly("ghosts", [ball.hidden()]), Plane.xy(), 0.1, distance=True)
    assert cut.dims == (1, 1) and cut.instances == [] and cut.parts == [] and cut.overlaps == [] and cut.runs == 0
    assert cut.part_ids.tolist() == [[-1]] and cut.inside_count.tolist() == [[0]] and cut.nearest.tolist() == [[-1]]
    assert cut.part_ids.dtype == numpy.int32 and cut.inside_count.dtype == numpy.uint8 and numpy.isposinf(cut.distance).all()
    # a plane that misses every box launches nothing either (without distance)
    miss = cc.section(cc.assembly("ball", [ball]), Plane.xy(5), 0.1)
    assert miss.dims == (10, 10) and (miss.part_ids == -1).all() and not miss.inside_count.any() and miss.runs == 0 and miss.distance is None


# ---- windows and top tiles --------------------------------------------------------------------------------------------

def _hand_made():
    a = shapes.box(4, 2, 2).make_part("a")                           # x -2..2, y -1..1, z -1..1
    b = shapes.box(2, 2, 2).make_part("b").translated(20, 9, 0.5)    # x 19..21, y 8..10, z -0.5..1.5
    clear = shapes.box(2, 2, 2).make_part("c").translated(5, 5, 1.3) # z 0.3..2.3: a step above the plane z = 0
    close = shapes.box(2, 2, 2).make_part("d").translated(5, 5, 1.2) # z 0.2..2.2: within a step
    return cc.assembly("hand", [a, b, clear, close])


def test_windows_and_top_tiles_of_hand_made_boxes():
    instances = _instance_cells.visible(_hand_made(), 0.25)
    plane = Plane.xy(0.0)
    corner, step, dims, first, projected = lattice(instances, plane, 0.25)
    assert dims.tolist() == [92, 44] and first.tolist() == [-1.875, -0.875]
    wins = windows(projected, first, step, dims)
    assert wins[0].tolist() == [[0, 0, 0], [17, 9, 0]]               # floor((-2 + 1.875 - 0.25) / 0.25) clipped, ceil((2 + 1.875 + 0.25) / 0.25)
    assert wins[1].tolist() == [[82, 34, 0], [91, 43, 0]]
    assert (wins[2, 0] > wins[2, 1]).any()                           # clear of the plane: an empty window
    assert wins[3].tolist() == [[22, 18, 0], [33, 29, 0]]
    rows = top_tiles(wins, dims, 64)
    assert rows.tolist() == [[0, 0, 0b1001, 0], [64, 0, 0b0010, 0]]
    rows = top_tiles(wins, dims, 8)
    masks = {(int(r[0]) & 0xffff, int(r[0]) >> 16): int(r[2]) for r in rows}
    assert masks[(0, 0)] == 1 and masks[(16, 8)] == 0b0001 and masks[(16, 16)] == 0b1000 and masks[(88, 40)] == 0b0010
    assert all(not m & 0b0100 for m in masks.values()) and (40, 0) not in masks
    assert all(r[1] == 0 and r[3] == 0 for r in rows)
    # with distance, or without culling, every instance is a candidate of every tile
    every = top_tiles(wins, dims, 8, everywhere=True)
    assert len(every) == 12 * 6 and (every[:, 2] == 0b1111).all()
    assert _instance_cells.top_side(numpy.array([92, 44, 1]), first=64, factor=8) == 64
    assert _instance_cells.top_side(numpy.array([65536, 65536, 1]), first=64, factor=8) == 512
    assert _instance_cells.levels(512, 1, None, 8)[0] == [512, 64] and _instance_cells.levels(8, 1, None, 8)[0] == []
    # the defaults are interference's
    assert _instance_cells.top_side(numpy.array([4000, 4000, 30])) == 64 and _instance_cells.levels(64, 1, None)[0] == [64, 16]


def test_the_radius_of_a_tile():
    r = radius(8, numpy.float32(0.25))
    assert r.dtype == numpy.float32 and r == numpy.float32(8 * 0.25 * math.sqrt(2) / 2 * (1 + 2.0 ** -10))
    # it exceeds the distance from a tile's centre to its farthest sample by more than half a step's diagonal
    assert float(r) - 7 * 0.25 * math.sqrt(2) / 2 > 0.25 * math.sqrt(2) / 2


# ---- positions --------------------------------------------------------------------------------------------------------

def test_positions_of_an_xy_plane_are_those_of_grid_eval():
    """oracle.grid_eval over a (w, h, 1) grid from the same corner evaluates at corner + step * (float)gid: a shape whose
    distance at p is a coordinate of p (a half space) reads the position back."""
    asm, plane, resolution = random_case(2, 9, False, "named")
    plane = Plane.xy(0.37)
    corner, step, dims, _, _ = lattice(_instance_cells.visible(asm, resolution), plane, resolution)
    points = sample_positions(plane, corner, step, numpy.arange(dims[0]), numpy.arange(dims[1]))
    solid = shapes.sphere(2.5).translated(0.3, -0.2, 0.5)
    tape = nodes.make_program(solid)
    dense = oracle.grid_eval(tape, corner, step, (dims[0], dims[1], 1))[:, :, 0, :]              # [x][y]
    at_points = oracle.evaluate_points(tape, points.reshape(-1, 3)).reshape(dims[1], dims[0], 4)   # [j][i]
    assert dense.transpose(1, 0, 2).tobytes() == at_points.tobytes()
    # and the formula itself, coordinate by coordinate
    i, j = 5, 3
    a, b = step * numpy.float32(i), step * numpy.float32(j)
    assert points[j, i].tolist() == [corner[0] + a, corner[1] + b, corner[2]]
    oblique = Plane((1, 2, 3), (1, 1, 1))
    want = [(corner[c] + oblique.u[c] * a) + oblique.v[c] * b for c in range(3)]
    assert all(type(x) is numpy.float32 for x in want)
    assert sample_positions(oblique, corner, step, [i], [j])[0, 0].tolist() == want
    cut = Section([], oblique, corner, step, (8, 8), None, None, None, None, [], [], 0, 0)
    assert tuple(cut.position(i, j)) == tuple(float(x) for x in want)


def test_the_reference_section_is_a_slice_of_the_dense_evaluation():
    asm = boxes_and_ball()
    resolution = 0.125
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims = _instance_cells.lattice(instances, resolution)
    k = 17
    plane = Plane.xy(float(corner[2] + step * numpy.float32(k)))
    ref = reference_section(asm, plane, resolution)
    assert ref.corner.tobytes() == numpy.array([corner[0], corner[1], plane.origin[2]], numpy.float32).tobytes()
    assert ref.dims.tolist() == dims[:2].tolist()
    dense = numpy.stack([oracle.grid_eval(nodes.make_program(i.shape()), corner, step, dims)[:, :, k, 3].T for i in instances])
    assert dense.tobytes() == ref.w.tobytes()
    part_ids, inside_count, distance, nearest = maps_of(dense)
    assert (part_ids == ref.part_ids).all() and (inside_count == ref.inside_count).all() and (nearest == ref.nearest).all()
    assert inside_count.max() == 3 and (part_ids == -1).any()


def test_map_rules_on_hand_made_distances():
    nan = float("nan")
    w = numpy.array([[[1, -1, 0.0, 2, nan, nan]], [[-2, -1, -0.0, 2, 3, nan]], [[-3, 5, 1, 1, nan, nan]]], dtype=numpy.float32)
    part_ids, inside_count, distance, nearest = maps_of(w)
    assert part_ids.tolist() == [[1, 0, -1, -1, -1, -1]] and inside_count.tolist() == [[2, 2, 0, 0, 0, 0]]
    assert distance[0, :5].tolist() == [-3, -1, 0, 1, 3] and numpy.isnan(distance[0, 5])
    assert nearest.tolist() == [[2, 0, 0, 2, 1, 0]]
    acc = accumulators_of(w)
    assert acc == {(0, 0): (1, (1, 0), ((1, 0), (1, 0))), (1, 1): (2, (1, 0), ((0, 0), (1, 0))), (2, 2): (1, (0, 0), ((0, 0), (0, 0))),
                   (0, 1): (1, (1, 0), ((1, 0), (1, 0))), (1, 2): (1, (0, 0), ((0, 0), (0, 0)))}


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def test_two_boxes_in_closed_form():
    asm, plane, resolution, ref = scenario("two_boxes")
    assert ref.dims.tolist() == [56, 32]
    assert ref.acc[(0, 0)][0] == 32 * 32 and ref.acc[(1, 1)][0] == 32 * 16 and ref.acc[(0, 1)][0] == 8 * 16
    assert ref.acc[(0, 1)][2] == ((24, 12), (31, 27))
    assert (ref.part_ids[ref.inside_count == 2] == 0).all() and (ref.inside_count == 2).sum() == 128


def test_the_fits_of_plate_and_shaft():
    tight, clear = scenario("shaft_tight")[3], scenario("shaft_clear")[3]
    both = tight.inside_count == 2
    assert both.sum() == tight.acc[(0, 1)][0] and both.sum() * 0.05 ** 2 == pytest.approx(math.pi * (0.8 ** 2 - 0.7 ** 2), rel=0.1)
    j, i = numpy.nonzero(both)                                # a ring: around the axis, nothing at it
    x, y = tight.corner[0] + 0.05 * i, tight.corner[1] + 0.05 * j
    assert (numpy.hypot(x, y) > 0.65).all() and (numpy.hypot(x, y) < 0.85).all() and len(set(numpy.sign(x))) == 2 == len(set(numpy.sign(y)))
    assert clear.inside_count.max() == 1 and (0, 1) not in clear.acc and (clear.part_ids == -1).any()


@pytest.mark.parametrize("name", ["gears_mid", "gears_oblique", "grid_64"])
def test_large_scenarios_have_empty_tiles_overlaps_and_a_rim(name):
    asm, plane, resolution, ref = scenario(name)
    assert empty_tiles(ref) >= 4 and (ref.inside_count > 0).any()
    assert ref.dims[0] % 8 or ref.dims[1] % 8                # a rim of lanes past the lattice
    assert max(ref.dims) > 64                                # more than one top tile: a level of tiles above the finest
    if name == "grid_64":
        assert len(ref.instances) == 64 and len(list(asm.all_instances())) == 77
        owners = set(ref.part_ids[ref.part_ids >= 0].tolist())
        assert min(owners) < 32 <= max(owners) and len(owners) > 30          # both words of the mask
    else:
        assert len(ref.instances) == 8 and any(i < j for i, j in ref.acc)   # the pins go through the planets


@pytest.mark.parametrize("seed,k,blended", RANDOM)
def test_random_scenarios(seed, k, blended):
    named, oblique, missing = (scenario("random_%d_%s" % (seed, kind))[3] for kind in ("named", "oblique", "missing"))
    for ref in (named, oblique):
        assert len(ref.instances) == k and (ref.inside_count > 0).any() and (ref.part_ids == -1).any()
        assert numpy.isfinite(ref.w).all()
    assert not missing.inside_count.any() and (missing.distance > 0).all() and missing.acc == {}
    assert len(set(missing.nearest.ravel().tolist())) >= 2
    assert scenario("random_%d_oblique" % seed)[1].u.tolist() != [1, 0, 0]


def test_random_scenarios_have_overlaps_on_their_cuts():
    cuts = [scenario("random_%d_%s" % (seed, kind))[3] for seed, _, _ in RANDOM for kind in ("named", "oblique")]
    assert sum(ref.inside_count.max() >= 2 for ref in cuts) >= 3


def test_small_scenarios_are_all_rim():
    one, bar965 = scenario("one_sample")[3], scenario("nine_by_65")[3]
    assert one.dims.tolist() == [1, 1] and one.part_ids.tolist() == [[0]]
    assert bar965.dims.tolist() == [9, 65] and (bar965.part_ids == 0).all() and bar965.acc[(0, 0)] == (585, (9 * 4 * 65, 9 * 32 * 65), ((0, 0), (8, 64)))


def test_the_coincident_instances_tie_everywhere():
    asm, plane, resolution, ref = scenario("coincident")
    assert ref.w[0].tobytes() == ref.w[1].tobytes() and (ref.w[0] < ref.w[2]).any() and (ref.w[2] < ref.w[0]).any()
    assert set(ref.nearest.ravel().tolist()) == {0, 2} and set(ref.part_ids.ravel().tolist()) == {-1, 0, 2}
    assert ref.acc[(0, 0)] == ref.acc[(1, 1)] == ref.acc[(0, 1)]


def test_the_far_scenario_has_a_coarse_float32():
    asm, plane, resolution, ref = scenario("far")
    ulp = float(numpy.spacing(numpy.abs(ref.corner).max()))
    assert resolution / 8 <= ulp <= resolution / 4
    assert asm.transform != cc.util.Transformation.zero()      # placed by the assembly's own transform
    assert ref.inside_count.max() >= 2 and (ref.part_ids == -1).any() and len(ref.acc) >= 3


# ---- the traversal, emulated ------------------------------------------------------------------------------------------

def emulated_section(asm, plane, resolution, distance):
    """The traversal of section.py and csrc/instance_section.hip in NumPy over the oracle: the host's windows and top
    tiles, the tiles levels' rule at the children's centres, the finest tiles at their samples -> the four maps and
    the share of (sample, instance) evaluations the finest level did."""
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    wins = windows(projected, first, step, dims)
    side = _instance_cells.top_side(numpy.array([dims[0], dims[1], 1]), first=64, factor=8)
    tapes = [nodes.make_program(i.shape()) for i in instances]
    tiles = [(int(r[0]) & 0xffff, int(r[0]) >> 16, int(r[2]) | (int(r[3]) << 32)) for r in top_tiles(wins, dims, side, everywhere=distance)]

    def values(mask, points):
        ks = [k for k in range(len(instances)) if mask >> k & 1]
        return ks, numpy.stack([oracle.evaluate_points(tapes[k], points.reshape(-1, 3))[:, 3].reshape(points.shape[:2]) for k in ks])

    while side > 8:
        child = side // 8
        r, h, children = radius(child, step), numpy.float32(0.5) * numpy.float32(child - 1), []
        for x0, y0, mask in tiles:
            xs, ys = x0 + numpy.arange(8) * child, y0 + numpy.arange(8) * child
            ks, w = values(mask, sample_positions(plane, corner, step, xs.astype(numpy.float32) + h, ys.astype(numpy.float32) + h))
            bound = numpy.fmin.reduce(w, axis=0) + (r + r)
            assert bound.dtype == numpy.float32
            for j, y in enumerate(ys):
                for i, x in enumerate(xs):
                    if x >= dims[0] or y >= dims[1]:
                        continue
                    keep = 0
                    for n, k in enumerate(ks):
                        reach = distance or (x <= wins[k, 1, 0] and x + child - 1 >= wins[k, 0, 0] and
                                             y <= wins[k, 1, 1] and y + child - 1 >= wins[k, 0, 1])
                        if (reach and not w[n, j, i] >= r) or (distance and not w[n, j, i] > bound[j, i]):
                            keep |= 1 << k
                    if keep:
                        children.append((int(x), int(y), keep))
        tiles, side = children, child
    shape = (int(dims[1]), int(dims[0]))
    part_ids, inside_count = numpy.full(shape, -1, numpy.int32), numpy.zeros(shape, numpy.uint8)
    least, nearest = numpy.full(shape, numpy.inf, numpy.float32), numpy.full(shape, -1, numpy.int32)
    evaluations = 0
    for x0, y0, mask in tiles:
        xs, ys = numpy.arange(x0, min(x0 + 8, shape[1])), numpy.arange(y0, min(y0 + 8, shape[0]))
        ks, w = values(mask, sample_positions(plane, corner, step, xs, ys))
        evaluations += w.size
        ids, count, d, near = maps_of(w)
        at = (slice(y0, y0 + 8), slice(x0, x0 + 8))
        part_ids[at], inside_count[at] = numpy.where(ids >= 0, numpy.array(ks)[numpy.maximum(ids, 0)], -1), count
        least[at], nearest[at] = d, numpy.array(ks)[near]
    return part_ids, inside_count, least, nearest, evaluations / (shape[0] * shape[1] * len(instances))


@pytest.mark.parametrize("name", ["two_boxes", "gears_oblique", "grid_64", "nine_by_65", "coincident", "far", "random_2_oblique",
                                  "random_5_named", "random_4_missing"])
def test_the_culling_rule_loses_nothing(name):
    """What the device is asked to do, done here: windows, top tiles and the two keep rules with their slack give, on the
    scenarios of the GPU file, exactly the reference's maps -- and do cull."""
    asm, plane, resolution, ref = scenario(name)
    part_ids, inside_count, _, _, share = emulated_section(asm, plane, resolution, False)
    assert numpy.array_equal(part_ids, ref.part_ids) and numpy.array_equal(inside_count, ref.inside_count)
    part_ids, inside_count, least, nearest, share_with_distance = emulated_section(asm, plane, resolution, True)
    assert numpy.array_equal(part_ids, ref.part_ids) and numpy.array_equal(inside_count, ref.inside_count)
    assert numpy.array_equal(least, ref.distance) and numpy.array_equal(nearest, ref.nearest)
    assert share <= share_with_distance <= 1
    if name in ("gears_oblique", "grid_64", "far", "random_2_oblique", "random_5_named"):
        assert share < 0.2 and share_with_distance < 0.5


# ---- colouring --------------------------------------------------------------------------------------------------------

def test_colouring_of_synthetic_maps():
    part_ids = numpy.array([[0, 0, 1, 1], [0, 0, 1, -1], [-1, -1, -1, -1]], dtype=numpy.int32)      # [j][i], j = 0 at the bottom
    inside_count = numpy.array([[1, 2, 1, 1], [1, 1, 3, 0], [0, 0, 0, 0]], dtype=numpy.uint8)
    hues = numpy.array([[0.2, 0.4, 0.6], [1.0, 0.5, 0.0]], dtype=numpy.float32)
    flat = assembly_section.section_colors(part_ids, inside_count, hues, overlap_color=(1, 0, 0), background=(1, 1, 1), outline=False)
    assert flat.dtype == numpy.uint8 and flat.shape == (3, 4, 3)
    assert (flat[0] == 255).all()                              # v points up: the last row of the maps is the first of the image
    assert flat[2, 0].tolist() == [51, 102, 153] and flat[2, 2].tolist() == [255, 128, 0] and flat[1, 3].tolist() == [255, 255, 255]
    assert flat[2, 1].tolist() == [255, 0, 0] and flat[1, 2].tolist() == [255, 0, 0]
    lined = assembly_section.section_colors(part_ids, inside_count, hues, overlap_color=(0, 0, 1), background=(0.5, 0.5, 0.5), outline=True)
    assert lined[2, 0].tolist() == [51, 102, 153]              # all four neighbours (that exist) are the same part
    assert lined[2, 1].tolist() == [0, 0, 128] and lined[2, 2].tolist() == [128, 64, 0]       # the boundary between 0 and 1, darkened
    assert lined[0].tolist() == [[64, 64, 64]] * 3 + [[128, 128, 128]]                        # background next to a part, and not
    assert lined[1, 3].tolist() == [64, 64, 64]


def test_bad_colours_are_value_errors_before_any_launch():
    asm = two_boxes()
    for kwargs in ({"colors": "rainbow"}, {"colors": [(1, 0, 0)]}, {"overlap_color": (2, 0, 0)}, {"background": (1, 1)}, {"background": "white"}):
        with pytest.raises(ValueError):
            rendering.render_assembly_section_pixels(asm, Plane.xy(), 0.1, **kwargs)
    assert [tuple(h) for h in assembly_picture.part_colors(_instance_cells.visible(asm, 1.0), "parts")] == \
        [tuple(numpy.float32(c)) for c in assembly_picture.PALETTE[:2]]


# ---- the C ABI and the ISA --------------------------------------------------------------------------------------------

def _arguments(name):
    with open(_lib.HEADER) as f:
        proto = re.search(r"int %s\(([^;]*)\);" % name, f.read()).group(1)
    return [re.split(r"[\s*]+", re.sub(r"\[\d*\]", "", p.strip()))[-1] for p in proto.split(",")]


def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_section_tiles", "hu_section_leaf"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name]) == len(_arguments(name))
        with open(os.path.join(os.path.dirname(_lib.HEADER), "..", "INTEGRATION.md")) as f:
            assert ("int %s(" % name) in f.read()
    # the launch records first (test_hip_util_host.py holds them to the header), then the plane's frame and the check's own
    assert _lib.PROTOTYPES["hu_section_tiles"][:2] == [ctypes.POINTER(_lib.CellsLaunch), ctypes.POINTER(_lib.CellsChildren)]
    assert _lib.PROTOTYPES["hu_section_leaf"][0] == ctypes.POINTER(_lib.CellsLaunch)
    assert _arguments("hu_section_tiles") == ["launch", "children", "u", "v", "with_distance"]
    assert _arguments("hu_section_leaf") == ["launch", "u", "v", "with_distance", "part_ids_dev", "inside_count_dev", "distance_dev",
                                             "nearest_dev", "acc_dev"]
    # argument checks need no device
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    nan3 = (ctypes.c_float * 3)(0, float("nan"), 0)
    held = cells_abi.held(p, (64, 64, 1))
    NULL_RECORD = cells_abi.NULL_RECORD

    def tiles_call(u=f3, v=f3, child_side=8, thr=1.0, counter_dev=p, children_dev=p, children={}, **broken):
        listed = cells_abi.children(counter_dev=counter_dev, children_dev=children_dev, capacity=1, child_side=child_side, thr=thr, **children)
        return lib.hu_section_tiles(cells_abi.launch(**dict(held, **broken)), listed, u, v, 0)

    def leaf_call(u=f3, v=f3, with_distance=0, part_ids=p, inside_count=p, distance=None, nearest=None, acc=p, **broken):
        return lib.hu_section_leaf(cells_abi.launch(**dict(held, **broken)), u, v, with_distance, part_ids, inside_count, distance, nearest, acc)

    common = [{"table_dev": None}, {"windows_dev": None}, {"parents_dev": None}, {"n_parents_dev": None}, {"evaluations_dev": None},
              NULL_RECORD, {"u": None}, {"v": None}, {"n": 0}, {"n": 65}, {"dims": (0, 8, 1)}, {"dims": (8, 65537, 1)},
              {"dims": (65536, 8192, 1)}, {"step": float("nan")}, {"step": -1.0}, {"u": nan3}, {"corner": (0, float("nan"), 0)}]
    for kwargs in common + [{"child_side": 4}, {"child_side": 12}, {"child_side": 16384}, {"thr": -1.0}, {"thr": float("nan")},
                            {"counter_dev": None}, {"children_dev": None}, {"children": NULL_RECORD}]:
        assert tiles_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    for kwargs in common + [{"part_ids": None}, {"inside_count": None}, {"acc": None}, {"with_distance": 1},
                            {"with_distance": 1, "distance": p}, {"with_distance": 1, "nearest": p}]:
        assert leaf_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    assert leaf_call(**NULL_RECORD) == -3 and b"NULL" in lib.hu_last_error()


def test_the_kernels_keep_their_records_in_scalar_registers(tmp_path):
    """What tests/test_assemblies.py asks of the interference and clearance kernels, of every instantiation of the
    section's: no scratch; no vector-memory load (arguments, the table, the windows, a tile's row, the records and
    constants of a program are wave-uniform); the interpreter's fetch groups as wide scalar loads off a pointer that was
    itself loaded from memory; and the maps leave through ordinary vector stores."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_section.hip" in builder.SOURCES and "instance_section.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_section.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_section.hip")], check=True, capture_output=True)
    text = out.read_text()
    seen = set()
    for chunk in re.split(r"\n(?=_Z\w+:\s+; @)", text):
        m = re.match(r"(_Z\w+):", chunk)
        if not m or "k_section_" not in m.group(1):
            continue
        name, flags = re.search(r"(k_section_\w+?)I((?:Lb[01]E)+)E", m.group(1)).groups()
        seen.add((name, "".join(re.findall(r"Lb([01])E", flags))))
        scratch = re.search(r"; ScratchSize: (\d+)", chunk)
        assert scratch and int(scratch.group(1)) == 0, m.group(1)
        body = chunk.split(".section")[0]
        assert not re.search(r"\t(flat|global|buffer|scratch)_load", body), m.group(1)
        assert not re.search(r"\tscratch_", body), m.group(1)
        loaded = set(re.findall(r"\ts_load_dwordx[24] s\[(\d+):\d+\]", body))
        wide = collections.Counter(re.findall(r"\ts_load_dwordx(?:8|16) s\[\d+:\d+\], s\[(\d+):\d+\]", body))
        assert any(n >= 2 and base in loaded for base, n in wide.items()), m.group(1)
        stores = set(re.findall(r"\t((?:flat|global|buffer)_(?:store|atomic)\w*)", body))
        assert stores and all(s.startswith("global_") for s in stores), (m.group(1), stores)
        if name == "k_section_leaf":
            assert {"global_store_dword", "global_store_byte"} <= stores
    assert seen == {(k, a + b) for k in ("k_section_tiles", "k_section_leaf") for a in "01" for b in "01"}
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", text.split(".amdgpu_metadata")[1])) >= 8
