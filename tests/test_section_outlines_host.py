"""The outlines of an assembly's section (codecad_amd/section_outlines.py), the parts that need no device: the REFERENCE
OUTLINES that test_gpu_section_outlines.py holds the device to, the reference traversal, `stitch` on synthetic segments,
the raster property of the stitched loops, the scenarios of the GPU file (each shown here to contain what it is for), the
C ABI, the ISA of the kernels and the SVG writer.

The reference: every instance's tape evaluated by the oracle at the float32 positions of the ringed samples
(`section.sample_positions` at the indices -1 .. dims), inside = w < 0, an edge crossed when exactly one end is inside,
t = w_p / (w_p - w_q) in NumPy float32 (0.5 for a NaN).  The segments of a square are DERIVED, not tabulated: the crossed
edges are paired (in a saddle, each inside corner's two edges) and each pair is directed by the sign of a cross product
against an inside corner, so that kernel and reference share no case table.
"""
import collections
import ctypes
import functools
import math
import os
import re
import subprocess
import sys
import xml.etree.ElementTree

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, nodes, rendering, _instance_cells
from codecad_amd.section import Plane, lattice, windows, top_tiles, sample_positions
from codecad_amd.section_outlines import SEGMENT, Outlines, Loop, stitch, sort_segments, square_windows, radius
from codecad_amd.rendering import assembly_picture, assembly_section_svg
from codecad_amd.hip_util import _lib
import oracle

so = sys.modules["codecad_amd.section_outlines"]       # (the package's attribute of that name is the function)

import heavy_instances
import cells_abi
import test_section_host as tsh
from test_gpu_interference import _gear_train


# ---- the reference ----------------------------------------------------------------------------------------------------

Reference = collections.namedtuple("Reference", "instances corner step dims first w segments counts")

# edge e of the unit square: its lower-index corner p and higher-index corner q; corner c sits at (c & 1, c >> 1)
EDGE_ENDS = {0: (0, 1), 1: (1, 3), 2: (2, 3), 3: (0, 2)}
CORNER_XY = {c: (c & 1, c >> 1) for c in range(4)}


def square_segments(inside):
    """[(e_from, e_to)] of a square from its four inside bits (corner c at (c & 1, c >> 1)), derived: the crossed edges
    are paired -- two of them as they are; four (a saddle) per inside corner, the two edges that meet in it -- and a
    pair is directed so that an inside corner lies on its left."""
    crossed = [e for e, (p, q) in EDGE_ENDS.items() if inside[p] != inside[q]]
    if not crossed:
        return []
    if len(crossed) == 2:
        pairs = [(crossed, [c for c in range(4) if inside[c]][0])]
    else:
        assert len(crossed) == 4
        pairs = [([e for e, ends in EDGE_ENDS.items() if c in ends], c) for c in range(4) if inside[c]]
    out = []
    for (e, f), c in pairs:
        mid = lambda g: tuple((CORNER_XY[EDGE_ENDS[g][0]][k] + CORNER_XY[EDGE_ENDS[g][1]][k]) / 2 for k in range(2))
        p, q = mid(e), mid(f)
        cross = (q[0] - p[0]) * (CORNER_XY[c][1] - p[1]) - (q[1] - p[1]) * (CORNER_XY[c][0] - p[0])
        assert cross != 0
        out.append((e, f) if cross > 0 else (f, e))          # the inside corner on the left of from -> to
    return out


def crossing(wp, wq):
    with numpy.errstate(all="ignore"):
        t = numpy.float32(wp) / (numpy.float32(wp) - numpy.float32(wq))
    assert t.dtype == numpy.float32
    return numpy.float32(0.5) if numpy.isnan(t) else t


def segments_of(w):
    """The sorted SEGMENT records of the distances w[k, t, s] at the ringed samples (shifted indices s along u, t along v)."""
    records = []
    for k in range(len(w)):
        inside = w[k] < 0
        differs = numpy.zeros((w.shape[1] - 1, w.shape[2] - 1), dtype=bool)
        for dj, di in ((0, 1), (1, 0), (1, 1)):
            differs |= inside[:-1, :-1] != inside[dj:inside.shape[0] - 1 + dj, di:inside.shape[1] - 1 + di]
        for b, a in numpy.argwhere(differs):
            corner_w = [w[k, b + (c >> 1), a + (c & 1)] for c in range(4)]
            t = {e: crossing(corner_w[p], corner_w[q]) for e, (p, q) in EDGE_ENDS.items()}
            for e, f in square_segments([bool(v < 0) for v in corner_w]):
                records.append((a, b, k, e, f, 0, t[e], t[f]))
    return sort_segments(numpy.array(records, dtype=SEGMENT))


def ringed_values(instances, plane, corner, step, dims):
    points = sample_positions(plane, corner, step, numpy.arange(-1, dims[0] + 1), numpy.arange(-1, dims[1] + 1))
    assert points.dtype == numpy.float32 and points.shape == (dims[1] + 2, dims[0] + 2, 3)
    w = numpy.zeros((len(instances), int(dims[1]) + 2, int(dims[0]) + 2), dtype=numpy.float32)
    for k, inst in enumerate(instances):
        w[k] = oracle.evaluate_points(nodes.make_program(inst.shape()), points.reshape(-1, 3))[:, 3].reshape(w.shape[1:])
    return w


def reference_outlines(asm, plane, resolution):
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    w = ringed_values(instances, plane, corner, step, dims)
    segments = segments_of(w)
    counts = numpy.bincount(segments["k"], minlength=len(instances)).astype(numpy.int64)
    return Reference(instances, corner, step, dims, first, w, segments, counts)


Traversal = collections.namedtuple("Traversal", "rows evaluations dropped_outside dropped_inside")


def reference_traversal(asm, plane, resolution, cull=True):
    """What section_outlines.py and csrc/instance_outline.hip do, in NumPy over the oracle: the windows of squares, the top
    tiles, the keep rule at the children's centres -> the rows {(a0, b0, mask)} of every level from the top one to the
    finest, the evaluations of all levels, and how many candidates a level dropped for w >= r and for w <= -r."""
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    wins = square_windows(windows(projected, first, step, dims))
    squares = numpy.array([dims[0] + 1, dims[1] + 1, 1])
    side = _instance_cells.top_side(squares, first=64, factor=8) if cull else 8
    tapes = [nodes.make_program(i.shape()) for i in instances]
    tiles = [(int(r[0]) & 0xffff, int(r[0]) >> 16, int(r[2]) | (int(r[3]) << 32)) for r in top_tiles(wins, squares[:2], side, everywhere=not cull)]
    rows, evaluations, outside, inside = [sorted(tiles)], 0, 0, 0
    if not tiles:
        return Traversal(rows, 0, 0, 0)                       # nothing is launched
    while side > 8:
        child = side // 8
        r, children = radius(child, step), []
        for a0, b0, mask in tiles:
            xs, ys = a0 + numpy.arange(8) * child, b0 + numpy.arange(8) * child
            ks = [k for k in range(len(instances)) if mask >> k & 1]
            points = sample_positions(plane, corner, step, (xs - 1 + child / 2).astype(numpy.float32), (ys - 1 + child / 2).astype(numpy.float32))
            w = numpy.stack([oracle.evaluate_points(tapes[k], points.reshape(-1, 3))[:, 3].reshape(8, 8) for k in ks])
            for j, y in enumerate(ys):
                for i, x in enumerate(xs):
                    if x >= squares[0] or y >= squares[1]:
                        continue
                    evaluations += len(ks)
                    keep = 0
                    for n, k in enumerate(ks):
                        if not (x <= wins[k, 1, 0] and x + child - 1 >= wins[k, 0, 0] and y <= wins[k, 1, 1] and y + child - 1 >= wins[k, 0, 1]):
                            continue
                        if w[n, j, i] >= r:
                            outside += 1
                        elif w[n, j, i] <= -r:
                            inside += 1
                        else:
                            keep |= 1 << k
                    if keep:
                        children.append((int(x), int(y), keep))
        tiles, side = children, child
        rows.append(sorted(tiles))
    for a0, b0, mask in tiles:      # a finest tile: the samples a0 .. a0 + 8 by b0 .. b0 + 8 that exist
        evaluations += (min(a0 + 8, squares[0]) - a0 + 1) * (min(b0 + 8, squares[1]) - b0 + 1) * bin(mask).count("1")
    return Traversal(rows, int(evaluations), outside, inside)


def segments_reached(ref, leaf_rows):
    """The reference's segments in the squares and of the candidates of the finest rows: what the traversal emits."""
    masks = {(a0, b0): mask for a0, b0, mask in leaf_rows}
    s = ref.segments
    keep = [bool(masks.get((int(a) & ~7, int(b) & ~7), 0) >> int(k) & 1) for a, b, k in zip(s["a"], s["b"], s["k"])]
    return s[numpy.array(keep, dtype=bool)] if len(s) else s


# ---- the scenarios of test_gpu_section_outlines.py --------------------------------------------------------------------

def diagonal():
    """One part of three unit boxes in a zigzag: the first two meet along the edge x = y = 0.5, the last two along
    x = 1.5, y = 0.5 -- one contact on each diagonal of a lattice square."""
    box = shapes.box(1, 1, 1)
    return cc.assembly("zigzag", [(box + box.translated(1, 1, 0) + box.translated(2, 0, 0)).make_part("zigzag")])


def speck():
    return cc.assembly("speck", [shapes.box(0.1, 0.1, 1).make_part("speck")])


def gear_train_cut():
    asm = _gear_train()
    box = asm.shape().bounding_box()
    c = tsh.centre_of(asm)
    return asm, Plane.xz(c[1]), max(box.size().x, box.size().z) / 94


def oblique_of(asm):
    return Plane(tsh.centre_of(asm), (1, -2, 3), (3, 1, 0.5))


FAR_RESOLUTION = 0.0625
# name -> (assembly, plane, resolution)
SCENARIOS = {
    "two_boxes": tsh.SCENARIOS["two_boxes"],
    "boxes_and_ball": lambda: (tsh.boxes_and_ball(), oblique_of(tsh.boxes_and_ball()), 0.0625),
    "coincident": tsh.SCENARIOS["coincident"],
    "diagonal": lambda: (diagonal(), Plane.xy(0.1), 0.25),
    "bar_64_9": lambda: (tsh.bar(64, 9, 0.125), Plane.xy(0.1), 0.125),
    "speck": lambda: (speck(), Plane.xy(0.1), 0.125),
    "grid_64": lambda: (tsh.grid_64_with_hidden(), Plane.xz(0.6), 0.25),
    "far": lambda: (tsh.far_assembly(FAR_RESOLUTION), Plane(tsh.centre_of(tsh.far_assembly(FAR_RESOLUTION)), (1, 1, 2)), FAR_RESOLUTION),
    "missing": lambda: (tsh.two_boxes(), Plane.xy(5), 0.0625),
    "random_2_named": functools.partial(tsh.random_case, 2, 9, False, "named"),
    "gear_train": gear_train_cut,
}
SCENARIOS.update(heavy_instances.plane_scenarios())      # parts with wide register files among light ones


@functools.lru_cache(maxsize=None)
def scenario(name):
    """(assembly, plane, resolution, its reference outlines)"""
    asm, plane, resolution = SCENARIOS[name]()
    return asm, plane, resolution, reference_outlines(asm, plane, resolution)


@functools.lru_cache(maxsize=None)
def traversal(name, cull=True):
    asm, plane, resolution, ref = scenario(name)
    return reference_traversal(asm, plane, resolution, cull)


def outlines_of(ref, plane):
    """The Outlines a device run must give, from the reference (evaluations and runs left 0)."""
    named = [_instance_cells.Instance(i.name, i) for i in ref.instances]
    return Outlines(named, plane, ref.corner, ref.step, tuple(int(d) for d in ref.dims), ref.segments,
                    stitch(ref.segments, len(ref.instances), ref.first, float(ref.step)), ref.counts, 0, 0)


# ---- the derivation of a square's segments ----------------------------------------------------------------------------

def test_exports():
    assert cc.section_outlines is so.section_outlines and cc.Outlines is Outlines and cc.Loop is Loop
    assert rendering.render_assembly_section_svg is assembly_section_svg.render_assembly_section_svg
    assert Outlines._fields == ("instances", "plane", "corner", "step", "dims", "segments", "loops", "counts", "evaluations", "runs")
    assert Loop._fields == ("points", "closed", "area")


def test_derived_segments_of_the_sixteen_cases():
    assert square_segments([False] * 4) == [] and square_segments([True] * 4) == []
    assert square_segments([True, False, False, False]) == [(0, 3)]          # round the corner (0, 0), counter-clockwise
    assert square_segments([False, True, True, True]) == [(3, 0)]            # and clockwise round the only outside one
    assert square_segments([True, True, False, False]) == [(1, 3)]           # material below: the boundary runs to the left
    assert square_segments([False, True, False, True]) == [(2, 0)]           # material on the right: it runs down
    assert sorted(square_segments([True, False, False, True])) == [(0, 3), (2, 1)]
    assert sorted(square_segments([False, True, True, False])) == [(1, 0), (3, 2)]
    for case in range(1, 15):
        inside = [bool(case >> c & 1) for c in range(4)]
        got = square_segments(inside)
        assert len(got) == (2 if case in (6, 9) else 1)
        for e, f in got:                            # from and to are crossed edges, and the complement runs backwards
            assert all(inside[EDGE_ENDS[g][0]] != inside[EDGE_ENDS[g][1]] for g in (e, f))
        assert sorted(square_segments([not v for v in inside])) == sorted((f, e) for e, f in got) or case in (6, 9)


def test_crossings_are_float32_and_half_for_no_number():
    assert crossing(-1.0, 3.0) == numpy.float32(0.25) and crossing(2.0, -6.0) == numpy.float32(0.25)
    assert crossing(numpy.float32(-0.1), numpy.float32(0.2)) == numpy.float32(-0.1) / (numpy.float32(-0.1) - numpy.float32(0.2))
    assert crossing(-1.0, float("nan")) == numpy.float32(0.5) and crossing(-numpy.inf, numpy.inf) == numpy.float32(0.5)
    assert crossing(-0.0, -1.0) == 0 and crossing(-1.0, 0.0) == 1        # a surface through a sample: that sample is outside


# ---- stitch on synthetic segments -------------------------------------------------------------------------------------

def field_segments(*fields):
    """The segments of hand-made fields w[t, s] (one instance each), through the reference's derivation."""
    return segments_of(numpy.array(fields, dtype=numpy.float32))


def _disc(size, centre, r):
    y, x = numpy.mgrid[:size, :size]
    return numpy.hypot(x - centre[0], y - centre[1]) - r


def test_stitch_a_disc():
    loops = stitch(field_segments(_disc(12, (5.3, 5.6), 3.2)), 1)
    assert len(loops) == 1 and len(loops[0]) == 1
    loop = loops[0][0]
    assert loop.closed and loop.area > 0 and loop.area == pytest.approx(math.pi * 3.2 ** 2, rel=0.05)
    assert loop.points.dtype == numpy.float64 and loop.points.shape[1] == 2
    # points are shifted index - 1; the loop starts at its smallest (b, a, e_from): the first of the sorted segments
    first = field_segments(_disc(12, (5.3, 5.6), 3.2))[0]
    assert tuple(loop.points[0]) == tuple(so.vertices(first["a"], first["b"], first["e_from"], first["t_from"]) - 1)


def test_stitch_a_ring_with_a_hole():
    w = numpy.maximum(_disc(16, (7.4, 7.7), 6.1), -_disc(16, (7.4, 7.7), 2.3))
    loops = stitch(field_segments(w), 1)[0]
    assert len(loops) == 2 and all(l.closed for l in loops)
    assert loops[0].area > 0 > loops[1].area                     # material counter-clockwise and first: it starts lower
    assert loops[0].area + loops[1].area == pytest.approx(math.pi * (6.1 ** 2 - 2.3 ** 2), rel=0.05)


def test_stitch_two_diagonal_squares_is_two_loops():
    for flip in (False, True):
        w = numpy.ones((4, 4), dtype=numpy.float32)
        w[1, 2 if flip else 1] = w[2, 1 if flip else 2] = -1     # two inside samples on a diagonal: one saddle between them
        segments = field_segments(w)
        assert len(segments) == 8
        saddle = segments[(segments["a"] == 1) & (segments["b"] == 1)]
        assert sorted(zip(saddle["e_from"].tolist(), saddle["e_to"].tolist())) == ([(1, 0), (3, 2)] if flip else [(0, 3), (2, 1)])
        loops = stitch(segments, 1)[0]
        assert len(loops) == 2 and all(l.closed and len(l.points) == 4 and l.area == pytest.approx(0.5) for l in loops)
        assert loops[0].points[:, 1].min() < loops[1].points[:, 1].min()      # ordered by their start keys: the lower one first


def test_stitch_a_contour_cut_by_the_rim_is_open():
    w = _disc(10, (9.2, 4.5), 3.1)                                # runs out of the lattice on the right
    segments = field_segments(w, _disc(10, (4.4, 4.6), 2.2))      # and a second instance, closed
    loops = stitch(segments, 2)
    assert len(loops[0]) == 1 and not loops[0][0].closed and len(loops[1]) == 1 and loops[1][0].closed
    cut = loops[0][0]
    assert cut.points[0, 0] == cut.points[-1, 0] == 8             # both ends on the last column of samples (shifted 9)
    assert len(cut.points) == (segments["k"] == 0).sum() + 1
    assert cut.points[0, 1] > cut.points[-1, 1]                   # the inside (to the right, off the lattice) on the left: downwards


def test_stitch_keys_and_errors():
    assert stitch(numpy.zeros(0, dtype=SEGMENT), 3) == [[], [], []]
    segments = field_segments(_disc(8, (3.5, 3.5), 2.0), _disc(8, (3.5, 3.5), 2.0))
    a, b = stitch(segments, 2)
    assert numpy.array_equal(a[0].points, b[0].points)            # the same edges, kept apart by the instance in the key
    twice = numpy.concatenate([segments[:1], segments])
    with pytest.raises(ValueError):
        stitch(twice, 2)
    shifted = stitch(segments, 2, first=(10.0, -4.0), step=0.5)
    assert numpy.array_equal(shifted[0][0].points, numpy.array([10.0, -4.0]) + 0.5 * a[0].points)
    assert shifted[0][0].area == pytest.approx(0.25 * a[0].area)


# ---- the raster property ----------------------------------------------------------------------------------------------

def even_odd_fill(loops, shape):
    """bool[t, s]: the even-odd fill of the loops (points in shifted index - 1 coordinates) at the ringed samples: the
    crossings of each loop's edges with the ray from a sample along +u, the usual half-open rule on v."""
    toggles = numpy.zeros((shape[0], shape[1] + 1), dtype=numpy.int64)
    for loop in loops:
        p = loop.points + 1.0
        q = numpy.roll(p, -1, axis=0)
        if not loop.closed:
            p, q = p[:-1], q[:-1]
        for (x1, y1), (x2, y2) in zip(p, q):
            for row in range(int(math.floor(min(y1, y2))), int(math.floor(max(y1, y2))) + 1):
                if (y1 > row) != (y2 > row):
                    x = x1 + (row - y1) * (x2 - x1) / (y2 - y1)
                    toggles[row, 0] += 1                          # every sample of the row with s < x
                    toggles[row, min(shape[1], max(0, int(math.ceil(x))))] -= 1
    return (numpy.cumsum(toggles, axis=1)[:, :shape[1]] & 1).astype(bool)


def touched_samples(segments, k, shape):
    """bool[t, s]: the samples a vertex of instance k coincides with (a t of exactly 0 or 1 on one of their edges)."""
    out = numpy.zeros(shape, dtype=bool)
    for s in segments[segments["k"] == k]:
        for e, t in ((int(s["e_from"]), s["t_from"]), (int(s["e_to"]), s["t_to"])):
            if t == 0 or t == 1:
                p = EDGE_ENDS[e][0 if t == 0 else 1]
                out[int(s["b"]) + (p >> 1), int(s["a"]) + (p & 1)] = True
    return out


def check_raster_property(segments, w, step):
    n = len(w)
    loops = stitch(segments, n)
    left_out = 0
    for k in range(n):
        assert all(l.closed for l in loops[k])
        filled, skip = even_odd_fill(loops[k], w[k].shape), touched_samples(segments, k, w[k].shape)
        left_out += int(skip.sum())
        assert numpy.array_equal(filled[~skip], (w[k] < 0)[~skip]), k
        perimeter = sum(float(numpy.hypot(*(numpy.roll(l.points, -1, axis=0) - l.points).T).sum()) for l in loops[k])
        area, count = sum(l.area for l in loops[k]), int((w[k] < 0).sum())
        assert abs(area - count) <= perimeter + 1e-9, k          # in steps: |area - count * step^2| <= perimeter * step
    assert left_out <= 0.01 * w[0].size * n
    return loops


RASTER = ["two_boxes", "boxes_and_ball", "coincident", "diagonal", "bar_64_9", "speck", "grid_64", "far", "random_2_named", "gear_train"]


@pytest.mark.parametrize("name", RASTER)
def test_the_fill_of_the_stitched_loops_is_the_inside_map(name):
    asm, plane, resolution, ref = scenario(name)
    assert max(ref.dims) <= 96
    loops = check_raster_property(ref.segments, ref.w, float(ref.step))
    assert sum(len(l) for l in loops) >= 1 and len(ref.segments) == ref.counts.sum()
    # the plane coordinates of Outlines are first + step * (shifted index - 1)
    placed = outlines_of(ref, plane)
    for a, b in zip(sum(loops, []), sum(placed.loops, [])):
        assert numpy.array_equal(b.points, ref.first + float(ref.step) * a.points) and a.closed == b.closed
    loop = sum(placed.loops, [])[0]
    p3 = placed.points3d(loop)
    assert p3.shape == (len(loop.points), 3) and p3.dtype == numpy.float64
    o, u, v = (x.astype(numpy.float64) for x in (plane.origin, plane.u, plane.v))
    assert numpy.array_equal(p3[0], o + loop.points[0, 0] * u + loop.points[0, 1] * v)


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def test_two_boxes_outline_in_closed_form():
    asm, plane, resolution, ref = scenario("two_boxes")
    assert ref.dims.tolist() == [56, 32] and ref.w.shape == (2, 34, 58)
    loops = stitch(ref.segments, 2, ref.first, float(ref.step))
    assert [len(l) for l in loops] == [1, 1]
    # the faces lie half-way between samples: t = 0.5 on every crossing up to rounding, the outline is the rectangle with cut corners
    assert loops[0][0].area == pytest.approx(4.0 - 4 * 0.0625 ** 2 / 8) and loops[1][0].area == pytest.approx(2.0 - 4 * 0.0625 ** 2 / 8)
    assert ref.counts.tolist() == [4 * 31 + 4, 2 * (31 + 15) + 4]        # the squares along a face, and a corner square each


def test_the_diagonal_scenario_has_both_saddles():
    asm, plane, resolution, ref = scenario("diagonal")
    s = ref.segments
    squares = collections.Counter(zip(s["a"].tolist(), s["b"].tolist()))
    saddles = [sq for sq, count in squares.items() if count == 2]
    kinds = {tuple(sorted(s["e_from"][(s["a"] == a) & (s["b"] == b)].tolist())) for a, b in saddles}
    assert kinds == {(0, 2), (1, 3)}                          # inside corners 0 and 3; inside corners 1 and 2
    loops = stitch(s, 1)[0]
    assert len(loops) == 3 and all(l.closed and l.area > 0 for l in loops)       # never joined across a saddle


def test_the_grid_uses_bit_63_and_hides_what_is_hidden():
    asm, plane, resolution, ref = scenario("grid_64")
    assert len(ref.instances) == 64 and len(list(asm.all_instances())) == 77
    assert (ref.counts > 0).sum() > 30 and ref.segments["k"].min() < 32 <= ref.segments["k"].max()      # both words of the mask
    leaf = traversal("grid_64").rows[-1]
    assert any(mask >> 63 for _, _, mask in leaf) and any(mask & 0xffffffff for _, _, mask in leaf)
    # (instance 63, a ball with a square hole, is thinner than a step on every such plane: bit 63 is a candidate of finest
    # tiles and is evaluated there, which the evaluations count, but has no segment)


def test_the_bar_has_a_tile_with_a_single_live_column():
    asm, plane, resolution, ref = scenario("bar_64_9")
    assert ref.dims.tolist() == [64, 9]                       # 65 by 10 squares
    leaf = traversal("bar_64_9").rows[-1]
    assert (64, 0, 1) in leaf and (64, 8, 1) in leaf
    assert ((ref.segments["a"] == 64) & (ref.segments["b"] < 8)).sum() == 8       # the right face, in that one column


def test_the_speck_is_one_sample():
    asm, plane, resolution, ref = scenario("speck")
    assert ref.dims.tolist() == [1, 1] and (ref.w[0] < 0).sum() == 1 and ref.w[0, 1, 1] < 0
    assert len(ref.segments) == 4 and sorted(zip(ref.segments["a"].tolist(), ref.segments["b"].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    loops = stitch(ref.segments, 1)[0]
    assert len(loops) == 1 and loops[0].closed and len(loops[0].points) == 4 and loops[0].area > 0


def test_coincident_instances_have_identical_segments():
    asm, plane, resolution, ref = scenario("coincident")
    a, b = ref.segments[ref.segments["k"] == 0].copy(), ref.segments[ref.segments["k"] == 1].copy()
    b["k"] = 0
    assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_a_plane_that_misses_every_part_has_no_tile():
    asm, plane, resolution, ref = scenario("missing")
    assert len(ref.segments) == 0 and traversal("missing").rows == [[]] and traversal("missing").evaluations == 0


def test_a_tile_list_overflows_at_capacity_one():
    assert len(traversal("boxes_and_ball").rows) == 2 and len(traversal("boxes_and_ball").rows[-1]) > 1
    assert len(scenario("boxes_and_ball")[3].segments) > 1


@pytest.mark.parametrize("name", ["two_boxes", "boxes_and_ball", "coincident", "diagonal", "bar_64_9", "speck", "grid_64", "far",
                                  "random_2_named", "gear_train"])
def test_the_culling_rule_loses_no_segment(name):
    asm, plane, resolution, ref = scenario(name)
    culled, dense = traversal(name), traversal(name, False)
    assert len(dense.rows) == 1 and len(dense.rows[0]) == -(-(ref.dims[0] + 1) // 8) * -(-(ref.dims[1] + 1) // 8)
    assert dense.evaluations == (ref.dims[0] + 2 + len(range(8, ref.dims[0] + 1, 8))) * (ref.dims[1] + 2 + len(range(8, ref.dims[1] + 1, 8))) * len(ref.instances)
    assert segments_reached(ref, dense.rows[-1]).tobytes() == ref.segments.tobytes()
    assert segments_reached(ref, culled.rows[-1]).tobytes() == ref.segments.tobytes()
    assert culled.evaluations <= dense.evaluations + 64 * len(ref.instances) * len(culled.rows[0])


def test_the_culled_traversal_drops_candidates_both_ways():
    two, three = traversal("two_boxes"), traversal("boxes_and_ball")
    assert two.dropped_inside >= 1                            # tiles deep inside a box: inside at every corner sample
    assert three.dropped_outside >= 1 and three.dropped_inside >= 1
    assert three.evaluations < traversal("boxes_and_ball", False).evaluations


def test_radius_and_windows_of_squares():
    r = radius(8, numpy.float32(0.25))
    assert r.dtype == numpy.float32 and r == numpy.float32((9 * 0.25 * math.sqrt(2) / 2) * (1 + 2.0 ** -10))
    assert float(r) - 8 * 0.25 * math.sqrt(2) / 2 > 0.25 * math.sqrt(2) / 2        # beyond the farthest corner sample by half a step's diagonal
    wins = numpy.array([[[3, 4, 0], [10, 12, 0]], [[65536, 65536, 0], [0, 0, 0]]])
    assert square_windows(wins).tolist() == [[[3, 4, 0], [11, 13, 0]], [[65536, 65536, 0], [1, 1, 0]]]
    assert wins[0, 1, 0] == 10                                  # (a copy)


def test_what_cannot_be_outlined():
    ball = shapes.sphere(1).make_part("ball")
    pair = cc.assembly("pair", [ball, ball.translated_x(3)])
    with pytest.raises(ValueError, match="assembly"):
        cc.section_outlines(shapes.sphere(1), Plane.xy(), 0.1)
    with pytest.raises(ValueError, match="3D"):
        cc.section_outlines(cc.assembly("flat", [shapes.circle(1).make_part("disc")]), Plane.xy(), 0.1)
    with pytest.raises(ValueError, match="64"):
        cc.section_outlines(cc.assembly("crowd", [ball.translated_x(3 * i) for i in range(65)]), Plane.xy(), 0.1)
    for bad in (0, -1, float("nan"), "fine"):
        with pytest.raises(ValueError, match="resolution"):
            cc.section_outlines(pair, Plane.xy(), bad)
    with pytest.raises(ValueError, match="Plane"):
        cc.section_outlines(pair, ((0, 0, 0), (0, 0, 1)), 0.1)
    with pytest.raises(ValueError, match="65535"):
        # 65536 samples along u: a section, but one index too many here
        cc.section_outlines(cc.assembly("rod", [shapes.box(5, 0.01, 0.01).make_part("rod")]), Plane.xy(), 5.0 / 65535.5)
    with pytest.raises(ValueError, match="finite"):
        cc.section_outlines(cc.assembly("endless", [ball, shapes.half_space().make_part("half")]), Plane.xy(), 0.1)
    # nothing to show, or a plane that misses every box: no launch
    for asm, plane in ((cc.assembly("ghosts", [ball.hidden()]), Plane.xy()), (cc.assembly("ball", [ball]), Plane.xy(5))):
        o = cc.section_outlines(asm, plane, 0.1)
        assert o.runs == 0 and o.evaluations == 0 and len(o.segments) == 0 and o.segments.dtype == SEGMENT
        assert o.loops == [[] for _ in o.instances] and o.counts.tolist() == [0] * len(o.instances)


# ---- the C ABI and the ISA --------------------------------------------------------------------------------------------

def _arguments(name):
    with open(_lib.HEADER) as f:
        proto = re.search(r"int %s\(([^;]*)\);" % name, f.read()).group(1)
    return [re.split(r"[\s*]+", re.sub(r"\[\d*\]", "", p.strip()))[-1] for p in proto.split(",")]


def test_abi_of_the_outline_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_outline_tiles", "hu_outline_leaf"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name]) == len(_arguments(name))
    assert _lib.PROTOTYPES["hu_outline_tiles"][:2] == [ctypes.POINTER(_lib.CellsLaunch), ctypes.POINTER(_lib.CellsChildren)]
    assert _lib.PROTOTYPES["hu_outline_leaf"][0] == ctypes.POINTER(_lib.CellsLaunch)
    section_tiles, tiles, leaf = tsh._arguments("hu_section_tiles"), _arguments("hu_outline_tiles"), _arguments("hu_outline_leaf")
    assert tiles == [a for a in section_tiles if a != "with_distance"]
    assert leaf == ["launch", "u", "v", "segments_dev", "segment_capacity", "totals_dev"]
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    nan3 = (ctypes.c_float * 3)(0, float("nan"), 0)
    held = cells_abi.held(p, (64, 64, 1))
    NULL_RECORD = cells_abi.NULL_RECORD

    def tiles_call(u=f3, v=f3, child_side=8, thr=1.0, counter_dev=p, children_dev=p, children={}, **broken):
        listed = cells_abi.children(counter_dev=counter_dev, children_dev=children_dev, capacity=1, child_side=child_side, thr=thr, **children)
        return lib.hu_outline_tiles(cells_abi.launch(**dict(held, **broken)), listed, u, v)

    def leaf_call(u=f3, v=f3, segments=p, capacity=1, totals=p, **broken):
        return lib.hu_outline_leaf(cells_abi.launch(**dict(held, **broken)), u, v, segments, capacity, totals)

    common = [{"table_dev": None}, {"windows_dev": None}, {"parents_dev": None}, {"n_parents_dev": None}, {"evaluations_dev": None},
              NULL_RECORD, {"u": None}, {"v": None}, {"n": 0}, {"n": 65}, {"dims": (0, 8, 1)}, {"dims": (8, 65537, 1)}, {"dims": (65537, 8, 1)},
              {"step": float("nan")}, {"step": -1.0}, {"u": nan3}, {"v": nan3}, {"corner": (0, float("nan"), 0)}]
    for kwargs in common + [{"child_side": 4}, {"child_side": 12}, {"child_side": 16384}, {"thr": -1.0}, {"thr": float("nan")},
                            {"counter_dev": None}, {"children_dev": None}, {"children": NULL_RECORD}]:
        assert tiles_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    for kwargs in common + [{"segments": None}, {"totals": None}]:
        assert leaf_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    assert leaf_call(**NULL_RECORD) == -3 and b"NULL" in lib.hu_last_error()


def test_the_outline_kernels_use_no_scratch_and_the_registers_recorded(tmp_path):
    """From the ISA of instance_outline.hip, as the sister tests read theirs: no kernel has scratch, and each has the vector
    registers that DESIGN.md section 9 records."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_outline.hip" in builder.SOURCES and "instance_outline.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_outline.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_outline.hip")], check=True, capture_output=True)
    text = out.read_text()
    with open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")) as f:
        design = f.read()
    seen = {}
    for chunk in re.split(r"\n(?=_Z\w+:\s+; @)", text):
        m = re.match(r"(_Z\w+):", chunk)
        if not m or "k_outline_" not in m.group(1):
            continue
        name, flag = re.search(r"(k_outline_\w+?)ILb([01])E", m.group(1)).groups()
        scratch = re.search(r"; ScratchSize: (\d+)", chunk)
        assert scratch and int(scratch.group(1)) == 0, m.group(1)
        seen[(name, flag)] = int(re.search(r"; NumVgprs: (\d+)", chunk).group(1))
    assert sorted(seen) == [(k, f) for k in ("k_outline_leaf", "k_outline_tiles") for f in "01"]
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", text.split(".amdgpu_metadata")[1])) >= 4
    for (name, flag), vgprs in seen.items():
        recorded = re.search(r"`%s<%s>` (\d+) VGPRs" % (name, {"0": "false", "1": "true"}[flag]), design)
        assert recorded and int(recorded.group(1)) == vgprs, (name, flag, vgprs)


# ---- the SVG ----------------------------------------------------------------------------------------------------------

def _paths(document):
    root = xml.etree.ElementTree.fromstring(document)
    return root, [e for e in root if e.tag.endswith("path")]


def test_svg_of_reference_outlines():
    asm, plane, resolution, ref = scenario("boxes_and_ball")
    outlines = outlines_of(ref, plane)
    root, paths = _paths(assembly_section_svg.assembly_section_svg_document(outlines))
    with_loops = [k for k, loops in enumerate(outlines.loops) if loops]
    assert len(with_loops) == 3 == len(paths)
    hues = assembly_picture.part_colors(ref.instances, "parts")
    for k, path in zip(with_loops, paths):
        assert path.get("fill-rule") == "evenodd"
        assert path.get("fill") == "#%02x%02x%02x" % tuple(int(round(float(c) * 255)) for c in hues[k])
        d = path.get("d")
        assert d.count("M") == d.count("Z") == len(outlines.loops[k])
        x, y = (float(c) for c in re.match(r"M([^,]+),([^LZ]+)", d).groups())
        assert (x, y) == (outlines.loops[k][0].points[0, 0], -outlines.loops[k][0].points[0, 1])      # v up: y negated
        assert len(re.findall(r"[ML]", d)) == sum(len(l.points) for l in outlines.loops[k])
    step = float(ref.step)
    box = [float(c) for c in root.get("viewBox").split()]
    assert box[2] == pytest.approx(step * (ref.dims[0] + 1)) and box[3] == pytest.approx(step * (ref.dims[1] + 1))
    assert box[0] == pytest.approx(ref.first[0] - step, abs=1e-5) and box[1] == pytest.approx(-(ref.first[1] + step * ref.dims[1]), abs=1e-5)
    assert root.get("width") == "%rmm" % box[2]
    own = assembly_section_svg.assembly_section_svg_document(outlines, colors=[(1, 0, 0), (0, 1, 0), (0, 0, 1)])
    assert [p.get("fill") for p in _paths(own)[1]] == ["#ff0000", "#00ff00", "#0000ff"]


def test_svg_strokes_open_loops_and_refuses_bad_colours():
    segments = field_segments(_disc(10, (9.2, 4.5), 3.1), _disc(10, (4.4, 4.6), 2.2))
    asm = tsh.two_boxes()
    named = [_instance_cells.Instance(i.name, i) for i in _instance_cells.visible(asm, 1.0)]
    outlines = Outlines(named, Plane.xy(), numpy.zeros(3, numpy.float32), numpy.float32(1), (8, 8), segments, stitch(segments, 2),
                        numpy.bincount(segments["k"]), 0, 0)
    root, paths = _paths(assembly_section_svg.assembly_section_svg_document(outlines))
    assert [p.get("class") for p in paths] == ["open", None] and "Z" not in paths[0].get("d") and paths[0].get("fill") is None
    assert paths[1].get("fill-rule") == "evenodd" and root.get("viewBox").split() == ["-1.0", "-8.0", "9.0", "9.0"]
    for colors in ("rainbow", [(1, 0, 0)], {"nobody": (1, 0, 0)}, [(2, 0, 0), (0, 0, 0)]):
        with pytest.raises(ValueError):
            assembly_section_svg.assembly_section_svg_document(outlines, colors)
        with pytest.raises(ValueError):
            rendering.render_assembly_section_svg(asm, os.devnull, Plane.xy(), 0.1, colors)      # before any launch
