"""The layered outlines of an assembly (codecad_amd/layer_outlines.py), the parts that need no device: the heights, the
record, the top rows, the reference stack of layer_outlines_scenes.py shown to be the loop over the per-plane reference
(records, counts, corner, dims and evaluations: the stack IS the loop), the culling rule, the areas of two boxes in closed
form, the C ABI, the ISA of the kernels and the SVG writer."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import rendering, _instance_cells
from codecad_amd.section import Plane, lattice
from codecad_amd.section_outlines import SEGMENT, Outlines, stitch
from codecad_amd.rendering import assembly_layers_svg, assembly_section_svg
from codecad_amd.hip_util import _lib

import cells_abi
import layer_outlines_scenes as scenes
import test_section_host as tsh
import test_section_outlines_host as tso

lo = sys.modules["codecad_amd.layer_outlines"]       # (the package's attribute of that name is the function)


def layers_of(ref):
    """The Layers a device run must give, from the reference (evaluations and runs left 0)."""
    named = [_instance_cells.Instance(i.name, i) for i in ref.instances]
    return lo.Layers(named, ref.plane, ref.heights, ref.planes, ref.corners, ref.step, tuple(int(d) for d in ref.dims), ref.segments,
                     ref.layer_counts, ref.counts, 0, 0)


def test_exports():
    assert cc.layer_outlines is lo.layer_outlines and cc.layer_heights is lo.layer_heights and cc.Layers is lo.Layers
    assert cc.LAYER_SEGMENT is lo.LAYER_SEGMENT and lo.LAYER_SEGMENT.itemsize == 16
    assert rendering.render_assembly_layers_svg is assembly_layers_svg.render_assembly_layers_svg
    assert lo.Layers._fields == ("instances", "plane", "heights", "planes", "corners", "step", "dims", "segments", "layer_counts", "counts",
                                 "evaluations", "runs")
    assert cc.layer_outlines.__doc__ and "layer_outlines" in cc.__doc__


# ---- heights ----------------------------------------------------------------------------------------------------------

def test_heights_are_validated():
    asm = tsh.two_boxes()
    for bad in ([], [0.0, -1.0], [0.0, 0.0], [0.0, float("nan")], [0.0, float("inf")], [[0.0, 1.0]], "high", None,
                numpy.arange((1 << 20) + 1, dtype=numpy.float64)):
        with pytest.raises(ValueError, match="heights"):
            cc.layer_outlines(asm, Plane.xy(0), 0.0625, bad)
    assert lo.checked_heights(numpy.arange(1 << 20)).shape == (1 << 20,) and lo.checked_heights([3]).tolist() == [3.0]
    with pytest.raises(ValueError, match="Plane"):
        cc.layer_outlines(asm, ((0, 0, 0), (0, 0, 1)), 0.0625, [0.0])
    with pytest.raises(ValueError, match="resolution"):
        cc.layer_outlines(asm, Plane.xy(0), 0, [0.0])
    with pytest.raises(ValueError, match="assembly"):
        cc.layer_outlines(tsh.two_boxes().shape(), Plane.xy(0), 0.1, [0.0])


def test_layer_heights_of_two_boxes():
    asm = tsh.two_boxes()
    h = cc.layer_heights(asm, Plane.xy(0), 0.5)
    assert h.dtype == numpy.float64 and h.tolist() == [-1.75, -1.25, -0.75, -0.25, 0.25, 0.75]
    assert cc.layer_heights(asm, Plane.xy(0.5), 1.0).tolist() == [-2.0, -1.0, 0.0]          # from the plane's origin
    assert cc.layer_heights(asm, Plane.xy(0), 0.7).tolist() == [-2 + 0.7 * (l + 0.5) for l in range(5)]
    for bad in (0, -0.5, float("nan"), float("inf"), "thin", 3.0 / (1 << 20) / 1.001):
        with pytest.raises(ValueError, match="layer_height"):
            cc.layer_heights(asm, Plane.xy(0), bad)
    assert len(cc.layer_heights(asm, Plane.xy(0), 3.0 / (1 << 20))) == 1 << 20
    with pytest.raises(ValueError, match="Plane"):
        cc.layer_heights(asm, None, 0.5)
    ball = cc.shapes.sphere(1).make_part("ball")
    assert cc.layer_heights(cc.assembly("ghosts", [ball.hidden()]), Plane.xy(0), 0.5).shape == (0,)


def test_planes_and_corners_of_the_layers():
    asm, plane, resolution, heights, ref = scenes.scenario("boxes_and_ball")
    assert len(heights) == 5 and numpy.all(numpy.diff(heights) > 0)
    planes, corners = lo.layer_planes(plane, heights, ref.first)
    assert corners.dtype == numpy.float32 and corners.tobytes() == ref.corners.tobytes()
    for mine, theirs in zip(planes, ref.planes):
        assert isinstance(mine, Plane) and mine.origin.dtype == numpy.float32 and mine.origin.tobytes() == theirs.origin.tobytes()
        assert mine.u is plane.u and mine.v is plane.v and mine.normal is plane.normal          # the frame, untouched
    # a layer of a named plane IS the named plane at that height, and its corner the per-plane lattice's
    asm, plane, resolution, heights, ref = scenes.scenario("two_boxes")
    for l, h in enumerate(heights):
        named = scenes.named_plane(plane, h)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ref.planes[l], named))
        assert lattice(ref.instances, named, resolution)[0].tobytes() == ref.corners[l].tobytes()
    assert scenes.named_plane(Plane.xz(0), 0.25).origin.tolist() == [0, -0.25, 0]


# ---- the record -------------------------------------------------------------------------------------------------------

def test_records_pack_and_unpack():
    for layer in (0, 4095, 4096, 65535, 65536, (1 << 20) - 1):
        for e_from, e_to in itertools.product(range(4), range(4)):
            word = lo.pack(63, e_from, e_to, layer)
            assert word.dtype == numpy.uint32 and int(word) == 63 + e_from * 256 + e_to * 1024 + layer * 4096 < 1 << 32
            assert [int(x) for x in lo.unpack(word)] == [63, e_from, e_to, layer]
    records = numpy.zeros(3, dtype=lo.LAYER_SEGMENT)
    records["a"], records["b"], records["t_from"], records["t_to"] = [5, 65535, 1], [7, 2, 65535], [0.25, 0.5, 1], [0.75, 0, 0.125]
    records["word"] = lo.pack([63, 0, 7], [3, 0, 1], [1, 2, 3], [(1 << 20) - 1, 0, 65536])
    raw = records.view(numpy.uint32).reshape(3, 4)
    assert raw[0].tolist() == [5 | 7 << 16, 63 | 3 << 8 | 1 << 10 | ((1 << 20) - 1) << 12, 0x3e800000, 0x3f400000]
    segments = lo.to_segments(records)
    assert segments.dtype == SEGMENT and segments["k"].tolist() == [63, 0, 7] and segments["e_from"].tolist() == [3, 0, 1]
    assert segments["e_to"].tolist() == [1, 2, 3] and segments["a"].tolist() == [5, 65535, 1] and segments["b"].tolist() == [7, 2, 65535]
    assert segments["t_from"].tolist() == [0.25, 0.5, 1] and segments["t_to"].tolist() == [0.75, 0, 0.125]
    assert [int(x) for x in lo.unpack(lo.sort_records(records)["word"])[3]] == [0, 65536, (1 << 20) - 1]
    # the order: layer, k, b, a, e_from
    mixed = numpy.zeros(5, dtype=lo.LAYER_SEGMENT)
    mixed["word"] = lo.pack([1, 0, 0, 0, 0], [0, 0, 0, 2, 1], 0, [0, 1, 0, 0, 0])
    mixed["a"], mixed["b"] = [0, 0, 9, 3, 3], [0, 0, 1, 2, 2]
    assert lo.sort_records(mixed).tolist() == [mixed[i].tolist() for i in (2, 4, 3, 0, 1)]


# ---- the top rows -----------------------------------------------------------------------------------------------------

def device_top_rows(asm, plane, resolution, heights, cull=True):
    """[(layer, a0, b0, mask)] as layer_outlines() lists them."""
    instances = _instance_cells.visible(asm, resolution)
    planted = lo.seed(instances, plane, resolution, numpy.asarray(heights, dtype=numpy.float64), cull)
    rows = planted.top
    candidate = lo.candidates(lo.box_corners(instances), numpy.stack([p.origin for p in planted.planes]), plane.normal, planted.step)
    assert rows.dtype == numpy.uint32 and rows.shape[1] == 4
    return [(int(r[1]), int(r[0]) & 0xffff, int(r[0]) >> 16, int(r[2]) | int(r[3]) << 32) for r in rows], candidate


def test_top_rows_of_two_boxes():
    asm, plane, resolution, heights, ref = scenes.scenario("two_boxes")
    rows, candidate = device_top_rows(asm, plane, resolution, heights)
    # -2.25 and 1.5 miss both boxes by more than a step; -1.75 meets b alone; 0.9375 is one step below the tops of both
    assert candidate.tolist() == [[False, False], [False, True], [True, True], [True, True], [True, True], [False, False]]
    assert sorted({r[0] for r in rows}) == [1, 2, 3, 4] and all(mask for _, _, _, mask in rows)
    assert {mask for l, _, _, mask in rows if l == 1} == {2} and {mask for l, _, _, mask in rows if l == 4} == {3}
    assert rows == scenes.reference_top_rows(asm, plane, resolution, heights)[0]
    # ordered by layer, then as cell_rows orders them (a0 before b0)
    assert rows == sorted(rows, key=lambda r: (r[0], r[1], r[2]))
    # within a step of a face: still listed; beyond it: not
    near, _ = device_top_rows(asm, plane, resolution, [1.0 + 0.0625, 1.0 + 0.0626])
    assert {r[0] for r in near} == {0} and all(mask == 3 for _, _, _, mask in near)
    # every tile with the layer's candidates
    dense, _ = device_top_rows(asm, plane, resolution, heights, cull=False)
    assert dense == scenes.reference_top_rows(asm, plane, resolution, heights, cull=False)[0]
    assert len(dense) == 4 * -(-(ref.dims[0] + 1) // 8) * -(-(ref.dims[1] + 1) // 8) and {mask for l, _, _, mask in dense if l == 1} == {2}


def test_top_rows_never_list_a_hidden_instance():
    asm, plane, resolution, heights, ref = scenes.scenario("grid_64")
    rows, candidate = device_top_rows(asm, plane, resolution, heights)
    assert candidate.shape == (3, 64) and len(list(asm.all_instances())) == 77
    assert rows == scenes.reference_top_rows(asm, plane, resolution, heights)[0]
    assert any(mask >> 63 for _, _, _, mask in rows) and any(mask & 0xffffffff for _, _, _, mask in rows)
    assert not candidate.all(axis=1).any() and candidate.any(axis=1).all()          # every layer cuts some solids and misses others
    for name in ("boxes_and_ball", "far", "diagonal", "bar_64_9", "coincident"):
        asm, plane, resolution, heights, ref = scenes.scenario(name)
        assert device_top_rows(asm, plane, resolution, heights)[0] == scenes.reference_top_rows(asm, plane, resolution, heights)[0], name


def test_too_many_top_rows_and_none_at_all():
    wins = numpy.array([[[0, 0, 0], [7, 7, 0]]])
    squares = numpy.array([8, 8, 1])
    some = lo.top_rows(wins, numpy.ones((1 << 20, 1), dtype=bool), squares, 8)
    assert some.shape == (1 << 20, 4) and some[:, 1].tolist() == list(range(1 << 20)) and (some[:, 2] == 1).all()
    with pytest.raises(ValueError, match="top rows"):
        lo.top_rows(numpy.array([[[0, 0, 0], [39, 7, 0]]]), numpy.ones((1 << 20, 1), dtype=bool), numpy.array([40, 8, 1]), 8)
    assert lo.top_rows(wins, numpy.zeros((4, 1), dtype=bool), squares, 8).shape == (0, 4)
    # nothing to show, or layers that miss every box: no launch
    ball = cc.shapes.sphere(1).make_part("ball")
    for asm, heights in ((cc.assembly("ghosts", [ball.hidden()]), [0.0, 1.0]), (cc.assembly("ball", [ball]), [5.0, 6.0])):
        got = cc.layer_outlines(asm, Plane.xy(0), 0.1, heights)
        assert got.runs == 0 and got.evaluations == 0 and len(got.segments) == 0 and got.segments.dtype == lo.LAYER_SEGMENT
        assert got.layer_counts.shape == (2, len(got.instances)) and not got.layer_counts.any() and got.counts.tolist() == [0] * len(got.instances)
        assert len(got.planes) == 2 and got.corners.shape == (2, 3) and got.heights.tolist() == heights
        assert got.layer(1).loops == [[] for _ in got.instances] and got.areas().shape == (2, len(got.instances))
        with pytest.raises(IndexError):
            got.layer(2)


# ---- the stack is the loop --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", scenes.NAMED)
def test_the_reference_stack_is_the_loop_over_the_per_plane_reference(name):
    asm, plane, resolution, heights, ref = scenes.scenario(name)
    assert 1 <= len(heights) <= 8
    stack = layers_of(ref)
    evaluations = 0
    for l, h in enumerate(heights):
        named = scenes.named_plane(plane, h)
        single = tso.reference_outlines(asm, named, resolution)
        layer = stack.layer(l)
        assert isinstance(layer, Outlines) and layer.segments.dtype == SEGMENT and layer.segments.tobytes() == single.segments.tobytes()
        assert layer.counts.tolist() == single.counts.tolist() == ref.layer_counts[l].tolist()
        assert layer.corner.tobytes() == single.corner.tobytes() and layer.dims == tuple(int(d) for d in single.dims) and layer.step == single.step
        assert all(a.tobytes() == b.tobytes() for a, b in zip(layer.plane, named))
        want = stitch(single.segments, len(single.instances), single.first, float(single.step))
        assert [[(p.points.tobytes(), p.closed, p.area) for p in loops] for loops in layer.loops] == \
            [[(p.points.tobytes(), p.closed, p.area) for p in loops] for loops in want]
        evaluations += tso.reference_traversal(asm, named, resolution).evaluations
    assert scenes.traversal(name).evaluations == evaluations > 0
    assert ref.counts.tolist() == ref.layer_counts.sum(axis=0).tolist() and len(ref.segments) == ref.counts.sum()
    assert ref.segments.tobytes() == lo.sort_records(ref.segments[::-1]).tobytes()


@pytest.mark.parametrize("name", sorted(scenes.SCENARIOS))
def test_the_culling_rule_loses_no_segment(name):
    asm, plane, resolution, heights, ref = scenes.scenario(name)
    assert 1 <= len(heights) <= 8 and len(ref.segments) > 0
    culled, dense = scenes.traversal(name), scenes.traversal(name, False)
    assert len(dense.rows) == 1 and len(culled.rows) >= 2
    assert scenes.records_reached(ref, dense.rows[-1]).tobytes() == ref.segments.tobytes()
    assert scenes.records_reached(ref, culled.rows[-1]).tobytes() == ref.segments.tobytes()
    assert all(child[0] in {row[0] for row in culled.rows[0]} for child in culled.rows[-1])      # children keep their parent's layer


def test_what_the_scenarios_hold():
    ref = scenes.scenario("two_boxes")[4]
    assert ref.layer_counts[0].tolist() == ref.layer_counts[5].tolist() == [0, 0] and ref.layer_counts[1, 0] == 0 < ref.layer_counts[1, 1]
    assert (ref.layer_counts[2:5] > 0).all()
    ref = scenes.scenario("diagonal")[4]
    for l in range(3):                      # both saddles on every layer
        s = lo.to_segments(ref.segments[lo.unpack(ref.segments["word"])[3] == l])
        twice = [(a, b) for (a, b), count in __import__("collections").Counter(zip(s["a"].tolist(), s["b"].tolist())).items() if count == 2]
        assert {tuple(sorted(s["e_from"][(s["a"] == a) & (s["b"] == b)].tolist())) for a, b in twice} == {(0, 2), (1, 3)}
    asm, plane, resolution, heights, ref = scenes.scenario("bar_64_9")
    assert ref.dims.tolist() == [64, 9] and all((l, 64, 0, 1) in scenes.traversal("bar_64_9").rows[-1] for l in range(2))
    ref = scenes.scenario("grid_64")[4]
    k = lo.unpack(ref.segments["word"])[0]
    assert len(ref.instances) == 64 and k.min() < 32 <= k.max() and any(mask >> 63 for _, _, _, mask in scenes.traversal("grid_64").rows[-1])
    ref = scenes.scenario("coincident")[4]
    k, _, _, layer = lo.unpack(ref.segments["word"])
    for l in range(3):
        a, b = ref.segments[(layer == l) & (k == 0)].copy(), ref.segments[(layer == l) & (k == 1)].copy()
        b["word"] -= 1
        assert len(a) > 0 and a.tobytes() == b.tobytes()
    asm, plane, resolution, heights, ref = scenes.scenario("far")
    assert numpy.diff(heights).tolist() == [resolution, resolution] and (ref.layer_counts.sum(axis=1) > 0).all()
    assert numpy.abs(ref.corners).min() > 2.0 ** 17                       # a float32 ulp there is a good part of a step


def _two_boxes_areas(ref, heights, cut_corners):
    areas = layers_of(ref).areas()
    assert areas.shape == (len(heights), 2) and areas.dtype == numpy.float64
    print(areas.tolist())
    for l, h in enumerate(heights):
        for k, (inside, area) in enumerate(((abs(h) < 1, 4.0), (-2 < h < 1, 2.0))):
            if inside:
                assert areas[l, k] == pytest.approx(area - cut_corners, rel=1e-5), (l, k, areas[l, k])
            else:
                assert areas[l, k] == 0, (l, k)


def test_two_boxes_areas_with_their_cut_corners():
    """At the scenario's step of 0.0625 the faces lie half-way between samples, so every crossing is at t = 0.5 and marching
    squares cuts each of a rectangle's four corners off along a diagonal of half a step: step^2 / 8 each, 3.998046875 and
    1.998046875 on every layer that cuts a box (tso.test_two_boxes_outline_in_closed_form has the same figure for one cut)."""
    asm, plane, resolution, heights, ref = scenes.scenario("two_boxes")
    _two_boxes_areas(ref, heights, 4 * 0.0625 ** 2 / 8)


def test_two_boxes_areas_in_closed_form():
    """The rectangles' own areas, 4 and 2, within 1e-5 relative.  The outline of a rectangle misses its area by the four cut
    corners of the test above, step^2 / 2 in all whatever the layer: 4.9e-4 and 9.8e-4 of the areas at the scenario's step of
    0.0625, which no arithmetic can mend -- so this test takes the same boxes, plane and heights at a step of 2^-8, where the
    cut corners are 7.6e-6 in all: 1.9e-6 of part a's area and 3.8e-6 of part b's, within the bound."""
    asm, plane, resolution, heights = scenes.SCENARIOS["two_boxes"]()
    ref = scenes.reference_layers(asm, plane, 2.0 ** -8, heights)
    assert ref.dims.tolist() == [896, 512]
    _two_boxes_areas(ref, heights, 0.0)


def test_the_speck_reference_has_four_segments_on_each_of_70000_layers():
    asm, plane, resolution, heights, records, evaluations = scenes.speck_reference()
    k, e_from, e_to, layer = lo.unpack(records["word"])
    assert len(records) == 4 * scenes.SPECK_LAYERS and layer.max() == scenes.SPECK_LAYERS - 1 > 65535 and (numpy.bincount(layer) == 4).all()
    assert records.tobytes() == lo.sort_records(records).tobytes() and (k == 0).all()
    # a layer of it is the per-plane reference
    for l in (0, 65536, scenes.SPECK_LAYERS - 1):
        single = tso.reference_outlines(asm, Plane.xy(heights[l]), resolution)
        assert lo.to_segments(records[layer == l]).tobytes() == single.segments.tobytes()
        assert tso.reference_traversal(asm, Plane.xy(heights[l]), resolution).evaluations == 10 == evaluations // scenes.SPECK_LAYERS


# ---- the C ABI and the ISA --------------------------------------------------------------------------------------------

def test_abi_of_the_layer_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_layer_tiles", "hu_layer_leaf"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name]) == len(tso._arguments(name))
    for layered, plain in (("hu_layer_tiles", "hu_outline_tiles"), ("hu_layer_leaf", "hu_outline_leaf")):
        want = tso._arguments(plain)
        at = want.index("v") + 1
        assert tso._arguments(layered) == want[:at] + ["layer_corners_dev", "n_layers"] + want[at:]
        assert _lib.PROTOTYPES[layered] == _lib.PROTOTYPES[plain][:at] + [_lib._vp, _lib._u32] + _lib.PROTOTYPES[plain][at:]
        assert _lib.PROTOTYPES[layered][0] == ctypes.POINTER(_lib.CellsLaunch)
    assert _lib.PROTOTYPES["hu_layer_tiles"][1] == ctypes.POINTER(_lib.CellsChildren)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    nan3 = (ctypes.c_float * 3)(0, float("nan"), 0)
    held = cells_abi.held(p, (64, 64, 1))
    NULL_RECORD = cells_abi.NULL_RECORD

    def tiles_call(u=f3, v=f3, corners=p, layers=1, child_side=8, thr=1.0, counter_dev=p, children_dev=p, children={}, **broken):
        listed = cells_abi.children(counter_dev=counter_dev, children_dev=children_dev, capacity=1, child_side=child_side, thr=thr, **children)
        return lib.hu_layer_tiles(cells_abi.launch(**dict(held, **broken)), listed, u, v, corners, layers)

    def leaf_call(u=f3, v=f3, corners=p, layers=1, segments=p, capacity=1, totals=p, **broken):
        return lib.hu_layer_leaf(cells_abi.launch(**dict(held, **broken)), u, v, corners, layers, segments, capacity, totals)

    common = [{"table_dev": None}, {"windows_dev": None}, {"parents_dev": None}, {"n_parents_dev": None}, {"evaluations_dev": None},
              NULL_RECORD, {"u": None}, {"v": None}, {"n": 0}, {"n": 65}, {"dims": (0, 8, 1)}, {"dims": (8, 65537, 1)}, {"dims": (65537, 8, 1)},
              {"step": float("nan")}, {"step": -1.0}, {"u": nan3}, {"v": nan3}, {"corner": (0, float("nan"), 0)},
              {"corners": None}, {"layers": 0}, {"layers": (1 << 20) + 1}]
    for kwargs in common + [{"child_side": 4}, {"child_side": 12}, {"child_side": 16384}, {"thr": -1.0}, {"thr": float("nan")},
                            {"counter_dev": None}, {"children_dev": None}, {"children": NULL_RECORD}]:
        assert tiles_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    for kwargs in common + [{"segments": None}, {"totals": None}]:
        assert leaf_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    assert leaf_call(**NULL_RECORD) == -3 and b"NULL" in lib.hu_last_error()


def test_the_layer_kernels_use_no_scratch_and_the_registers_recorded(tmp_path):
    """From the ISA of instance_layers.hip, as the sister tests read theirs: no kernel has scratch, and each has the vector
    registers that DESIGN.md section 9 records."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_layers.hip" in builder.SOURCES and "instance_layers.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_layers.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_layers.hip")], check=True, capture_output=True)
    text = out.read_text()
    with open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")) as f:
        design = f.read()
    seen = {}
    for chunk in re.split(r"\n(?=_Z\w+:\s+; @)", text):
        m = re.match(r"(_Z\w+):", chunk)
        if not m or "k_layer_" not in m.group(1):
            continue
        name, flag = re.search(r"(k_layer_\w+?)ILb([01])E", m.group(1)).groups()
        scratch = re.search(r"; ScratchSize: (\d+)", chunk)
        assert scratch and int(scratch.group(1)) == 0, m.group(1)
        seen[(name, flag)] = int(re.search(r"; NumVgprs: (\d+)", chunk).group(1))
    assert sorted(seen) == [(k, f) for k in ("k_layer_leaf", "k_layer_tiles") for f in "01"]
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", text.split(".amdgpu_metadata")[1])) >= 4
    for (name, flag), vgprs in seen.items():
        recorded = re.search(r"`%s<%s>` (\d+) VGPRs" % (name, {"0": "false", "1": "true"}[flag]), design)
        assert recorded and int(recorded.group(1)) == vgprs, (name, flag, vgprs)


# ---- the SVG ----------------------------------------------------------------------------------------------------------

def test_svg_one_drawing_per_layer(tmp_path, monkeypatch):
    asm, plane, resolution, heights, ref = scenes.scenario("two_boxes")
    stack = layers_of(ref)
    monkeypatch.setattr(assembly_layers_svg, "layer_outlines", lambda *args, **kwargs: stack)        # (the device's part is the GPU file's)
    got = rendering.render_assembly_layers_svg(asm, str(tmp_path / "stack"), plane, resolution, heights)
    assert got is stack and sorted(os.listdir(tmp_path / "stack")) == ["layer_%05d.svg" % l for l in range(6)]
    for l in range(6):
        text = (tmp_path / "stack" / ("layer_%05d.svg" % l)).read_text()
        assert text == assembly_section_svg.assembly_section_svg_document(stack.layer(l), "parts")
        root, paths = tso._paths(text)
        assert len(paths) == int((ref.layer_counts[l] > 0).sum())
    own = [(1, 0, 0), (0, 0, 1)]
    rendering.render_assembly_layers_svg(asm, str(tmp_path / "own"), plane, resolution, heights, colors=own)
    assert [p.get("fill") for p in tso._paths((tmp_path / "own" / "layer_00003.svg").read_text())[1]] == ["#ff0000", "#0000ff"]
    monkeypatch.setattr(assembly_layers_svg, "layer_outlines", lambda *args, **kwargs: pytest.fail("launched"))
    for colors in ("rainbow", [(1, 0, 0)], {"nobody": (1, 0, 0)}, [(2, 0, 0), (0, 0, 0)]):
        with pytest.raises(ValueError):
            rendering.render_assembly_layers_svg(asm, str(tmp_path / "bad"), plane, resolution, heights, colors)      # before any launch
    assert not (tmp_path / "bad").exists()
