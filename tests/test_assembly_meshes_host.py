"""The surface meshes of an assembly's parts (codecad_amd/assembly_meshes.py), the parts that need no device: the properties
of the REFERENCE MESHES of assembly_meshes_scenes.py that depend on no case table, the scenarios of the GPU file (each shown
here to contain what it is for), the reference traversal (the culling loses nothing), welding and sorting on synthetic
records, the C ABI, the ISA of the kernels and the STL writer."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, rendering, _instance_cells
from codecad_amd.assembly_meshes import (TRIANGLE, CORNERS, EDGES, EDGE_LOWER, EDGE_AXIS, Meshes, weld, sort_triangles, cube_windows,
                                          radius, top_cells, vertex_keys, vertex_points)
from codecad_amd.rendering import assembly_stl, stl_renderer
from codecad_amd.hip_util import _lib
import oracle

import assembly_meshes_scenes as scenes
import cells_abi
from assembly_meshes_scenes import (SCENES, scene, reference, traversal, meshes_of, check_mesh_properties, euler_characteristic,
                                    components, triangles_reached, dense_evaluations, default_capacity, case_table, crossing,
                                    triangles_of, is_closed_and_oriented, signed_volume)

am = sys.modules["codecad_amd.assembly_meshes"]        # (the package's attribute of that name is the function)


def test_exports():
    assert cc.assembly_meshes is am.assembly_meshes and cc.Meshes is Meshes and cc.TRIANGLE is TRIANGLE
    assert {"assembly_meshes", "Meshes", "TRIANGLE"} <= set(cc.__all__)
    assert Meshes._fields == ("instances", "corner", "step", "dims", "triangles", "counts", "evaluations", "runs")
    assert rendering.render_assembly_stl is assembly_stl.render_assembly_stl


def test_the_record_is_32_bytes_in_the_device_layout():
    assert TRIANGLE.itemsize == 32
    words = numpy.array([[3 | 7 << 16, 9 | 63 << 16 | 4 << 24, 0x5a | 1 << 8 | 10 << 16 | 11 << 24, 0,
                          numpy.float32(0.25).view(numpy.uint32), numpy.float32(0.5).view(numpy.uint32), numpy.float32(1).view(numpy.uint32), 0]],
                        dtype="<u4")
    r = words.view(TRIANGLE).reshape(-1)[0]
    assert (r["a"], r["b"], r["c"], r["k"], r["which"], r["case"]) == (3, 7, 9, 63, 4, 0x5a)
    assert r["e"].tolist() == [1, 10, 11] and r["t"].tolist() == [0.25, 0.5, 1.0] and r["zero"] == 0 and r["unused"] == 0


def test_the_numbering_is_the_generator_s():
    table = case_table()
    assert len(table) == 256 and table[0] == [] and table[255] == [] and max(len(t) for t in table) == 5
    assert EDGE_AXIS.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2]
    for e, (p, q) in enumerate(EDGES):
        lower, upper = sorted((CORNERS[p], CORNERS[q]))
        assert tuple(EDGE_LOWER[e]) == lower and upper[EDGE_AXIS[e]] == lower[EDGE_AXIS[e]] + 1
    assert [e for e, (p, q) in enumerate(EDGES) if CORNERS[q] < CORNERS[p]] == [2, 3, 6, 7]      # listed from their higher end
    for case, tris in enumerate(table):                              # the table lists crossed edges only
        for e in {e for tri in tris for e in tri}:
            assert (case >> EDGES[e][0] & 1) != (case >> EDGES[e][1] & 1)


def test_crossings_are_float32_from_the_lower_end_and_half_for_no_number():
    assert crossing(-1.0, 3.0) == numpy.float32(0.25) and crossing(2.0, -6.0) == numpy.float32(0.25)
    a, b = numpy.float32(-0.1), numpy.float32(0.2)
    assert crossing(a, b) == a / (a - b) and crossing(a, b).dtype == numpy.float32
    assert crossing(-1.0, float("nan")) == numpy.float32(0.5) and crossing(-numpy.inf, numpy.inf) == numpy.float32(0.5)
    assert crossing(-0.0, -1.0) == 0 and crossing(-1.0, 0.0) == 1        # a surface through a sample: that sample is outside
    # edge 2 runs from corner 2 (1, 1, 0) to corner 3 (0, 1, 0): t is measured from corner 3, the lower end
    w = numpy.ones((1, 4, 4, 4), dtype=numpy.float32)
    w[0, 1, 2, 1] = -3.0                                            # one inside sample: corner 3 of cube (1, 1, 1)
    records, cases = triangles_of(w)
    assert len(records) == 8 and cases[0, 1, 1, 1] == 8
    (r,) = records[(records["a"] == 1) & (records["b"] == 1) & (records["c"] == 1)]
    assert sorted(r["e"].tolist()) == [2, 3, 11] and set(r["t"].tolist()) == {numpy.float32(0.75), numpy.float32(0.25)}
    assert r["t"][r["e"].tolist().index(2)] == numpy.float32(0.75)      # w_p / (w_p - w_q) = -3 / -4 from the inside end (0, 1, 0)
    assert r["t"][r["e"].tolist().index(3)] == numpy.float32(0.25)      # edge 3 (corner 3 to corner 0) starts at corner 0: 1 / 4


# ---- welding and sorting on synthetic records -------------------------------------------------------------------------

def _record(a, b, c, k, which, case, e, t):
    r = numpy.zeros(1, dtype=TRIANGLE)
    r["a"], r["b"], r["c"], r["k"], r["which"], r["case"] = a, b, c, k, which, case
    r["e"], r["t"] = e, t
    return r


def test_sorting_is_by_k_c_b_a_which():
    rows = [(1, 0, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 1, 0, 0), (5, 1, 0, 0, 0), (4, 2, 0, 0, 0), (0, 0, 0, 1, 0)]
    records = numpy.concatenate([_record(a, b, c, k, which, 1, (0, 3, 8), (0.5, 0.5, 0.5)) for a, b, c, k, which in rows])
    got = sort_triangles(records)
    assert [(int(r["k"]), int(r["c"]), int(r["b"]), int(r["a"]), int(r["which"])) for r in got] == sorted(
        (k, c, b, a, which) for a, b, c, k, which in rows)


def test_welding_is_over_exact_keys_in_order_of_first_use():
    # two cubes side by side along x share the edge 9 of the first = the edge 8 of the second, and 1 = 3, 5 = 7, 10 = 11
    first = _record(2, 3, 4, 0, 0, 0, (0, 9, 1), (0.25, 0.5, 0.75))
    second = _record(3, 3, 4, 0, 0, 0, (8, 0, 3), (0.5, 0.125, 0.75))
    keys = vertex_keys(numpy.concatenate([first, second]))
    assert keys[0, 1] == keys[1, 0] and keys[0, 2] == keys[1, 2] and len(numpy.unique(keys)) == 4
    vertices, triangles = weld(numpy.concatenate([first, second]))
    assert triangles.dtype == numpy.uint32 and triangles.tolist() == [[0, 1, 2], [1, 3, 2]]
    assert vertices.dtype == numpy.float64 and vertices.tolist() == [[1.25, 2.0, 3.0], [2.0, 2.0, 3.5], [2.0, 2.75, 3.0], [2.125, 2.0, 3.0]]
    # a position is float64(corner) + float64(step) * (shifted index - 1), the float32 t widened
    corner, step = numpy.array([0.1, -2.0, 3.0], dtype=numpy.float32), numpy.float32(0.3)
    third = _record(0, 0, 0, 0, 0, 0, (8, 0, 3), (numpy.float32(0.1), 0.5, 1.0))
    placed, _ = weld(third, corner, step)
    assert numpy.array_equal(placed[0], corner.astype(numpy.float64) + float(step) * (numpy.array([0, 0, float(numpy.float32(0.1))]) - 1.0))
    assert vertex_points(third)[0].tolist() == [[0, 0, float(numpy.float32(0.1))], [0.5, 0, 0], [0, 1.0, 0]]
    assert [x.shape for x in weld(numpy.zeros(0, dtype=TRIANGLE))] == [(0, 3), (0, 3)]


def test_meshes_mesh_takes_the_records_of_its_instance():
    ref = reference("ball")
    meshes = meshes_of(ref)
    for k in range(2):
        vertices, triangles = meshes.mesh(k)
        own = ref.triangles[ref.triangles["k"] == k]
        assert len(triangles) == len(own) == ref.counts[k] and triangles.max() == len(vertices) - 1
        assert numpy.array_equal(numpy.unique(triangles.reshape(-1), return_index=True)[1].argsort(), numpy.arange(len(vertices)))
        want = ref.corner.astype(numpy.float64) + float(ref.step) * (vertex_points(own[:1])[0] - 1.0)
        assert numpy.array_equal(vertices[triangles[0]], want)
    with pytest.raises(IndexError):
        meshes.mesh(2)


# ---- the properties that depend on no table, on every scenario's reference mesh ----------------------------------------

@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_reference_mesh_is_closed_oriented_and_as_large_as_its_samples(name):
    ref = reference(name)
    assert len(ref.triangles) == ref.counts.sum() and ref.w.shape[1:] == tuple(int(d) + 2 for d in ref.dims)
    assert max(ref.dims) <= 108
    check_mesh_properties(meshes_of(ref), ref)
    for k in range(len(ref.instances)):                             # the ring is outside every part: nothing is cut open
        inner = ref.w[k][1:-1, 1:-1, 1:-1]
        assert (ref.w[k] < 0).sum() == (inner < 0).sum()


def _euler(name):
    ref = reference(name)
    meshes = meshes_of(ref)
    return [(euler_characteristic(*meshes.mesh(k)), components(*meshes.mesh(k))) for k in range(len(ref.instances))]


def test_euler_characteristics():
    assert _euler("ball") == [(2, 1), (2, 1)]                       # a ball and a box
    assert _euler("torus") == [(0, 1)] and _euler("box_with_hole") == [(0, 1)]
    assert _euler("speck") == [(2, 1)]
    assert _euler("zigzag") == [(6, 3)]                             # never joined across an ambiguous face: three closed boxes
    assert _euler("dust") == [(0, 0)]


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def _ambiguous_faces(case):
    """How many faces of a cube of this case have their inside corners on a diagonal only."""
    faces = [[m for m, c in enumerate(CORNERS) if c[axis] == side] for axis in range(3) for side in (0, 1)]
    count = 0
    for face in faces:
        inside = [m for m in face if case >> m & 1]
        if len(inside) == 2 and sum(abs(a - b) for a, b in zip(CORNERS[inside[0]], CORNERS[inside[1]])) == 2:
            count += 1
    return count


def test_the_rims_have_lanes_past_the_rim_and_a_cell_one_cube_wide():
    assert reference("rims").dims.tolist() == [13, 9, 11]           # 14 x 10 x 12 cubes: x and y end inside a cell
    assert reference("rims_4k1").dims.tolist() == [12, 8, 4]        # 13 x 9 x 5 cubes: the last cell of every axis is one cube wide
    leaf = traversal("rims_4k1").rows[-1]
    assert (12, 8, 4, 1) in leaf
    t = reference("rims_4k1").triangles
    assert ((t["a"] == 12) & (t["b"] == 8) & (t["c"] == 4)).sum() >= 1      # the far corner of the box, in that one cube
    for name in ("rims", "rims_4k1"):
        t = reference(name).triangles
        assert [int(t[f].max()) for f in "abc"] == reference(name).dims.tolist()      # triangles in the last cube of every axis
        assert [int(t[f].min()) for f in "abc"] == [0, 0, 0]


def test_the_zigzag_has_face_ambiguous_cases():
    ref = reference("zigzag")
    cases = numpy.unique(ref.triangles["case"]).tolist()
    assert any(_ambiguous_faces(c) for c in cases)
    assert sum(_ambiguous_faces(int(c)) for c in ref.cases[0].reshape(-1)) % 2 == 0        # every such face is shared by two cubes


def test_the_speck_is_one_sample_and_the_dust_none():
    ref = reference("speck")
    assert ref.dims.tolist() == [1, 1, 1] and (ref.w[0] < 0).sum() == 1 and ref.w[0, 1, 1, 1] < 0
    assert len(ref.triangles) == 8 and sorted(numpy.unique(ref.triangles["case"]).tolist()) == [1 << m for m in range(8)]
    assert (reference("dust").w < 0).sum() == 0 and len(reference("dust").triangles) == 0
    assert len(traversal("dust").rows[-1]) >= 1                     # finest cells are reached and evaluated, and give nothing


def test_coincident_instances_have_identical_records():
    ref = reference("coincident")
    a, b = ref.triangles[ref.triangles["k"] == 0].copy(), ref.triangles[ref.triangles["k"] == 1].copy()
    b["k"] = 0
    assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_the_64_solids_use_bit_63_and_hide_what_is_hidden():
    asm, resolution, instances, corner, step, dims = scene("solids64")
    ref = reference("solids64")
    assert len(instances) == 64 and len(list(asm.all_instances())) == 66
    assert (ref.counts > 0).all() and ref.counts[63] > 0 and ref.triangles["k"].max() == 63
    leaf = traversal("solids64").rows[-1]
    assert any(mask >> 63 for *_, mask in leaf) and any(mask & 0xffffffff and mask >> 32 for *_, mask in leaf)


def test_far_from_the_origin_a_step_is_four_ulps():
    ref = reference("far")
    assert numpy.abs(ref.corner).min() > 1e5
    xs = scenes.ringed_axes(ref.corner, ref.step, ref.dims)[0]
    assert (numpy.spacing(numpy.abs(ref.corner)) >= ref.step / 4).all() and len(numpy.unique(xs)) == len(xs)       # a quarter of a step is one ulp there
    assert (ref.counts > 0).all()


def test_strict_samples_on_faces_are_outside_and_crossed_at_exactly_0_or_1():
    ref = reference("strict")
    assert ref.corner.tolist() == [-1.0, -1.0, -1.0] and ref.step == 0.0625
    assert ((ref.w[1:] == 0).sum(axis=(1, 2, 3)) > 100).all()       # samples ON the faces of the two halves
    t = ref.triangles["t"]
    assert ((t == 0) | (t == 1)).sum() > 1000                       # the crossing is the sample itself
    k1 = ref.triangles[ref.triangles["k"] == 1]
    assert ((k1["t"] == 0) | (k1["t"] == 1)).all()                  # the half's faces all lie on samples
    vertices, triangles = meshes_of(ref).mesh(1)
    assert 0.95 < signed_volume(vertices, triangles) < 1.0          # t = 1 puts every vertex ON a face: the unit box, less its chamfered edges


def test_the_notch_gives_degenerate_triangles_and_they_are_kept():
    ref = reference("strict_notch")
    assert ref.corner.tolist() == [-0.5, -0.5, -0.5] and ref.step == 0.125 and (ref.w[1] == 0).sum() > 100
    own = ref.triangles[ref.triangles["k"] == 1]
    assert ((own["t"] == 0) | (own["t"] == 1)).all()
    points = vertex_points(own)
    degenerate = (points[:, 0] == points[:, 1]).all(axis=-1) | (points[:, 1] == points[:, 2]).all(axis=-1) | (points[:, 0] == points[:, 2]).all(axis=-1)
    assert degenerate.sum() >= 8                                    # along the concave edge: two crossings on one sample
    keys = vertex_keys(own[degenerate])
    assert all(len(set(k)) == 3 for k in keys.tolist())             # three lattice edges all the same: the keys keep the mesh closed
    vertices, triangles = meshes_of(ref).mesh(1)
    assert is_closed_and_oriented(triangles) and not is_closed_and_oriented(triangles[~degenerate])

def test_the_forced_sides_run_three_and_four_levels(monkeypatch):
    for name, levels in (("coarse_64", 3), ("coarse_256", 4)):
        dims = scene(name)[5]
        assert max(dims) < 100
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.forced_top_cells(dims + 1, SCENES[name].side))
        assert _instance_cells.top_side(dims + 1) == SCENES[name].side
        monkeypatch.undo()
        assert len(traversal(name).rows) == levels and all(len(r) >= 1 for r in traversal(name).rows)
    assert traversal("coarse_64").rows[-1] == traversal("coarse_256").rows[-1]
    assert _instance_cells.top_side(scene("gears")[5] + 1) == 16


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_culling_rule_loses_no_triangle(name):
    asm, resolution, instances, corner, step, dims = scene(name)
    ref, culled, dense = reference(name), traversal(name), traversal(name, False)
    assert len(dense.rows) == 1 and len(dense.rows[0]) == int(numpy.prod(-(-(dims + 1) // 4)))
    assert all(mask == (1 << len(instances)) - 1 for *_, mask in dense.rows[0])
    assert dense.evaluations == dense_evaluations(dims, len(instances))
    assert triangles_reached(ref, dense.rows[-1]).tobytes() == ref.triangles.tobytes()
    assert triangles_reached(ref, culled.rows[-1]).tobytes() == ref.triangles.tobytes()
    # every finest row's mask holds every instance that has a triangle there
    masks = {row[:3]: row[3] for row in culled.rows[-1]}
    t = ref.triangles
    for a, b, c, k in set(zip(t["a"].tolist(), t["b"].tolist(), t["c"].tolist(), t["k"].tolist())):
        assert masks[(a & ~3, b & ~3, c & ~3)] >> k & 1
    assert len(ref.triangles) <= default_capacity(name)             # the first triangle buffer holds them: one run


def test_the_culled_traversal_drops_candidates_both_ways():
    assert traversal("ball").dropped_outside >= 1 and traversal("gears").dropped_outside >= 1
    assert traversal("strict").dropped_inside >= 1 and traversal("coarse_64").dropped_inside >= 1
    assert traversal("solids64").evaluations < traversal("solids64", False).evaluations / 10


def test_radius_windows_and_top_cells():
    r = radius(4, numpy.float32(0.25))
    assert r.dtype == numpy.float32 and r == numpy.float32((5 * 0.25 * 3 ** 0.5 / 2) * (1 + 2.0 ** -10))
    assert float(r) - 4 * 0.25 * 3 ** 0.5 / 2 > 0.25 * 3 ** 0.5 / 2       # beyond the farthest corner sample by half a step's diagonal
    wins = numpy.array([[[3, 4, 5], [10, 12, 14]]])
    assert cube_windows(wins).tolist() == [[[3, 4, 5], [11, 13, 15]]] and wins[0, 1, 0] == 10
    rows = top_cells(cube_windows(wins), numpy.array([17, 17, 17]), 4, everywhere=True)
    assert len(rows) == 125 and (rows[:, 2] == 1).all() and (rows[:, 3] == 0).all()
    assert sorted(set((rows[:, 0] & 0xffff).tolist())) == [0, 4, 8, 12, 16] == sorted(set((rows[:, 0] >> 16).tolist())) == sorted(set(rows[:, 1].tolist()))
    some = top_cells(cube_windows(wins), numpy.array([17, 17, 17]), 16)
    assert len(some) == 1 and some[0].tolist() == [0, 0, 1, 0]


def test_what_cannot_be_meshed():
    ball = shapes.sphere(1).make_part("ball")
    pair = cc.assembly("pair", [ball, ball.translated_x(3)])
    with pytest.raises(ValueError, match="assembly"):
        cc.assembly_meshes(shapes.sphere(1), 0.1)
    with pytest.raises(ValueError, match="3D"):
        cc.assembly_meshes(cc.assembly("flat", [shapes.circle(1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError, match="64"):
        cc.assembly_meshes(cc.assembly("crowd", [ball.translated_x(3 * i) for i in range(65)]), 0.1)
    for bad in (0, -1, float("nan"), "fine"):
        with pytest.raises(ValueError, match="resolution"):
            cc.assembly_meshes(pair, bad)
    with pytest.raises(ValueError, match="65535"):
        # 65536 samples along x: a lattice interference() takes, but one index too many for the cubes
        cc.assembly_meshes(cc.assembly("rod", [shapes.box(5, 0.01, 0.01).make_part("rod")]), 5.0 / 65535.5)
    with pytest.raises(ValueError, match="finite"):
        cc.assembly_meshes(cc.assembly("endless", [ball, shapes.half_space().make_part("half")]), 0.1)
    m = cc.assembly_meshes(cc.assembly("ghosts", [ball.hidden()]), 0.1)         # nothing to show: no launch
    assert m.runs == 0 and m.evaluations == 0 and len(m.triangles) == 0 and m.triangles.dtype == TRIANGLE
    assert m.instances == [] and m.counts.tolist() == []


# ---- the C ABI and the ISA --------------------------------------------------------------------------------------------

def _arguments(name):
    with open(_lib.HEADER) as f:
        proto = re.search(r"int %s\(([^;]*)\);" % name, f.read()).group(1)
    return [re.split(r"[\s*]+", re.sub(r"\[\d*\]", "", p.strip()))[-1] for p in proto.split(",")]


def test_abi_of_the_mesh_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_mesh_cells", "hu_mesh_leaf_instances"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name]) == len(_arguments(name))
    # a level is what traverse() passes every level, and the leaf adds its records after the launch record
    assert _lib.PROTOTYPES["hu_mesh_cells"] == _lib.PROTOTYPES["hu_clearance_cells_indirect"] == \
        [ctypes.POINTER(_lib.CellsLaunch), ctypes.POINTER(_lib.CellsChildren)]
    assert _arguments("hu_mesh_cells") == _arguments("hu_clearance_cells_indirect") == ["launch", "children"]
    assert _lib.PROTOTYPES["hu_mesh_leaf_instances"][0] == ctypes.POINTER(_lib.CellsLaunch)
    assert _arguments("hu_mesh_leaf_instances") == ["launch", "triangles_dev", "triangle_capacity", "totals_dev"]
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    held = cells_abi.held(p, (64, 64, 64))
    NULL_RECORD = cells_abi.NULL_RECORD

    def cells_call(child_side=4, thr=1.0, counter_dev=p, children_dev=p, children={}, **broken):
        listed = cells_abi.children(counter_dev=counter_dev, children_dev=children_dev, capacity=1, child_side=child_side, thr=thr, **children)
        return lib.hu_mesh_cells(cells_abi.launch(**dict(held, **broken)), listed)

    def leaf_call(triangles=p, capacity=1, totals=p, **broken):
        return lib.hu_mesh_leaf_instances(cells_abi.launch(**dict(held, **broken)), triangles, capacity, totals)

    common = [{"table_dev": None}, {"windows_dev": None}, {"parents_dev": None}, {"n_parents_dev": None}, {"evaluations_dev": None},
              NULL_RECORD, {"n": 0}, {"n": 65}, {"dims": (0, 8, 8)}, {"dims": (8, 65537, 8)}, {"dims": (65537, 8, 8)}, {"dims": (8, 8, 65537)},
              {"step": float("nan")}, {"step": -1.0}]
    for kwargs in common + [{"child_side": 2}, {"child_side": 12}, {"child_side": 32768}, {"thr": -1.0}, {"thr": float("nan")},
                            {"counter_dev": None}, {"children_dev": None}, {"children": NULL_RECORD}]:
        assert cells_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    for kwargs in common + [{"triangles": None}, {"totals": None}]:
        assert leaf_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    assert leaf_call(**NULL_RECORD) == -3 and b"NULL" in lib.hu_last_error()


def test_the_mesh_kernels_use_no_scratch_and_the_registers_recorded(tmp_path):
    """From the ISA of instance_mesh.hip, as the sister tests read theirs: no kernel has scratch, and each has the vector
    registers that DESIGN.md section 9 records."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_mesh.hip" in builder.SOURCES and "instance_mesh.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_mesh.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_mesh.hip")], check=True, capture_output=True)
    text = out.read_text()
    with open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")) as f:
        design = f.read()
    seen = {}
    for chunk in re.split(r"\n(?=_Z\w+:\s+; @)", text):
        m = re.match(r"(_Z\w+):", chunk)
        if not m or "k_mesh_" not in m.group(1):
            continue
        name, flag = re.search(r"(k_mesh_\w+?)ILb([01])E", m.group(1)).groups()
        scratch = re.search(r"; ScratchSize: (\d+)", chunk)
        assert scratch and int(scratch.group(1)) == 0, m.group(1)
        seen[(name, flag)] = int(re.search(r"; NumVgprs: (\d+)", chunk).group(1))
    assert sorted(seen) == [(k, f) for k in ("k_mesh_cells", "k_mesh_leaf") for f in "01"]
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", text.split(".amdgpu_metadata")[1])) >= 4
    for (name, flag), vgprs in seen.items():
        recorded = re.search(r"`%s<%s>` (\d+) VGPRs" % (name, {"0": "false", "1": "true"}[flag]), design)
        assert recorded and int(recorded.group(1)) == vgprs, (name, flag, vgprs)


def test_the_sources_of_the_library():
    from codecad_amd.hip_util import builder
    assert "instance_mesh.hip" in builder.SOURCES and "instance_mesh.hip" not in builder.FLAGGED_SOURCES
    assert os.path.exists(os.path.join(builder.CSRC, "instance_mesh.hip"))


# ---- the STL files ----------------------------------------------------------------------------------------------------

def test_stl_files_of_reference_meshes(tmp_path):
    ref = reference("ball")
    meshes = meshes_of(ref)
    paths = rendering.write_assembly_stl(meshes, str(tmp_path / "parts"))
    assert [os.path.basename(p) for p in paths] == ["00_ball.stl", "01_box.stl"]
    for k, path in enumerate(paths):
        with open(path, "rb") as f:
            data = f.read()
        assert len(data) == 84 + 50 * int(ref.counts[k]) and struct.unpack("<I", data[80:84])[0] == ref.counts[k]
        got = numpy.frombuffer(data[84:], dtype=stl_renderer.RECORD)
        want = oracle.stl_records(*meshes.mesh(k))
        assert got.tobytes() == want.tobytes() and (got["attr"] == 0).all() and got["vectors"].dtype == numpy.float32
    assert assembly_stl.stl_name(7, "a b/c:d.e-f_g") == "07_a_b_c_d.e-f_g.stl" and assembly_stl.stl_name(12, "é") == "12__.stl"
