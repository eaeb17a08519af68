"""Assemblies on the host (codecad_amd/assemblies.py, rendering/bom.py) and what the interference check decides without
a device: its argument checks, its lattice, its top-level cells, and the ISA of its kernels and the clearance check's."""
import collections
import csv
import math
import os
import re
import subprocess

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, util, nodes, assemblies
from codecad_amd._instance_cells import lattice, top_cells as _top_cells, top_side as _top_side, visible as _visible


def _parts():
    bolt = shapes.cylinder(h=4, d=1).make_part("bolt", ["M1", "steel"])
    nut = shapes.box(2, 2, 1).make_part("nut", ["M1"])
    washer = shapes.cylinder(h=0.2, d=2).make_part("washer")
    return bolt, nut, washer


def _names(items):
    return [(item.name, item.count) for item in items]


def test_bom_recursive_flat_visible_and_suffixes():
    bolt, nut, washer = _parts()
    other_nut = shapes.box(3, 3, 1).make_part("nut")         # a distinct part with the same name
    third_nut = shapes.box(4, 4, 1).make_part("nut")
    joint = cc.assembly("joint", [bolt, nut.translated_z(1), washer.translated_z(0.5)])
    asm = cc.assembly("frame", [joint, joint.translated_x(10), other_nut.hidden(), nut.translated_y(5), third_nut])

    assert _names(asm.bom()) == [("bolt", 2), ("nut", 3), ("nut-2", 1), ("nut-3", 1), ("washer", 2)]
    assert _names(asm.bom(visible_only=True)) == [("bolt", 2), ("nut", 3), ("nut-2", 1), ("washer", 2)]
    assert _names(asm.bom(recursive=False)) == [("joint", 2), ("nut", 1), ("nut-2", 1), ("nut-3", 1)]
    item = next(i for i in asm.bom() if i.name == "bolt")
    assert item.part is bolt.part and item.shape() is bolt.part.data and str(item) == "2x bolt"
    # the two joints are one part (the same Assembly object) in the flat BOM
    flat = cc.assembly("pair", [joint, joint.rotated_z(90)])
    assert _names(flat.bom(recursive=False)) == [("joint", 2)]
    assert _names(flat.bom()) == [("bolt", 2), ("nut", 2), ("washer", 2)]


def test_hidden_subassembly_hides_its_instances():
    bolt, nut, _ = _parts()
    inner = cc.assembly("inner", [bolt, nut])
    asm = cc.assembly("outer", [inner.hidden(), nut.translated_x(3)])
    assert [i.visible for i in asm.all_instances()] == [False, False, True]
    assert _names(asm.bom(visible_only=True)) == [("nut", 1)]
    assert asm.hidden().visible is False and asm.hidden().hidden(False).visible is True


def test_assembly_value_errors():
    with pytest.raises(ValueError):
        cc.assembly("empty", [])
    with pytest.raises(ValueError):
        cc.assembly("mixed", [shapes.circle(1).make_part("disc"), shapes.sphere(1).make_part("ball")])
    with pytest.raises(ValueError):
        shapes.sphere(1).make_part("ball").translated(1, 2)
    assert not hasattr(shapes.sphere(1).make_part("ball"), "scaled")        # solid bodies: no scaling


def test_dimensions_and_2d_assemblies():
    disc = shapes.circle(2).make_part("disc")
    asm2 = cc.assembly("plate", [disc, disc.translated(3, 0).rotated(90), disc.translated_y(1)])
    assert asm2.dimension() == 2 and isinstance(asm2, assemblies.AssemblyTransform2D)
    assert asm2.shape().dimension() == 2
    box = asm2.shape().bounding_box()
    assert box.b.y == pytest.approx(4.0) and box.a.x == pytest.approx(-1.0)
    asm3 = cc.assembly("stack", [shapes.sphere(1).make_part("ball")])
    assert asm3.dimension() == 3 and isinstance(asm3, assemblies.AssemblyTransform3D)


def test_shape_is_the_union_of_the_visible_instances():
    bolt, nut, washer = _parts()
    sub = cc.assembly("sub", [nut.translated(1, 2, 3), washer.rotated_x(30)])
    asm = cc.assembly("top", [bolt, sub.rotated((1, 1, 0), 45).translated_z(2), washer.hidden()])
    visible = [i.shape() for i in asm.all_instances() if i.visible]
    assert len(visible) == 3
    got, want = nodes.make_program(asm.shape()), nodes.make_program(shapes.union(visible))
    assert got.tobytes() == want.tobytes()
    # a placed assembly is its union placed
    moved = asm.translated(5, 0, 0)
    assert nodes.make_program(moved.shape()).tobytes() == nodes.make_program(shapes.union(visible).translated(5, 0, 0)).tobytes()


def test_nested_transforms_compose():
    block = shapes.box(2, 2, 2).make_part("block")
    inner = cc.assembly("inner", [block.translated_x(3)])
    middle = cc.assembly("middle", [inner.rotated_z(90)])
    outer = cc.assembly("outer", [middle.translated(0, 0, 10), block])
    first, second = list(outer.all_instances())
    # block at x = 3, turned about z by 90 degrees -> y = 3, then lifted by 10
    b = first.shape().bounding_box()
    assert tuple(b.a) == pytest.approx((-1, 2, 9), abs=1e-9) and tuple(b.b) == pytest.approx((1, 4, 11), abs=1e-9)
    assert tuple(second.shape().bounding_box().a) == pytest.approx((-1, -1, -1))
    t = first.transform.transform_vector(util.Vector(0, 0, 0))
    assert tuple(t) == pytest.approx((0, 3, 10), abs=1e-12)
    assert first.name == "block" and first.attributes == []


def test_render_bom_csv(tmp_path):
    bolt, nut, washer = _parts()
    asm = cc.assembly("joint", [bolt, nut, nut.translated_z(2), washer])
    path = tmp_path / "bom.csv"
    cc.rendering.render_bom(asm, str(path))
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows == [["name", "count"], ["bolt", "1", "M1", "steel"], ["nut", "2", "M1"], ["washer", "1"]]


def test_interference_argument_checks_need_no_device():
    disc = shapes.circle(1).make_part("disc")
    with pytest.raises(ValueError, match="3D"):
        cc.interference(cc.assembly("flat", [disc, disc.translated_x(1)]), 0.1)
    ball = shapes.sphere(1).make_part("ball")
    crowd = cc.assembly("crowd", [ball.translated_x(i) for i in range(65)])
    with pytest.raises(ValueError, match="64"):
        cc.interference(crowd, 0.1)
    # hidden instances do not count against the limit
    assert len(_visible(cc.assembly("crowd", [ball.translated_x(i) for i in range(64)] + [ball.hidden()]), 0.1)) == 64
    pair = cc.assembly("pair", [ball, ball.translated_x(1)])
    for bad in (0, -0.1, float("nan"), float("inf"), "0.1", None):
        with pytest.raises(ValueError, match="resolution"):
            cc.interference(pair, bad)
    with pytest.raises(ValueError, match="65536"):
        cc.interference(pair, 1e-5)
    with pytest.raises(ValueError, match="assembly"):
        cc.interference(shapes.sphere(1), 0.1)


def test_interference_lattice_and_top_cells():
    ball = shapes.sphere(2).make_part("ball")
    far = cc.assembly("far", [ball, ball.translated_x(10)])
    corner, step, dims = lattice(_visible(far, 0.25), 0.25)
    assert step == numpy.float32(0.25) and corner.dtype == numpy.float32
    assert corner.tolist() == [-0.875, -0.875, -0.875] and dims.tolist() == [48, 8, 8]
    # boxes three metres apart share no top cell: nothing to launch
    assert _top_side(dims) == 16 and len(_top_cells(_visible(far, 0.25), corner, float(step), dims, 16)) == 0
    near = cc.assembly("near", [ball, ball.translated_x(1.5)])
    inst = _visible(near, 0.25)
    corner, step, dims = lattice(inst, 0.25)
    rows = _top_cells(inst, corner, float(step), dims, 16)
    assert rows.tolist() == [[0, 0, 3, 0]]
    assert _top_side(numpy.array([4000, 4000, 30])) == 64 and _top_side(numpy.array([4000, 4000, 4000])) == 256


def check_instance_kernels_isa(text):
    """Every interference and clearance kernel: no scratch; no vector-memory load at all (what they read -- arguments,
    the instance table, the windows, the records and constants of a program, a cell's row, the list's length and a
    pair's least key -- is wave-uniform); and the interpreter's fetch groups as wide scalar loads off one pointer loaded
    from memory (the program's), not only the single wide load of the kernel arguments.  Returns the instantiations
    seen, as (kernel, its boolean template arguments)."""
    seen = set()
    for chunk in re.split(r"\n(?=_Z\w+:\s+; @)", text):
        m = re.match(r"(_Z\w+):", chunk)
        if not m or not re.search(r"k_(interference|clearance|instance)_", m.group(1)):
            continue
        name, flags = re.search(r"(k_(?:interference|clearance|instance)_\w+?)I((?:Lb[01]E)+)E", m.group(1)).groups()
        seen.add((name, "".join(re.findall(r"Lb([01])E", flags))))
        scratch = re.search(r"; ScratchSize: (\d+)", chunk)
        assert scratch and int(scratch.group(1)) == 0, m.group(1)
        body = chunk.split(".section")[0]
        assert not re.search(r"\t(flat|global|buffer)_load", body), m.group(1)
        loaded = set(re.findall(r"\ts_load_dwordx[24] s\[(\d+):\d+\]", body))       # pointers read from memory
        wide = collections.Counter(re.findall(r"\ts_load_dwordx(?:8|16) s\[\d+:\d+\], s\[(\d+):\d+\]", body))
        assert any(n >= 2 and base in loaded for base, n in wide.items()), m.group(1)
    return seen


def test_instance_kernels_keep_their_records_in_scalar_registers(tmp_path):
    """The interference and clearance kernels reach every instance's program through a device table indexed by a
    wave-uniform instance number: their records must still come in through scalar loads, and nothing may spill to
    scratch.  Every instantiation the library launches: k_instance_cells<distance only, windowed> is interference's
    cells kernel without windows and clearance's with them."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_pairs.hip" in builder.SOURCES and "instance_pairs.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_pairs.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_pairs.hip")], check=True, capture_output=True)
    assert check_instance_kernels_isa(out.read_text()) == {
        ("k_instance_cells", "00"), ("k_instance_cells", "10"), ("k_interference_leaf", "0"), ("k_interference_leaf", "1"),
        ("k_instance_cells", "01"), ("k_instance_cells", "11"), ("k_clearance_leaf", "0"), ("k_clearance_leaf", "1"),
        ("k_clearance_witness", "0"), ("k_clearance_witness", "1")}


def test_interference_entry_points_reject_bad_arguments():
    from codecad_amd.hip_util import _lib
    import ctypes
    import cells_abi
    lib = _lib.load()
    dl, lb = ctypes.c_int(0), ctypes.c_uint32(0)
    buf = (ctypes.c_uint8 * 64)()
    tapes = (ctypes.c_void_p * 1)(None)
    assert lib.hu_instance_table(tapes, 1, 0, buf, 64, ctypes.byref(dl), ctypes.byref(lb)) == -3
    assert lib.hu_instance_table(tapes, 65, 0, buf, 64, ctypes.byref(dl), ctypes.byref(lb)) == -3
    nulls = cells_abi.launch(table_dev=None, parents_dev=None, n_parents_dev=None, evaluations_dev=None)
    assert lib.hu_interference_leaf_indirect(nulls, None) == -3
    assert b"NULL" in lib.hu_last_error()
