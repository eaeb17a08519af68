"""The reference and the scenarios of test_gpu_assembly_mass.py, and the host side of assembly_mass_properties(), checked
without a device.

assembly_mass_scenes.reference_mass has two halves, the dense definition and the traversal of csrc/instance_mass.hip done
in NumPy; that both give the same sums on every scenario is the first test.  Every scenario is then inspected: the edge
it was built for is IN THE REFERENCE, and wherever the rule calls a child full the dense half shows every sample of that
child inside (the premise of the traversal)."""
import collections
import ctypes
import math
import os
import re
import subprocess
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells, assembly_mass
from codecad_amd.hip_util import _lib

import assembly_mass_scenes as scenes
import cells_abi
from assembly_mass_scenes import SCENES, scene, reference


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_index_sums_of_a_small_lattice_by_hand():
    weight = numpy.zeros((3, 4, 5), dtype=numpy.int32)
    weight[1, 2, 3] = 1
    weight[2, 3, 4] = 2                                           # (a sample added twice counts twice)
    assert scenes.index_sums(weight) == (3, 5, 8, 11, 9, 22, 41, 14, 19, 30)
    inside = [numpy.array([[[True, True, False]]]), numpy.array([[[False, True, True]]])]
    assert [m.ravel().tolist() for m in scenes.owners(inside)] == [[True, True, False], [False, False, True]]


@pytest.mark.parametrize("retire", [True, False])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_both_halves_of_the_reference_agree_and_the_premise_holds(name, retire):
    ref = reference(name, retire)
    assert ref.traversal_sums == ref.sums and ref.traversal_owned == ref.owned
    assert ref.premise_broken == 0
    assert sum(o[0] for o in ref.owned) == ref.union_count > 0
    assert all(numpy.isfinite(w).all() for w in ref.w)
    if not retire:
        assert all(level.retired == 0 and level.mixed == 0 for level in ref.levels) and ref.leaf.mixed == 0
    else:
        assert ref.evaluations <= reference(name, False).evaluations


def test_threshold_is_the_drivers():
    for child in (4, 16, 64):
        assert scenes.threshold(child, numpy.float32(0.07)) == assembly_mass.threshold(child, numpy.float32(0.07))
        bound = (child - 1) * float(numpy.float32(0.07)) * math.sqrt(3) / 2      # how far a child's samples lie from its centre
        assert float(scenes.threshold(child, numpy.float32(0.07))) > bound


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def axis_count(lo, hi, corner, step, n):
    """(count, sum, sum of squares) of the indices whose samples lie strictly between lo and hi on one axis."""
    p = float(corner) + float(step) * numpy.arange(n)
    i = numpy.nonzero((p > lo) & (p < hi))[0]
    return len(i), int(i.sum()), int((i * i).sum())


def test_boxes_in_closed_form():
    asm, resolution, instances, corner, step, dims = scene("boxes")
    ref = reference("boxes")
    assert max(dims) <= 48 and dims.tolist() == [28, 16, 24]
    for k, (a, b) in enumerate((scenes.BOX_A, scenes.BOX_B)):
        (nx, sx, sxx), (ny, sy, syy), (nz, sz, szz) = (axis_count(a[c], b[c], corner[c], step, dims[c]) for c in range(3))
        assert ref.sums[k] == (nx * ny * nz, sx * ny * nz, nx * sy * nz, nx * ny * sz, sxx * ny * nz, nx * syy * nz, nx * ny * szz,
                               sx * sy * nz, sx * ny * sz, nx * sy * sz)
    assert ref.owned[0] == ref.sums[0] and ref.owned[1] != ref.sums[1]
    assert ref.sums[1][0] - ref.owned[1][0] == 4 * 8 * 16        # the overlap, 0.5 x 1 x 2
    assert SCENES["boxes"].densities == scenes.BOX_DENSITIES and scenes.BOX_DENSITIES[0] != scenes.BOX_DENSITIES[1]


def test_the_sphere_retires_at_the_finest_level():
    asm, resolution, instances, corner, step, dims = scene("sphere")
    assert resolution == 1 / 16 and dims.tolist() == [32, 32, 32]
    ref = reference("sphere")
    assert [level.child for level in ref.levels] == [4]
    level = ref.levels[0]
    assert level.retired > 0                                      # children of side 4 retire,
    assert level.mixed > 0                                        # children keep a boundary candidate next to a full one,
    assert ref.leaf.mixed > 0                                     # leaf cells mix an inherited full candidate with an evaluated one
    assert ref.evaluations < reference("sphere", False).evaluations


def test_coarse_levels_retire(monkeypatch):
    """A child of side s retires only where the part is (s step sqrt(3) / 2)(1 + 2^-10) deep: 13.9 samples for 16, 55.5 for
    64.  On a lattice of at most 96 samples nothing is 55 samples deep, so the box 80 samples wide retires children of
    side 16 under both forced top sides and its children of side 64 survive; the box of 160 samples retires one of 64."""
    for name, side in (("coarse_64", 64), ("coarse_256", 256), ("coarse_160", 256)):
        asm, resolution, instances, corner, step, dims = scene(name)
        assert SCENES[name].side == side and _instance_cells.top_side(dims) == 16
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.forced_top_cells(dims, side))
        assert _instance_cells.top_side(dims) == side
        monkeypatch.undo()
        by_child = {level.child: level for level in reference(name).levels}
        assert sorted(by_child) == ([4, 16] if side == 64 else [4, 16, 64])
        assert by_child[16].retired >= 1 and by_child[4].retired >= 1
    for name in ("coarse_64", "coarse_256"):
        dims = scene(name)[5]
        assert max(dims) <= 96 and reference(name).boxes[0][1][0] - reference(name).boxes[0][0][0] == 79
    assert {level.child: level.retired for level in reference("coarse_256").levels}[64] == 0
    assert {level.child: level.retired for level in reference("coarse_160").levels}[64] >= 1
    assert reference("coarse_64").sums == reference("coarse_256").sums


def test_ownership_follows_the_order_and_nothing_else_does():
    refs = {order: reference("ownership_%d%d%d" % order) for order in scenes.OWNERSHIP_ORDERS}
    by_part = {}
    for order, ref in refs.items():
        asm, resolution, instances, corner, step, dims = scene("ownership_%d%d%d" % order)
        every = list(asm.all_instances())
        assert len(every) == 4 and [i.visible for i in every] == [True, False, True, True]      # a hidden one between them
        assert sum(isinstance(i, cc.assemblies.AssemblyTransform3D) for i in asm) == 1          # one nested subassembly
        assert [i.name for i in instances] == [("ball", "block", "peg")[p] for p in order]
        inside = [w < 0 for w in ref.w]
        assert (inside[0] & inside[1] & inside[2]).any()
        assert all((inside[i] & inside[j] & ~inside[3 - i - j]).any() for i in range(3) for j in range(i + 1, 3))
        by_part[order] = {p: (ref.sums[k], ref.owned[k]) for k, p in enumerate(order)}
        assert ref.owned[0] == ref.sums[0] and ref.owned[1] != ref.sums[1] and ref.owned[2] != ref.sums[2]
    first = by_part[scenes.OWNERSHIP_ORDERS[0]]
    for order in scenes.OWNERSHIP_ORDERS[1:]:
        assert all(by_part[order][p][0] == first[p][0] for p in range(3))                      # the V_k do not change,
        assert any(by_part[order][p][1] != first[p][1] for p in range(3))                      # the O_k do,
        assert refs[order].union_count == refs[scenes.OWNERSHIP_ORDERS[0]].union_count          # their total does not


@pytest.mark.parametrize("name,n", [("solids33", 33), ("solids64", 64)])
def test_solids_overlap_across_the_words_of_the_mask(name, n):
    asm, resolution, instances, corner, step, dims = scene(name)
    every = list(asm.all_instances())
    assert len(instances) == n and len(every) > n and sum(isinstance(i, cc.assemblies.AssemblyTransform3D) for i in asm) == 1
    ref = reference(name)
    assert all(s[0] > 0 for s in ref.sums)
    inside = [w < 0 for w in ref.w]
    low = numpy.zeros_like(inside[0])
    for m in inside[:32]:
        low |= m
    crossing = [k for k in range(32, n) if (inside[k] & low).any()]
    assert crossing and all(ref.owned[k][0] < ref.sums[k][0] for k in crossing)      # an index below 32 takes samples from one above
    assert any(0 < ref.owned[k][0] for k in crossing)
    if n == 64:
        assert len(crossing) >= 8 and any(ref.owned[k][0] < ref.sums[k][0] for k in range(1, 32))
    assert ref.levels[0].retired > 0 and ref.leaf.mixed > 0


def test_rims_reach_the_last_index_of_every_axis():
    asm, resolution, instances, corner, step, dims = scene("rims")
    assert dims.tolist() == [13, 9, 11] and all(d % 4 for d in dims)
    ref = reference("rims")
    assert ref.boxes[0] == ((0, 0, 0), (12, 8, 10)) and ref.sums[0][0] == 13 * 9 * 11
    assert ref.owned[1][0] == 0 and ref.sums[1][0] > 0    # the ball lies inside the block: it owns nothing


def test_strictness_a_sample_on_a_face_is_not_inside():
    asm, resolution, instances, corner, step, dims = scene("strict")
    assert step == 0.0625 and corner.tolist() == [-1.0] * 3 and dims.tolist() == [33] * 3
    ref = reference("strict")
    outer, right, left = ref.w
    assert (right == 0).sum() >= 6 * 15 * 15 and (left == 0).sum() >= 6 * 15 * 15
    assert ref.sums[1][0] == 15 ** 3 == ref.sums[2][0] and int((right <= 0).sum()) == 17 ** 3
    assert ref.owned[1][0] == 0 == ref.owned[2][0] and ref.owned[0][0] == ref.sums[0][0] == ref.union_count


@pytest.mark.parametrize("name", ["blend", "gears", "random_1", "random_2", "random_5"])
def test_blends_and_gears(name):
    """The premise itself is checked for every scenario above (premise_broken == 0); none of this group had to be replaced."""
    asm, resolution, instances, corner, step, dims = scene(name)
    ref = reference(name)
    assert len(instances) == {"blend": 2, "gears": 8, "random_1": 4, "random_2": 9, "random_5": 12}[name] and max(dims) <= 108
    assert any(o[0] < s[0] for o, s in zip(ref.owned, ref.sums))                      # parts overlap
    assert sum(level.retired for level in ref.levels) > 0 and ref.evaluations < reference(name, False).evaluations
    if name == "blend":
        assert "blend" in {i.name for i in instances}


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_densities_forms_and_errors():
    asm = scenes._boxes()
    instances = _instance_cells.visible(asm, 0.125)
    assert assembly_mass.part_densities(instances, None) == [1.0, 1.0]
    assert assembly_mass.part_densities(instances, (2, numpy.float32(0.5))) == [2.0, 0.5]
    assert assembly_mass.part_densities(instances, {"b": 7.8}) == [1.0, 7.8]
    assert assembly_mass.part_densities(instances, {"b": 0, "nobody": 3.0}) == [1.0, 0.0]
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, -1.0], [1.0, float("nan")], [float("inf"), 1.0], {"a": -2.0}, {"a": "steel"}, [1.0, None],
                {"nobody": float("nan")}):
        with pytest.raises(ValueError):
            assembly_mass.part_densities(instances, bad)
    with pytest.raises(ValueError):                                # before any launch
        cc.assembly_mass_properties(asm, 0.125, densities=[1.0])


def test_refusals_of_interference_and_the_overflow_bound():
    ball = shapes.sphere(r=1).make_part("ball")
    for bad in (0, -1.0, float("nan"), "fine"):
        with pytest.raises(ValueError):
            cc.assembly_mass_properties(cc.assembly("one", [ball]), bad)
    with pytest.raises(ValueError):
        cc.assembly_mass_properties(shapes.sphere(r=1), 0.1)
    with pytest.raises(ValueError):
        cc.assembly_mass_properties(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.assembly_mass_properties(cc.assembly("many", [ball.translated_x(3 * k) for k in range(65)]), 0.5)
    with pytest.raises(ValueError):                                # 70000 samples on an axis
        cc.assembly_mass_properties(cc.assembly("long", [shapes.box(700, 1, 1).make_part("rod")]), 0.01)
    # prod(dims) (max(dims) - 1)^2 >= 2^64: 60000^3 x 59999^2 is about 2^79
    assembly_mass.check_overflow((7131, 7131, 7131))               # 7131^3 x 7130^2 < 2^64 ...
    assert 7131 ** 3 * 7130 ** 2 < 2 ** 64 <= 7132 ** 3 * 7131 ** 2
    with pytest.raises(ValueError):
        assembly_mass.check_overflow((7132, 7132, 7132))          # ... and one more sample per axis is refused
    with pytest.raises(ValueError):
        cc.assembly_mass_properties(cc.assembly("cube", [shapes.box(600).make_part("cube")]), 0.01)


def test_no_visible_instance_gives_an_empty_report():
    ghost = shapes.box(1).make_part("ghost").hidden()
    r = cc.assembly_mass_properties(cc.assembly("nothing", [ghost]), 0.1)
    assert r.instances == [] and r.parts == [] and r.traversals == 0 and r.samples_evaluated == 0
    assert r.total_mass == 0 and r.union_volume == 0 and r.total.volume == 0 and not r.total.inertia_tensor.any()
    assert tuple(int(d) for d in r.dims) == (1, 1, 1)


def test_physical_quantities_from_sums_by_hand():
    # two samples, at indices (0, 0, 0) and (2, 0, 0), corner (1, 2, 3), step 0.5: cubes centred on x = 1 and x = 2
    got = assembly_mass.integrals((2, 2, 0, 0, 4, 0, 0, 0, 0, 0), numpy.array([1.0, 2.0, 3.0]), 0.5)
    cube = 0.125
    assert got["1"] == 2 * cube and got["x"] == cube * 3 and got["y"] == cube * 4 and got["z"] == cube * 6
    assert got["xx"] == pytest.approx(cube * (1 + 4 + 2 * 0.25 / 12)) and got["yy"] == pytest.approx(cube * (8 + 2 * 0.25 / 12))
    assert got["xy"] == pytest.approx(cube * (2 + 4)) and got["yz"] == pytest.approx(cube * 12)
    acc = numpy.zeros(1, dtype=assembly_mass._ACC)
    acc["v"][0] = acc["o"][0] = (2, 2, 0, 0, 4, 0, 0, 0, 0, 0)
    acc["hi"][0] = (2, 0, 0)
    inst = types.SimpleNamespace(name="pair")
    r = assembly_mass.report([inst], numpy.array([1, 2, 3], numpy.float32), numpy.float32(0.5), numpy.array([3, 1, 1]), acc, [4.0], 0, 1)
    part = r.parts[0]
    assert (part.count, part.volume, part.mass, part.index_box) == (2, 0.25, 1.0, ((0, 0, 0), (2, 0, 0)))
    assert tuple(part.properties.centroid) == pytest.approx((1.5, 2.0, 3.0)) and r.total_mass == 1.0 and r.union_volume == 0.25
    assert tuple(r.total.centroid) == pytest.approx((1.5, 2.0, 3.0))
    # two cubes of side 0.5 half a unit either side of the centroid: about x each s^2 / 6 per unit mass, about y and z also the offsets
    own, steiner = 0.125 * 0.25 / 6, 0.125 * 0.25
    assert numpy.diag(part.properties.inertia_tensor) == pytest.approx([2 * own, 2 * (own + steiner), 2 * (own + steiner)])
    assert numpy.diag(r.total.inertia_tensor) == pytest.approx([4 * 2 * own, 4 * 2 * (own + steiner), 4 * 2 * (own + steiner)])


class _FakeBuffer:
    made = []

    def __init__(self, dtype, shape, queue=None):
        self.dtype, self.shape, self.written, self.device_ptr = dtype, shape, None, 0x1000 * (len(_FakeBuffer.made) + 1)
        _FakeBuffer.made.append(self)

    def enqueue_write(self, array):
        self.written = numpy.array(array, copy=True)

    def read(self):
        return self.written

    def release(self):
        pass


def _recorded_run(monkeypatch, top, **kwargs):
    calls = []

    def as_called(arg):
        """a launch record as it was when the call was made (_run() moves its parent fields on from level to level)"""
        record = getattr(arg, "_obj", None)
        if not isinstance(record, ctypes.Structure):
            return arg
        values = {name: getattr(record, name) for name, _ in record._fields_}
        return {name: list(v) if isinstance(v, ctypes.Array) else v for name, v in values.items()}

    class Lib:
        def __getattr__(self, name):
            return lambda *args: calls.append((name, tuple(as_called(a) for a in args))) or 0

    _FakeBuffer.made = []
    monkeypatch.setattr(_instance_cells, "hip_manager", types.SimpleNamespace(lib=Lib(), queue=types.SimpleNamespace(handle=None)))
    monkeypatch.setattr(_instance_cells.hip_util, "Buffer", _FakeBuffer)
    from codecad_amd.interference import _PAIR
    table = types.SimpleNamespace(device_ptr=0x10)
    sides, capacities = _instance_cells.levels(16, len(top), None, **{k: v for k, v in kwargs.items() if k == "row_bytes"})
    _instance_cells._run(table, 2, 1, 64, None, top, sides, numpy.zeros(3, numpy.float32), numpy.float32(0.1), numpy.array([28, 16, 24]),
                         capacities, types.SimpleNamespace(handle=None), _PAIR, {"lo": 0xffffffff}, lambda child: numpy.float32(1),
                         "cells", [("leaf", ())], 4, (), **kwargs)
    monkeypatch.undo()
    return calls, list(_FakeBuffer.made), capacities


def test_the_default_rows_of_the_traversal_are_what_they_were(monkeypatch):
    """interference's first list, byte for byte: a 16-byte header {count, 0, 0, 0} and the 16-byte rows of top_cells();
    its entry points get the rows 16 bytes in, by the fields of their launch records; and the same with 32-byte rows where
    they are asked for."""
    asm, resolution, instances, corner, step, dims = scene("boxes")
    top = _instance_cells.top_cells(instances, corner, float(step), dims, 16)
    assert len(top) >= 1 and top.dtype == numpy.uint32 and top.shape[1] == 4
    calls, buffers, capacities = _recorded_run(monkeypatch, top)
    results, parents, children = buffers
    expected = numpy.concatenate([numpy.array([len(top), 0, 0, 0], dtype=numpy.uint32), top.ravel()])
    assert parents.written.tobytes() == expected.tobytes() and parents.shape == (len(top) + 1, 4)
    assert children.shape == (capacities[0] + 1, 4)
    by_name = dict(calls)
    assert by_name["hu_memset"][:3] == (children.device_ptr, 0, 16)

    def parents_of(launch):
        return launch["parents_dev"], launch["n_parents_dev"], launch["max_parents"]

    launch, listed = by_name["cells"]
    assert parents_of(launch) == (parents.device_ptr + 16, parents.device_ptr, len(top))
    assert (launch["table_dev"], launch["windows_dev"], launch["n"], launch["distance_only"], launch["lane_bytes"]) == (0x10, None, 2, 1, 64)
    assert (launch["dims"], launch["corner"], launch["step"]) == ([28, 16, 24], [0.0] * 3, numpy.float32(0.1))
    assert launch["evaluations_dev"] == results.device_ptr + 16
    assert (listed["counter_dev"], listed["children_dev"], listed["capacity"]) == (children.device_ptr, children.device_ptr + 16, capacities[0])
    assert (listed["child_side"], listed["thr"]) == (4, 1.0)
    launch, pairs = by_name["leaf"]
    assert parents_of(launch) == (children.device_ptr + 16, children.device_ptr, capacities[0]) and pairs == results.device_ptr + 32
    assert results.written.size == 16 + 16 + 4 * 64 and _instance_cells.levels(64, 1, None)[0] == [64, 16]
    # rows of 32 bytes, an argument and the accumulators for the cells level, one accumulator per instance
    rows = assembly_mass.top_rows(instances, corner, step, dims, 16)
    assert rows.shape[1] == 8 and not rows[:, 4:].any() and numpy.array_equal(rows[:, :4], _instance_cells.cell_rows(
        _instance_cells.windows(instances, corner, float(step), dims), dims, 16, least=1))
    calls, buffers, capacities = _recorded_run(monkeypatch, rows, row_bytes=32, cells_extra=(1,), accumulators=2)
    results, parents, children = buffers
    assert parents.written.tobytes()[:32] == numpy.array([len(rows)] + [0] * 7, dtype=numpy.uint32).tobytes()
    assert parents.written.tobytes()[32:] == rows.tobytes() and children.shape == (capacities[0] + 1, 8)
    by_name = dict(calls)
    assert parents_of(by_name["cells"][0]) == (parents.device_ptr + 32, parents.device_ptr, len(rows)) and len(by_name["cells"]) == 4
    assert by_name["cells"][2:] == (1, results.device_ptr + 32) and by_name["leaf"][0]["parents_dev"] == children.device_ptr + 32
    assert results.written.size == 16 + 16 + 2 * 64


# ---- the C ABI and the ISA --------------------------------------------------------------------------------------------

def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_assembly_mass_cells", "hu_assembly_mass_leaf"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        with open(_lib.HEADER) as f:
            proto = re.search(r"int %s\(([^;]*)\);" % name, f.read()).group(1)
        assert len(_lib.PROTOTYPES[name]) == len(proto.split(","))
        with open(os.path.join(os.path.dirname(_lib.HEADER), "..", "INTEGRATION.md")) as f:
            assert ("int %s(" % name) in f.read()
        assert _lib.PROTOTYPES[name][0] == ctypes.POINTER(_lib.CellsLaunch)
    assert _lib.PROTOTYPES["hu_assembly_mass_cells"][1] == ctypes.POINTER(_lib.CellsChildren)
    assert assembly_mass._ACC.itemsize == 192 and assembly_mass._ROW == 32
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    held = cells_abi.held(p, (64, 64, 64))
    NULL_RECORD = cells_abi.NULL_RECORD

    def cells_call(child_side=4, thr=1.0, counter_dev=p, children_dev=p, children={}, acc=p, **broken):
        listed = cells_abi.children(counter_dev=counter_dev, children_dev=children_dev, capacity=1, child_side=child_side, thr=thr, **children)
        return lib.hu_assembly_mass_cells(cells_abi.launch(**dict(held, **broken)), listed, 1, acc)

    def leaf_call(acc=p, **broken):
        return lib.hu_assembly_mass_leaf(cells_abi.launch(**dict(held, **broken)), acc)

    common = [{"table_dev": None}, {"parents_dev": None}, {"n_parents_dev": None}, {"evaluations_dev": None}, {"acc": None}, NULL_RECORD,
              {"n": 0}, {"n": 65}, {"dims": (0, 8, 8)}, {"dims": (8, 65537, 8)}, {"dims": (8, 8, 65537)}, {"dims": (7132, 7132, 7132)},
              {"step": float("nan")}, {"step": -1.0}]
    for kwargs in common + [{"child_side": 2}, {"child_side": 12}, {"child_side": 32768}, {"thr": -1.0}, {"thr": float("nan")},
                            {"counter_dev": None}, {"children_dev": None}, {"children": NULL_RECORD}]:
        assert cells_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    for kwargs in common:
        assert leaf_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    assert leaf_call(**NULL_RECORD) == -3 and b"NULL" in lib.hu_last_error()


def test_the_kernels_keep_their_records_in_scalar_registers(tmp_path):
    """What tests/test_section_host.py asks of the section's kernels, of every instantiation of these: no scratch; no
    vector-memory load (arguments, the table, a cell's row, the records and constants of a program are wave-uniform); the
    interpreter's fetch groups as wide scalar loads off a pointer that was itself loaded from memory; the rows leave
    through ordinary vector stores and the sums through 64-bit vector atomics."""
    from codecad_amd.hip_util import builder
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    assert "instance_mass.hip" in builder.SOURCES and "instance_mass.hip" not in builder.FLAGGED_SOURCES
    out = tmp_path / "instance_mass.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_mass.hip")], check=True, capture_output=True)
    text = out.read_text()
    seen = set()
    for chunk in re.split(r"\n(?=_Z\w+:\s+; @)", text):
        m = re.match(r"(_Z\w+):", chunk)
        if not m or "k_mass_" not in m.group(1):
            continue
        name, variant = re.search(r"(k_mass_\w+?)ILb([01])EE", m.group(1)).groups()
        seen.add((name, variant))
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
        assert {"global_atomic_add_x2", "global_atomic_umin", "global_atomic_umax"} <= stores
        assert ("global_store_dwordx4" in stores) == (name == "k_mass_cells")
    assert seen == {(k, v) for k in ("k_mass_cells", "k_mass_leaf") for v in "01"}
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", text.split(".amdgpu_metadata")[1])) >= 4
