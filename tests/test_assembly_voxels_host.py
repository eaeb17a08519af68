"""The reference and the scenarios of test_gpu_assembly_voxels.py, and the host side of assembly_voxels(), checked without a
device.

assembly_voxels_scenes.reference_voxels has two halves, the dense definition and the traversal of csrc/instance_voxels.hip
done in NumPy; that both give the same volume and counts on every scenario is the first test.  Every scenario is then
inspected: the edge it was built for is IN THE REFERENCE."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, rendering, _instance_cells
from codecad_amd.hip_util import _lib

import assembly_mass_scenes as mass_scenes
import cells_abi
import assembly_voxels_scenes as scenes
from assembly_voxels_scenes import SCENES, scene, reference, EMPTY

av = sys.modules["codecad_amd.assembly_voxels"]        # (the package's attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_dense_ids_of_a_small_lattice_by_hand():
    inside = [numpy.array([[[True, True, False, False]]]), numpy.array([[[False, True, True, False]]])]
    ids, counts = scenes.dense_ids(inside)
    assert ids.dtype == numpy.uint8 and ids.ravel().tolist() == [0, 0, 1, 255] and counts == [2, 1]
    assert scenes._top_bit(numpy.array([1, 6, 1 << 63, 0], dtype=numpy.uint64)).tolist() == [0, 2, 63, 0]


@pytest.mark.parametrize("retire", [True, False])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_traversal_writes_the_dense_volume_and_the_premise_holds(name, retire):
    ref = reference(name, retire)
    assert numpy.array_equal(ref.written, ref.ids) and ref.traversal_counts == ref.counts
    assert ref.counts == [int((ref.ids == k).sum()) for k in range(len(ref.counts))]
    assert ref.premise_broken == 0
    assert (ref.ids[~ref.touched] == EMPTY).all()                 # what is never written is the prefill
    dense = mass_scenes.reference(name, retire)
    assert ref.counts == [o[0] for o in dense.owned] and sum(ref.counts) == dense.union_count > 0
    if not retire:
        assert all(level.retired == 0 and level.listed_capped == 0 for level in ref.levels) and ref.leaf.capped == 0
        assert ref.evaluations <= dense.evaluations               # (ascending order stops nothing without a full candidate)
    else:
        assert ref.evaluations <= reference(name, False).evaluations
        assert ref.evaluations <= dense.evaluations               # the owner rule never evaluates more than the mass rule


def test_a_repeated_traversal_rewrites_the_same_bytes():
    """What a cell writes depends on the cell alone, and a list that overflowed holds a subset of the rows of the full one:
    a traversal cut to 32 rows a list touches fewer samples, and every byte it writes is the byte of the dense volume --
    which the full traversal then writes again."""
    asm, resolution, instances, corner, step, dims = scene("gears")
    full = reference("gears")
    cut = scenes.reference_voxels(instances, corner, step, dims, True, w=mass_scenes._fields("gears"), capacity=32)
    assert 0 < cut.touched.sum() < full.touched.sum() and not (cut.touched & ~full.touched).any()
    assert numpy.array_equal(cut.written[cut.touched], full.ids[cut.touched])
    assert (cut.written[~cut.touched] == EMPTY).all()
    assert max(level.listed for level in full.levels) > 32 and cut.evaluations < full.evaluations


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def test_the_sphere_retires_under_a_boundary_candidate():
    """The ball has index 0 and the core block lies inside it: a child deep in the ball that the block's surface crosses
    is owned by the ball whatever the block does there.  The mass rule keeps such a child (not every candidate is full)."""
    asm, resolution, instances, corner, step, dims = scene("sphere")
    assert [i.name for i in instances] == ["ball", "core"] and dims.tolist() == [32, 32, 32]
    ref = reference("sphere")
    assert [level.child for level in ref.levels] == [4]
    assert ref.levels[0].retired_under_boundary >= 1
    assert ref.levels[0].retired > mass_scenes.reference("sphere").levels[0].retired
    assert ref.evaluations < mass_scenes.reference("sphere").evaluations
    assert ref.counts[1] == 0 and ref.counts[0] > 0               # the core owns nothing


def test_coarse_levels_retire_with_wide_fills():
    for name, side in (("coarse_64", 64), ("coarse_256", 256), ("coarse_160", 256)):
        assert SCENES[name].side == side
        by_child = {level.child: level for level in reference(name).levels}
        assert sorted(by_child) == ([4, 16] if side == 64 else [4, 16, 64])
        assert by_child[16].retired >= 1 and by_child[4].retired >= 1
        assert by_child[16].filled_bytes >= 16 ** 3 and by_child[16].filled_bytes % 16 == 0
    assert {level.child: level.retired for level in reference("coarse_256").levels}[64] == 0
    big = {level.child: level for level in reference("coarse_160").levels}[64]
    assert big.retired >= 1 and big.filled_bytes == big.retired * 64 ** 3
    assert numpy.array_equal(reference("coarse_64").ids, reference("coarse_256").ids)


def test_rims_have_no_axis_a_multiple_of_four_and_a_padded_run():
    asm, resolution, instances, corner, step, dims = scene("rims")
    assert dims.tolist() == [13, 9, 11] and all(d % 4 for d in dims)
    assert av.volume_shape(dims, 2 ** 32) == (13, 9, 16)
    ref = reference("rims")
    assert (ref.ids == 0).all() and ref.counts == [13 * 9 * 11, 0]         # the ball lies inside the block


def test_the_reversed_orders_permute_the_ids():
    first = mass_scenes.OWNERSHIP_ORDERS[0]
    base = reference("ownership_%d%d%d" % first)
    inside_any = base.ids != EMPTY
    for order in mass_scenes.OWNERSHIP_ORDERS[1:]:
        ref = reference("ownership_%d%d%d" % order)
        assert numpy.array_equal(ref.ids != EMPTY, inside_any)              # the union does not change,
        part = numpy.array(order)                                          # index k of this order is part order[k]
        mine, theirs = part[ref.ids[inside_any]], numpy.array(first)[base.ids[inside_any]]
        assert (mine != theirs).any()                                      # the owners do,
        w = mass_scenes.reference("ownership_%d%d%d" % order).w
        lowest = numpy.full(ref.ids.shape, EMPTY, numpy.uint8)
        for k in reversed(range(3)):
            lowest[w[k] < 0] = k
        assert numpy.array_equal(ref.ids, lowest)                           # by the lowest index of THIS order
        assert sorted(set(ref.ids[inside_any].tolist())) == [0, 1, 2]


def test_solids64_has_owners_in_both_words_of_the_mask():
    ref = reference("solids64")
    assert len(ref.counts) == 64 and all(c > 0 for c in ref.counts[:32]) and sum(1 for c in ref.counts[32:] if c > 0) >= 8
    assert int(ref.ids[ref.ids != EMPTY].max()) >= 48
    assert ref.levels[0].retired > 0 and ref.leaf.capped > 0


def test_strictness_a_sample_on_a_face_is_not_inside():
    """In `strict` the outer box has index 0 and owns everything; with the outer box last, the samples ON the faces of the
    halves (w == 0 exactly) are seen to belong to it and not to a half."""
    ref = reference("strict")
    assert ref.counts[1] == 0 == ref.counts[2] and ref.counts[0] == sum(ref.counts) > 0
    asm, resolution, (right, left, outer), ref = scenes.strict_reversed()
    assert ref.ids.shape == (33, 33, 33) and numpy.array_equal(ref.written, ref.ids) and ref.premise_broken == 0
    on_a_face = ((right == 0) & ~(left < 0)) | ((left == 0) & ~(right < 0))
    assert on_a_face.sum() >= 6 * 15 * 15 and (ref.ids[on_a_face] == 2).all()
    assert ref.counts[0] == 15 ** 3 == ref.counts[1] and int((right <= 0).sum()) == 17 ** 3


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals_of_interference_and_the_size_bound():
    ball = shapes.sphere(r=1).make_part("ball")
    for bad in (0, -1.0, float("nan"), "fine"):
        with pytest.raises(ValueError):
            cc.assembly_voxels(cc.assembly("one", [ball]), bad)
    with pytest.raises(ValueError):
        cc.assembly_voxels(shapes.sphere(r=1), 0.1)
    with pytest.raises(ValueError):
        cc.assembly_voxels(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(ValueError):
        cc.assembly_voxels(cc.assembly("many", [ball.translated_x(3 * k) for k in range(65)]), 0.5)
    with pytest.raises(ValueError):                                # 70000 samples on an axis
        cc.assembly_voxels(cc.assembly("long", [shapes.box(700, 1, 1).make_part("rod")]), 0.01)
    assert av.volume_shape((13, 9, 11), 13 * 9 * 16) == (13, 9, 16) and av.volume_shape((5, 6, 32), 10 ** 9) == (5, 6, 32)
    with pytest.raises(ValueError):
        av.volume_shape((13, 9, 11), 13 * 9 * 16 - 1)
    asm, resolution, instances, corner, step, dims = scene("rims")
    with pytest.raises(ValueError):                                # before any launch
        cc.assembly_voxels(asm, resolution, max_bytes=13 * 9 * 16 - 1)


def test_no_visible_instance_gives_an_empty_volume():
    ghost = shapes.box(1).make_part("ghost").hidden()
    v = cc.assembly_voxels(cc.assembly("nothing", [ghost]), 0.1, max_bytes=16)
    assert v.instances == [] and v.counts == [] and v.traversals == 0 and v.samples_evaluated == 0
    assert v.part_ids.shape == (1, 1, 1) and v.part_ids.dtype == numpy.uint8 and v.part_ids[0, 0, 0] == EMPTY
    with pytest.raises(ValueError):
        cc.assembly_voxels(cc.assembly("nothing", [ghost]), 0.1, max_bytes=15)


def test_the_driver_prefills_once_and_passes_the_volume_to_both_entry_points(monkeypatch):
    """Without a device: the buffer is uint8[nx, ny, pz] at exactly max_bytes, filled with 255 by one hu_memset before the
    traversal; the cells level gets (retire, volume, pz) and then the accumulators, the finest level (volume, pz); the
    host returns the view [:, :, :nz] and the first n accumulators."""
    asm, resolution, instances, corner, step, dims = scene("rims")
    calls, made = [], []

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.shape, self.size, self.device_ptr = shape, int(numpy.prod(shape)), 0x4000
            assert numpy.dtype(dtype) == numpy.uint8
            made.append(self)

        def read(self):
            out = numpy.arange(self.size, dtype=numpy.uint32).astype(numpy.uint8).reshape(self.shape)
            return out

        def release(self):
            calls.append(("release",))

    class Lib:
        def hu_memset(self, *args):
            calls.append(("hu_memset", args))
            return 0

    def traverse(inst, top, side, c, s, d, initial_capacity, **kwargs):
        calls.append(("traverse", top, side, initial_capacity, kwargs))
        return 77, numpy.array([5, 6, 999], dtype=numpy.uint64), 2

    monkeypatch.setattr(av, "hip_manager", types.SimpleNamespace(lib=Lib(), queue=types.SimpleNamespace(handle=0x99)))
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    v = cc.assembly_voxels(asm, resolution, initial_capacity=7, retire=False, max_bytes=13 * 9 * 16)
    monkeypatch.undo()
    assert [c[0] for c in calls] == ["hu_memset", "traverse", "release"] and len(made) == 1 and made[0].shape == (13, 9, 16)
    assert calls[0][1] == (0x4000, 255, 13 * 9 * 16, 0x99)
    _, top, side, initial_capacity, kwargs = calls[1]
    assert side == 16 and initial_capacity == 7 and top.shape[1] == 4 and not (top[:, 1] >> 31).any()
    assert numpy.array_equal(top, _instance_cells.cell_rows(_instance_cells.windows(instances, corner, float(step), dims), dims, 16, least=1))
    assert kwargs["cells"] == "hu_assembly_voxels_cells" and kwargs["cells_extra"] == (0, 0x4000, 16)
    assert kwargs["finest"] == [("hu_assembly_voxels_leaf", (0x4000, 16))] and kwargs["accumulators"] == 3
    assert kwargs["pair_dtype"].itemsize == 8 and kwargs["pair_init"] == {} and "row_bytes" not in kwargs
    assert kwargs["thr"](4) == mass_scenes.threshold(4, step)
    assert v.part_ids.shape == (13, 9, 11) and numpy.array_equal(v.part_ids, made[0].read()[:, :, :11])
    assert v.counts == [5, 6] and all(type(c) is int for c in v.counts) and v.samples_evaluated == 77 and v.traversals == 2
    assert [i.name for i in v.instances] == ["block", "ball"]


def _hand_made():
    inst = _instance_cells.visible(mass_scenes._boxes(), 0.125)
    ids = numpy.full((3, 2, 2), EMPTY, dtype=numpy.uint8)
    ids[0, 0, 0], ids[1, 1, 0], ids[2, 0, 1] = 0, 1, 1
    return cc.AssemblyVoxels([_instance_cells.Instance(i.name, i) for i in inst], numpy.zeros(3, numpy.float32), numpy.float32(0.5),
                             numpy.array([3, 2, 2]), ids, [1, 2], 0, 1)


def test_helpers_of_the_result():
    v = _hand_made()
    assert v.mask(1).sum() == 2 and v.mask(1).dtype == bool and v.mask(0)[0, 0, 0]
    assert v.layer(1).shape == (3, 2) and v.layer(1).tolist() == [[255, 255], [255, 255], [1, 255]]
    assert v.volumes().dtype == numpy.float64 and v.volumes().tolist() == [0.125, 0.25]
    assert {"assembly_voxels", "AssemblyVoxels"} <= set(cc.__all__) and av.EMPTY == 255


def test_pixels_of_a_hand_made_volume():
    v = _hand_made()
    hues = rendering.assembly_picture.part_colors([i.instance for i in v.instances], "parts")
    px = rendering.render_assembly_voxel_pixels(v, 0)
    assert px.shape == (2, 3, 3) and px.dtype == numpy.uint8          # (ny, nx, 3), row 0 the greatest y
    colour = [numpy.rint(numpy.clip(h, 0, 1) * 255).astype(numpy.uint8).tolist() for h in hues]
    white = [255, 255, 255]
    assert px.tolist() == [[white, colour[1], white], [colour[0], white, white]]
    px = rendering.render_assembly_voxel_pixels(v, 1, colors=[(1, 0, 0), (0, 0, 1)], background=(0, 0, 0))
    assert px.tolist() == [[[0, 0, 0]] * 3, [[0, 0, 0], [0, 0, 0], [0, 0, 255]]]
    for bad in ({"z": 2}, {"z": -1}):
        with pytest.raises(IndexError):
            rendering.render_assembly_voxel_pixels(v, **bad)
    with pytest.raises(ValueError):
        rendering.render_assembly_voxel_pixels(v, 0, colors="rainbow")
    with pytest.raises(ValueError):
        rendering.render_assembly_voxel_pixels(v, 0, background=(2, 0, 0))


# ---- the C ABI and the kernels' resources -----------------------------------------------------------------------------

def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ("hu_assembly_voxels_cells", "hu_assembly_voxels_leaf"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        with open(_lib.HEADER) as f:
            proto = re.search(r"int %s\(([^;]*)\);" % name, f.read()).group(1)
        assert len(_lib.PROTOTYPES[name]) == len(proto.split(","))
        with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
            assert ("int %s(" % name) in f.read()
        assert _lib.PROTOTYPES[name][0] == ctypes.POINTER(_lib.CellsLaunch)
    assert _lib.PROTOTYPES["hu_assembly_voxels_cells"][1] == ctypes.POINTER(_lib.CellsChildren)
    buf = (ctypes.c_uint8 * 512)()
    p = (ctypes.addressof(buf) + 255) & ~255                       # aligned, as a volume must be
    held = cells_abi.held(p, (64, 64, 64))
    NULL_RECORD = cells_abi.NULL_RECORD

    def cells_call(child_side=4, thr=1.0, counter_dev=p, children_dev=p, children={}, volume=p, pitch=64, acc=p, **broken):
        listed = cells_abi.children(counter_dev=counter_dev, children_dev=children_dev, capacity=1, child_side=child_side, thr=thr, **children)
        return lib.hu_assembly_voxels_cells(cells_abi.launch(**dict(held, **broken)), listed, 1, volume, pitch, acc)

    def leaf_call(volume=p, pitch=64, acc=p, **broken):
        return lib.hu_assembly_voxels_leaf(cells_abi.launch(**dict(held, **broken)), volume, pitch, acc)

    unaligned = p + 4
    common = [{"table_dev": None}, {"parents_dev": None}, {"n_parents_dev": None}, {"evaluations_dev": None}, {"acc": None}, {"volume": None},
              NULL_RECORD, {"n": 0}, {"n": 65}, {"dims": (0, 8, 8)}, {"dims": (8, 65537, 8)}, {"dims": (8, 8, 65537)},
              {"step": float("nan")}, {"step": -1.0}, {"pitch": 48}, {"pitch": 72}, {"pitch": 0}, {"pitch": 65552}, {"volume": unaligned}]
    for kwargs in common + [{"child_side": 2}, {"child_side": 12}, {"child_side": 32768}, {"thr": -1.0}, {"thr": float("nan")},
                            {"counter_dev": None}, {"children_dev": None}, {"children": NULL_RECORD}]:
        assert cells_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    for kwargs in common:
        assert leaf_call(**kwargs) == -3, kwargs
        assert lib.hu_last_error()
    assert leaf_call(**NULL_RECORD) == -3 and b"NULL" in lib.hu_last_error()


def documented_vgprs():
    """{(kernel, distance-only): VGPRs} as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        m = re.search(r"`k_voxel_cells` (\d+) \(full programs\) and (\d+) \(distance-only\), `k_voxel_leaf` (\d+) and (\d+) VGPRs", f.read())
    assert m, "DESIGN.md section 9 states the VGPR counts of the four instantiations"
    a, b, c, d = (int(v) for v in m.groups())
    return {("k_voxel_cells", "0"): a, ("k_voxel_cells", "1"): b, ("k_voxel_leaf", "0"): c, ("k_voxel_leaf", "1"): d}


def test_the_kernels_use_no_scratch_and_the_registers_the_design_states(tmp_path):
    """Resources only, from the metadata of the four instantiations compiled for gfx950: a private segment of 0 bytes and
    the VGPR counts written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_voxels.hip" in builder.SOURCES and "instance_voxels.hip" not in builder.FLAGGED_SOURCES
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_voxels.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_voxels.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"(k_voxel_\w+?)ILb([01])EE", name)
        assert m, name
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[m.groups()] = int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1))
    assert found == documented_vgprs()
