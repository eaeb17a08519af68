"""The reference and the scenarios of test_gpu_assembly_components.py, and the host side of assembly_components() and
cavities(), checked without a device.

assembly_components_scenes.reference_components labels by a flood fill; that a second, independent labelling (repeated
min-propagation to a fixed point) gives the same labels on every scenario is the first test.  Every scenario is then
inspected: the edge it was built for is IN THE REFERENCE, as numbers."""
import os
import re
import subprocess
import sys
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.hip_util import _lib

import assembly_components_scenes as scenes
from assembly_components_scenes import SCENES, CASES, scene, reference, part_ids, EMPTY_SPACE, SOLID, NONE, TILE, EMPTY

ac = sys.modules["codecad_amd.assembly_components"]    # (the package's attribute of that name is the function)
av = sys.modules["codecad_amd.assembly_voxels"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_comp_local<true>", "k_comp_local<false>", "k_comp_merge_faces", "k_comp_merge_all", "k_comp_flatten", "k_comp_roots",
           "k_comp_stats", "k_comp_finish")


def closed(name, of=EMPTY_SPACE):
    return [c for c in reference(name, of).components if not c.touches_border]


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_labels_of_a_small_lattice_by_hand():
    s = numpy.array([[[1, 1, 0, 1]], [[0, 1, 0, 0]], [[1, 0, 0, 1]]], dtype=bool)          # 3 x 1 x 4
    n = NONE
    assert scenes.flood_labels(s).ravel().tolist() == [0, 0, n, 3, n, 0, n, n, 8, n, n, 11]
    assert scenes.propagated_labels(s).ravel().tolist() == [0, 0, n, 3, n, 0, n, n, 8, n, n, 11]
    ids = numpy.where(s, EMPTY, 2).astype(numpy.uint8)
    ids[1, 0, 2] = 5
    ref = scenes.reference_components(ids, EMPTY_SPACE)
    assert [tuple(c) for c in ref.components] == [(0, 3, ((0, 0, 0), (1, 0, 1)), (1, 0, 2), True, (2, 5)),
                                                  (3, 1, ((0, 0, 3), (0, 0, 3)), (0, 0, 3), True, (2,)),
                                                  (8, 1, ((2, 0, 0), (2, 0, 0)), (2, 0, 0), True, (2,)),
                                                  (11, 1, ((2, 0, 3), (2, 0, 3)), (2, 0, 3), True, (2,))]
    solid = scenes.reference_components(ids, SOLID)
    assert [(c.label, c.count, c.parts) for c in solid.components] == [(2, 5, (2, 5)), (4, 1, (2,))]


@pytest.mark.parametrize("name,of", CASES)
def test_the_flood_fill_agrees_with_min_propagation(name, of):
    ref = reference(name, of)
    in_set = (ref.ids == EMPTY) if of == EMPTY_SPACE else (ref.ids != EMPTY)
    assert numpy.array_equal(scenes.propagated_labels(in_set), ref.labels)
    assert ((ref.labels == NONE) == ~in_set).all()
    assert sum(c.count for c in ref.components) == int(in_set.sum())
    assert [c.label for c in ref.components] == sorted(c.label for c in ref.components)
    assert max(scene(name)[5]) < 100


# ---- the scenarios hold what they are for -----------------------------------------------------------------------------

def test_the_shell_has_one_cavity_and_spans_three_tiles_an_axis():
    dims = [int(d) for d in scene("shell")[5]]
    assert dims == [scenes.SHELL_SAMPLES] * 3 and all(d > 2 * t and d % t for d, t in zip(dims, TILE))
    (cavity,) = closed("shell")
    assert cavity.parts == (0,)
    corner, step = scene("shell")[3:5]
    at = [float(corner[k]) + float(step) * numpy.arange(dims[k]) for k in range(3)]
    inner = at[0][:, None, None] ** 2 + at[1][None, :, None] ** 2 + at[2][None, None, :] ** 2 < 1.0    # within the shell's wall
    assert cavity.count == int(((part_ids("shell") == EMPTY) & inner).sum()) == 5904     # every empty sample inside the shell


def test_two_cups_enclose_a_void_only_together():
    (cavity,) = closed("two_cups")
    assert cavity.parts == (0, 1) and cavity.count == 8 ** 3 and cavity.box == ((4, 4, 4), (11, 11, 11))
    assert [i.name for i in scene("two_cups")[2]] == ["lower", "upper"] and [i.name for i in scene("one_cup")[2]] == ["lower"]
    assert closed("one_cup") == [] and len(reference("one_cup").components) == 1
    assert reference("one_cup").components[0].count == 8 * 8 * 4


def test_the_serpentine_crosses_tile_faces_and_starts_at_its_far_end():
    ref = reference("serpentine")
    assert [int(d) for d in scene("serpentine")[5]] == list(scenes.SERPENTINE)
    (channel,) = ref.components
    assert not channel.touches_border and channel.parts == (0,)
    runs, wide = scenes.RUNS, 2 * 2
    assert runs - 1 >= 6                                                          # turns
    assert channel.count == runs * wide * 36 + (runs - 1) * 2 * 2 * 2            # the runs and what the joints add between them
    assert TILE == (8, 8, 16)
    # every run crosses z = 15|16 and 31|32; the joints 0, 2, 4 cross x = 7|8, 15|16, 23|24; nothing crosses a y face
    crossings = runs * 2 + 3
    assert scenes.face_pairs(ref.labels == channel.label) == crossings * wide == 68
    # the least index is the free end of run 0, the rest of the channel lies up to 26 samples further along x
    first = numpy.unravel_index(channel.label, ref.labels.shape)
    assert tuple(int(v) for v in first) == (4, 5, 4) and channel.box == ((4, 5, 4), (29, 6, 39))
    open_ = reference("serpentine_open")
    (joined,) = open_.components
    assert joined.touches_border and joined.count == channel.count + 2 * 2 * 4 and closed("serpentine_open") == []


def test_diagonal_contact_does_not_connect():
    assert [(c.count, c.box) for c in closed("diagonal")] == [(int(numpy.prod(numpy.subtract(hi, lo))), (lo, tuple(h - 1 for h in hi)))
                                                              for lo, hi in scenes.DIAGONAL_VOIDS]
    assert len(reference("diagonal").components) == 4
    a, b = reference("diagonal_solid", SOLID).components
    assert (a.count, a.parts, b.count, b.parts) == (512, (0,), 512, (1,))
    ids = part_ids("diagonal_solid")
    assert ids[7, 7, 0] == 0 and ids[8, 8, 0] == 1 and ids[7, 8, 0] == EMPTY == ids[8, 7, 0]


def test_rims_have_a_padded_run_and_no_empty_sample():
    dims = [int(d) for d in scene("rims")[5]]
    assert dims == [13, 9, 11] and all(d % 4 for d in dims) and av.volume_shape(dims, 2 ** 32)[2] == 16 > dims[2]
    assert reference("rims", EMPTY_SPACE).components == []
    (block,) = reference("rims", SOLID).components
    assert block.count == 13 * 9 * 11 and block.label == 0 and block.touches_border and block.parts == (0,)


def test_the_bubbles_straddle_faces_and_corners():
    ref = reference("bubbles")
    assert len(ref.components) == 125 == len(closed("bubbles")) and all(c.count == 8 and c.parts == (0,) for c in ref.components)
    assert [int(d) for d in scene("bubbles")[5]] == [47, 47, 47]
    corners = [c for c in ref.components if all((lo + 1) % t == 0 for lo, t in zip(c.box[0], TILE))]
    assert len(corners) == 5 * 5 * 2                                              # every x and y, z = 15|16 and 31|32
    assert scenes.face_pairs(ref.labels != NONE) == 125 * 4 * 2 + 50 * 4


def test_the_solid_scenes():
    box, ball = reference("coarse_64", SOLID).components
    assert box.parts == (0,) and ball.parts == (1,) and box.count > ball.count > 0
    ref = reference("solids64", SOLID)
    owners = set(numpy.unique(ref.ids[ref.ids != EMPTY]).tolist())
    assert 63 in owners
    listed = [k for c in ref.components for k in c.parts]
    assert sorted(listed) == sorted(owners)                                       # the masks partition the owners
    (space,) = reference("heavy_pair25").components
    assert space.touches_border and len(space.parts) >= 2


# ---- the driver, on the host -----------------------------------------------------------------------------------------

def test_refusals():
    ball = shapes.sphere(r=1).make_part("ball")
    for bad in ("void", None, 0, "SOLID"):
        with pytest.raises(ValueError):
            cc.assembly_components(cc.assembly("one", [ball]), 0.5, of=bad)
    with pytest.raises(ValueError):
        cc.assembly_components(cc.assembly("flat", [shapes.circle(r=1).make_part("disc")]), 0.1)
    with pytest.raises(TypeError):
        cc.cavities(cc.assembly("one", [ball]), 0.5, of=SOLID)
    asm, resolution = scene("rims")[:2]
    with pytest.raises(ValueError):                                # both volumes count: 5 bytes a sample, before any launch
        cc.assembly_components(asm, resolution, max_bytes=5 * 13 * 9 * 16 - 1)
    rod = cc.assembly("long", [shapes.box(40000 * 0.01, 300 * 0.01, 300 * 0.01).make_part("rod")])
    with pytest.raises(ValueError, match="2\\^31"):                # 40000 x 300 x 304 entries
        cc.assembly_components(rod, 0.01, max_bytes=2 ** 40)
    assert {"assembly_components", "cavities", "ComponentsReport", "CavityReport", "EMPTY_SPACE", "SOLID"} <= set(cc.__all__)


def test_no_visible_instance_gives_an_empty_report():
    ghost = shapes.box(1).make_part("ghost").hidden()
    report = cc.assembly_components(cc.assembly("nothing", [ghost]), 0.1, max_bytes=80)
    assert report.components == [] and report.component_capacity_runs == 0 and report.traversals == 0
    assert report.labels.shape == (1, 1, 1) and report.labels.dtype == numpy.uint32 and report.labels[0, 0, 0] == NONE
    found = cc.cavities(cc.assembly("nothing", [ghost]), 0.1)
    assert found.cavities == [] and found.sealed_volume == 0 and found.components_report.part_ids[0, 0, 0] == EMPTY
    with pytest.raises(ValueError):
        cc.assembly_components(cc.assembly("nothing", [ghost]), 0.1, max_bytes=79)


def fake_device(monkeypatch, n_components):
    """assembly_components() over a library that records its calls and a table with `n_components` roots."""
    calls = []

    class Buffer:
        def __init__(self, dtype, shape, queue=None):
            self.dtype, self.shape = numpy.dtype(dtype), tuple(shape)
            self.size = int(numpy.prod(shape)) * self.dtype.itemsize
            self.device_ptr = 0x1000 * (1 + len([c for c in calls if c[0] == "buffer"]))
            calls.append(("buffer", self.dtype, self.shape))

        def read(self):
            out = numpy.zeros(self.shape, self.dtype)
            if self.dtype == ac._ROW:
                out[:1].view(numpy.uint32)[0] = n_components
                for k in range(1, len(out)):
                    out[k] = (k, (k, 2 * k, 3 * k), 1 << (k % 2), (0xffffffff - 1,) * 3, (2, 3, 4), 100000 - k, k % 2)
            elif self.dtype == numpy.uint32:
                out[...] = 7
            return out

        def release(self):
            calls.append(("release", self.shape))

    class Lib:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name, args))
                return 0
            return call

    def traverse(inst, top, side, c, s, d, initial_capacity, **kwargs):
        calls.append(("traverse", initial_capacity, kwargs["cells_extra"][0]))
        return 77, numpy.array([5, 6, 999], dtype=numpy.uint64), 2

    manager = types.SimpleNamespace(lib=Lib(), queue=types.SimpleNamespace(handle=0x99))
    monkeypatch.setattr(av, "hip_manager", manager)
    monkeypatch.setattr(ac, "hip_manager", manager)
    monkeypatch.setattr(av.hip_util, "Buffer", Buffer)
    monkeypatch.setattr(av.cells, "traverse", traverse)
    return calls


def test_the_driver_keeps_the_volume_and_regrows_the_table_by_running_the_statistics_alone(monkeypatch):
    asm, resolution = scene("rims")[:2]
    calls = fake_device(monkeypatch, 3)
    report = cc.assembly_components(asm, resolution, of=SOLID, local=False, initial_components=2, initial_capacity=7,
                                    max_bytes=5 * 13 * 9 * 16)
    monkeypatch.undo()
    names = [c[0] for c in calls]
    assert names == ["buffer", "hu_memset", "traverse", "buffer", "hu_components_local", "hu_components_merge", "hu_components_flatten",
                     "buffer", "hu_memset", "hu_components_stats", "release",
                     "buffer", "hu_memset", "hu_components_stats", "release",        # the table regrown: the statistics alone
                     "release", "hu_components_finish", "release"]
    assert calls[2][1:] == (7, 1)                                                    # retire=True, the cell lists' capacity
    volume, labels = 0x1000, 0x2000
    dims = lambda a: list(a)                                                         # noqa: E731
    local = calls[4][1]
    assert (local[0], local[1], dims(local[2]), local[3:]) == (volume, labels, [13, 9, 11], (16, 1, 0, 0x99))
    assert calls[5][1][0] == labels and calls[5][1][2:] == (16, 0, 0x99) and calls[6][1][2:] == (16, 0x99)
    assert calls[3][1:] == (numpy.dtype(numpy.uint32), (13, 9, 16))
    first, second = calls[9][1], calls[13][1]
    assert calls[7][2] == (3,) and calls[11][2] == (4,)                              # capacity 2, then the count: a row more each
    assert calls[8][1] == (0x3000, 0, 3 * 72, 0x99) and calls[12][1] == (0x4000, 0, 4 * 72, 0x99)
    assert first[:2] == (volume, labels) and first[3:] == (16, 1, 1, 0x3000, 0x3000 + 72, 2, 0x99)
    assert second[3:] == (16, 1, 0, 0x4000, 0x4000 + 72, 3, 0x99)                    # slots are not assigned twice
    assert report.component_capacity_runs == 2 and report.traversals == 2 and report.samples_evaluated == 77
    assert report.labels.shape == (13, 9, 11) and (report.labels == 7).all() and report.part_ids.shape == (13, 9, 11)
    assert [c.label for c in report.components] == [99997, 99998, 99999]                      # ordered by label
    c = report.components[0]                                                         # (row 3 of the table)
    assert (c.count, c.index_sums, c.box, c.touches_border, c.parts) == (3, (3, 6, 9), ((1, 1, 1), (2, 3, 4)), True, (1,))
    step, corner = float(report.step), [float(v) for v in report.corner]
    assert c.volume == 3 * step ** 3 and tuple(c.centroid) == tuple(corner[k] + step * c.index_sums[k] / 3 for k in range(3))


def test_a_table_that_holds_every_root_runs_the_statistics_once(monkeypatch):
    asm, resolution = scene("rims")[:2]
    calls = fake_device(monkeypatch, 3)
    found = cc.cavities(asm, resolution)
    monkeypatch.undo()
    assert [c[0] for c in calls].count("hu_components_stats") == 1 and found.components_report.component_capacity_runs == 1
    stats = [c for c in calls if c[0] == "hu_components_stats"][0][1]
    assert stats[4:6] == (0, 1) and stats[8] == min(4096, 13 * 9 * 16)                # empty space; slots assigned
    assert [c.label for c in found.cavities] == [99998] and found.cavities[0].enclosed_by == ("block",)
    assert found.sealed_volume == found.cavities[0].volume


# ---- the C ABI and the kernels' resources -----------------------------------------------------------------------------

def test_abi_of_the_new_entry_points():
    lib = _lib.load()
    declared = _lib.header_symbols()
    with open(_lib.HEADER) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    for name in ("hu_components_local", "hu_components_merge", "hu_components_flatten", "hu_components_stats", "hu_components_finish"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(_lib.PROTOTYPES[name]) == len(proto.split(","))
        assert ("int %s(" % name) in integration
    tile = tuple(int(re.search(r"#define HU_COMPONENTS_TILE_%s (\d+)" % axis, header).group(1)) for axis in "XYZ")
    assert tile == TILE and TILE[2] % 16 == 0
    assert int(re.search(r"#define HU_COMPONENTS_ROW_BYTES (\d+)", header).group(1)) == ac._ROW.itemsize


def documented_resources():
    """{kernel: (VGPRs, LDS bytes)} as DESIGN.md states them."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    found = {}
    for name in KERNELS:
        m = re.search(r"`%s` (\d+) VGPRs and (\d+) B of LDS" % re.escape(name), text)
        assert m, "DESIGN.md section 9 states the VGPRs and the LDS of " + name
        found[name] = (int(m.group(1)), int(m.group(2)))
    return found


def test_the_kernels_use_no_scratch_and_the_resources_the_design_states(tmp_path):
    """Resources only, from the metadata of the unit compiled for gfx950: a private segment of 0 bytes, and the VGPR counts
    and LDS sizes written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_components.hip" in builder.SOURCES and "instance_components.hip" not in builder.FLAGGED_SOURCES
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_components.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_components.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"(k_comp_[a-z_]+?)(?:ILb([01])EE)?Ev?NS_8CompArgsE", name)
        assert m, name
        kernel = m.group(1) + ({"1": "<true>", "0": "<false>"}[m.group(2)] if m.group(2) else "")
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[kernel] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)))
    assert found == documented_resources()
