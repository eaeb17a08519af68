"""separation() without a device: the reference traversal of separation_scenes.py against the dense definition on every
scenario (so the branch and bound, as specified, loses no minimum and no witness), what the numbers bound, that the
pruning prunes, the refusals and the empty reports, and the resources of the kernels from their metadata."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.hip_util import _lib

import separation_scenes as scenes

sep = sys.modules["codecad_amd.separation"]            # (the package's attribute of that name is the function)


def same(dense, traversal):
    return numpy.array_equal(dense.keys, traversal.keys) and dense.witness == traversal.witness


@pytest.mark.parametrize("name", scenes.NAMES)
def test_the_traversal_finds_the_dense_minimum_and_witness(name):
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    dense, traversal = scenes.dense_reference(name), scenes.traversal_reference(name)
    n = len(instances)
    assert same(dense, traversal)
    assert set(dense.witness) == {(i, j) for i in range(n) for j in range(i + 1, n)}       # every pair has a sample
    assert traversal.side == sep.top_side(dims) and len(traversal.level_rows) == len(cc._instance_cells.levels(traversal.side, 1, None)[0])


@pytest.mark.parametrize("name", scenes.FORCED)
def test_the_result_does_not_depend_on_the_top_side(name):
    dense = scenes.dense_reference(name)
    for side in (16, 64, 256):
        traversal = scenes.traversal_reference(name, side)
        assert same(dense, traversal) and traversal.side == side and len(traversal.level_rows) == {16: 1, 64: 2, 256: 3}[side]
    for cells in (1, 512):
        assert same(dense, scenes.traversal_reference(name, None, cells))
    assert scenes.traversal_reference(name, None, 1).side == {"rims": 16, "spheres": 256, "random_1": 256}[name]      # one cell


def test_the_modules_helpers_are_the_references(monkeypatch):
    for dims in ([13, 9, 11], [91, 82, 72], [4000, 1861, 1861], [65536, 65536, 65536]):
        assert sep.top_side(numpy.array(dims)) == scenes.top_side(dims)
        monkeypatch.setattr(sep, "_MAX_TOP_CELLS", 1)
        assert sep.top_side(numpy.array(dims)) == scenes.top_side(dims, 1)
        monkeypatch.undo()
    assert sep._MAX_TOP_CELLS == 512 and sep.top_side(numpy.array([128, 128, 128])) == 16 and sep.top_side(numpy.array([129, 128, 128])) == 64
    for child in (4, 16, 64, 16384):
        for step in (0.05, 1e-3, 0.3):
            assert sep.radius(child, numpy.float32(step)).view(numpy.uint32) == scenes.radius(child, numpy.float32(step)).view(numpy.uint32)
    rows = sep.top_rows(33, numpy.array([40, 16, 17]), 16)
    assert rows.tolist() == [[x | (0 << 16), z, 0xffffffff, 1] for x in (0, 16, 32) for z in (0, 16)]
    keys = scenes.order_keys(numpy.array([-1.5, -0.0, 0.0, 2.0 ** -149, 3.25], dtype=numpy.float32))
    assert list(keys) == sorted(keys) and keys[1] == keys[2]
    assert [sep.key_to_float(int(k)) for k in keys] == [-1.5, 0.0, 0.0, 2.0 ** -149, 3.25] and sep.key_to_float(0xffffffff) is None
    assert not numpy.signbit(sep.key_to_float(int(keys[1])))
    assert sep.gap_bounds(numpy.float32(0.25), numpy.float32(0.5)) == (0.5 - 0.5 * math.sqrt(3), 0.5)


@pytest.mark.parametrize("name, gap", (("spheres", scenes.SPHERES_GAP), ("boxes", scenes.BOXES_GAP)))
def test_gap_bounds_contain_the_closed_form_gap(name, gap):
    asm, resolution, instances, corner, step, dims = scenes.scene(name)
    traversal = scenes.traversal_reference(name)
    lo, hi = sep.gap_bounds(scenes.key_value(traversal.keys[0, 1]), step)
    assert lo <= gap <= hi and abs((hi - lo) - float(step) * math.sqrt(3)) < 1e-12


def test_the_boxes_tie_over_a_plane_and_the_witness_is_the_first():
    asm, resolution, instances, corner, step, dims = scenes.scene("boxes")
    w = scenes.fields("boxes")
    dense = scenes.dense_reference("boxes")
    keys = scenes.order_keys(scenes.pair_value(w[0], w[1]))
    ties = numpy.argwhere(keys == dense.keys[0, 1])
    assert len(ties) >= 100 and len(set(ties[:, 0])) <= 2                      # a plane of samples, or two by symmetry
    assert dense.witness[(0, 1)] == tuple(ties[0]) == tuple(ties.min(axis=0)) and tuple(ties[0]) != tuple(ties[-1])


@pytest.mark.parametrize("name", scenes.NAMES)
def test_negative_exactly_where_samples_lie_inside_both(name):
    dense, traversal = scenes.dense_reference(name), scenes.traversal_reference(name)
    negative = {pair for pair in dense.witness if scenes.key_value(traversal.keys[pair]) < 0}
    assert negative == {pair for pair, count in dense.inside_both.items() if count > 0}
    if name in ("lens", "gears", "solids64"):
        assert negative


def test_the_rims_clip_q_and_solids64_fills_the_mask():
    dims = scenes.scene("rims")[5]
    assert all(int(d) % 4 for d in dims) and (numpy.minimum(numpy.array([12, 8, 8]) + 2, dims - 1) == dims - 1).all()
    assert len(scenes.scene("solids64")[2]) == 64 and len(scenes.dense_reference("solids64").witness) == 2016


def test_pruning_is_not_vacuous():
    """The two balls at 4000 samples along x (4000 x 1861 x 1861, 1.39e10 samples, 2.77e10 dense evaluations): the reference
    traversal evaluates 3,627,640 samples, 1.3e-4 of the dense count, from 16 top cells of side 1024, and lists
    (1024, 512, 1543, 12692) rows."""
    asm, resolution, dims, traversal = scenes.fine_spheres()
    assert dims.max() >= 4000
    print("evaluations", traversal.evaluations, "of", int(numpy.prod(dims)) * 2, "rows", traversal.level_rows)
    assert traversal.evaluations <= 1e-3 * float(numpy.prod(dims)) * 2
    lo, hi = sep.gap_bounds(scenes.key_value(traversal.keys[0, 1]), numpy.float32(resolution))
    assert lo <= scenes.SPHERES_GAP <= hi
    x, y, z = traversal.witness[(0, 1)]
    assert abs(x - 0.5 * (dims[0] - 1)) <= 2 and abs(y - 0.5 * (dims[1] - 1)) <= 2 and abs(z - 0.5 * (dims[2] - 1)) <= 2


def test_argument_checks_and_empty_reports_need_no_device():
    disc = shapes.circle(1).make_part("disc")
    with pytest.raises(ValueError, match="3D"):
        cc.separation(cc.assembly("flat", [disc, disc.translated_x(1)]), 0.1)
    ball = shapes.sphere(1).make_part("ball")
    with pytest.raises(ValueError, match="64"):
        cc.separation(cc.assembly("crowd", [ball.translated_x(i) for i in range(65)]), 0.1)
    pair = cc.assembly("pair", [ball, ball.translated_x(1)])
    for bad in (0, -0.1, float("nan"), float("inf"), "0.1", None):
        with pytest.raises(ValueError, match="resolution"):
            cc.separation(pair, bad)
    with pytest.raises(ValueError, match="65536"):
        cc.separation(pair, 1e-5)
    with pytest.raises(ValueError, match="assembly"):
        cc.separation(shapes.sphere(1), 0.1)
    for asm, n in ((cc.assembly("one", [ball, ball.hidden()]), 1), (cc.assembly("none", [ball.hidden()]), 0)):
        r = cc.separation(asm, 0.1)
        assert isinstance(r, cc.SeparationReport) and len(r.instances) == n
        assert r.pairs == [] and r.samples_evaluated == 0 and r.traversals == 0 and r.level_rows == ()
    assert cc.SeparationReport._fields == ("instances", "corner", "step", "dims", "pairs", "samples_evaluated", "traversals", "level_rows")
    assert cc.PairSeparation._fields == ("i", "j", "separation", "witness", "witness_point", "gap_bounds")
    assert {"separation", "SeparationReport", "PairSeparation"} <= set(cc.__all__)


def test_abi_of_the_new_entry_points():
    declared = _lib.header_symbols()
    with open(_lib.HEADER) as f:
        header = f.read()
    for name in ("hu_separation_cells", "hu_separation_leaf", "hu_separation_witness"):
        assert name in declared and name in _lib.PROTOTYPES
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(_lib.PROTOTYPES[name]) == len(proto.split(","))
        assert _lib.PROTOTYPES[name][0] == ctypes.POINTER(_lib.CellsLaunch)
        assert [a.split()[-1] for a in proto.split(",")][-2:] == ["top_side", "acc_dev"]
    assert _lib.PROTOTYPES["hu_separation_cells"][1] == ctypes.POINTER(_lib.CellsChildren)


def documented_vgprs():
    with open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")) as f:
        m = re.search(r"`k_gap_cells` (\d+) \(full programs\) and (\d+) \(distance-only\), `k_gap_leaf` (\d+) and (\d+), "
                      r"`k_gap_witness` (\d+) and (\d+) VGPRs", f.read())
    assert m, "DESIGN.md section 9 states the VGPR counts of the six instantiations"
    counts = [int(v) for v in m.groups()]
    return {(k, v): counts[2 * a + b] for a, k in enumerate(("k_gap_cells", "k_gap_leaf", "k_gap_witness")) for b, v in enumerate("01")}


def test_the_kernels_use_no_scratch_and_the_registers_the_design_states(tmp_path):
    """Resources only, from the metadata of the six instantiations compiled for gfx950 (test_assembly_voxels_host.py reads
    its kernels' alike): a private segment of 0 bytes and the VGPR counts written in DESIGN.md."""
    from codecad_amd.hip_util import builder
    assert "instance_gap.hip" in builder.SOURCES and "instance_gap.hip" not in builder.FLAGGED_SOURCES
    hipcc = builder.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc in this environment")
    out = tmp_path / "instance_gap.s"
    flags = [f for f in builder.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I", builder.INCLUDE, "--cuda-device-only", "-S", "-o", str(out),
                                      os.path.join(builder.CSRC, "instance_gap.hip")], check=True, capture_output=True)
    metadata = out.read_text().split(".amdgpu_metadata")[1]
    found = {}
    for block in metadata.split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"(k_gap_\w+?)ILb([01])EE", name)
        assert m, name
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        found[m.groups()] = int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1))
    assert found == documented_vgprs()
