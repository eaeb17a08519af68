"""The kernels over an assembly's cells at every workgroup shape cells_launch() can give them (csrc/instance_cells.hpp,
host.hpp hu_workgroup): 128 and 64 lanes through the genuine register files of heavy_instances.py, and 128 lanes, 64 lanes,
LDS above 64 KiB and the largest LDS that fits through a `lane_bytes` larger than the programs need (a valid argument: the
register file only has room to spare, and every offset still derives from it).  separation() keeps 4 bytes per instance
and lane behind the register file in all three of its kernels and its compaction scratch behind that: it runs on the heavy
scenes, padded from a forced top side of 256 (bounds of two levels) and padded with 64 instances, which start at 128 lanes
and take the regimes the rule leaves them.  Every comparison is the family's own, with
its own reference and its own `check`: exact, no tolerance anywhere.  test_cells_workgroup_shapes_host.py holds the table
of lanes per scene and kernel that the runs here are asserted to land on."""
import numpy
import pytest

import codecad_amd as cc
from codecad_amd import _instance_cells
from codecad_amd.section import Plane

import heavy_instances as hi
import assembly_mass_scenes as mass_scenes
import assembly_meshes_scenes as mesh_scenes
import layer_outlines_scenes as layer_scenes
import test_section_host as tsh
import test_section_outlines_host as tso
import test_gpu_section as gpu_section
import test_gpu_section_outlines as gpu_outlines
import test_gpu_layer_outlines as gpu_layers
import test_gpu_assembly_meshes as gpu_meshes
import test_gpu_assembly_mass as gpu_mass
import assembly_voxels_scenes as voxel_scenes
import separation_scenes as sep_scenes
import test_gpu_assembly_voxels as gpu_voxels
import test_gpu_separation as gpu_separation
from test_gpu_interference import device_pairs, dense_pairs
from test_gpu_clearance import device_near, dense_near
from test_instance_cells_reference_host import SCENARIOS as EDGE_SCENARIOS
from test_cells_workgroup_shapes_host import FIGURES, expected_lanes

pytestmark = pytest.mark.gpu

NAMES = sorted(hi.SCENES)


def landed(hip, name):
    """The device table's figures are the host's, and they give the lanes of the host file's table."""
    instances = hi.instances_of(name)
    table, distance_only, lane_bytes = _instance_cells.device_table(instances, hip.queue)
    table.release()
    assert (distance_only, lane_bytes) == FIGURES[name][:2] == hi.table_figures(instances)
    want = expected_lanes(name)
    assert {k: hi.cells_lanes(lane_bytes, e) for k, e in hi.kernel_extras(len(instances)).items()} == want
    return want


def small(name):
    return {"initial_capacity": 1} if name in ("heavy_pair", "heavy_64") else {}


# ---- genuine wide register files -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_interference_and_clearance(hip, name):
    want = landed(hip, name)
    assert want["interference leaf"] < 256 and want["clearance witness"] == FIGURES[name][3]
    asm, resolution, gap = hi.scene(name)
    pairs, _, _ = hi.pairs_reference(name, 0.0)
    near = hi.pairs_reference(name, gap)[1]
    assert pairs and near                                           # overlap and a near miss are the point of every scene
    inter = cc.interference(asm, resolution)
    close = cc.clearance(asm, resolution, gap)
    assert device_pairs(inter) == pairs and inter.pairs and inter.traversals == 1
    assert device_near(close) == near and close.pairs and close.traversals == 1
    if small(name):
        again, near_again = cc.interference(asm, resolution, **small(name)), cc.clearance(asm, resolution, gap, **small(name))
        assert device_pairs(again) == pairs and device_near(near_again) == near
        assert again.traversals > 1 and near_again.traversals > 1
        assert again.samples_evaluated == inter.samples_evaluated and near_again.samples_evaluated == close.samples_evaluated


@pytest.mark.parametrize("name", NAMES)
def test_section(hip, name):
    want = landed(hip, name)
    assert want["section tiles with distance"] == FIGURES[name][3] and want["section leaf"] < 256
    asm, resolution, _ = hi.scene(name)
    ref = hi.section_reference(name)
    for distance in (False, True):
        culled = cc.section(asm, hi.plane_of(name), resolution, distance=distance)
        gpu_section.check(culled, ref, distance)
        dense = cc.section(asm, hi.plane_of(name), resolution, distance=distance, cull=False)
        gpu_section.check(dense, ref, distance)
        assert culled.runs == dense.runs == 1
        if small(name):
            again = cc.section(asm, hi.plane_of(name), resolution, distance=distance, **small(name))
            gpu_section.check(again, ref, distance)
            assert again.runs > 1 and again.evaluations == culled.evaluations


@pytest.mark.parametrize("name", NAMES)
def test_section_outlines(hip, name):
    assert landed(hip, name)["outline leaf"] < 256
    asm, resolution, _ = hi.scene(name)
    ref = hi.outlines_reference(name)
    for cull in (True, False):
        o = cc.section_outlines(asm, hi.plane_of(name), resolution, cull=cull)
        gpu_outlines.check(o, ref, hi.outlines_traversal(name, cull).evaluations)
        assert o.runs == 1
    if small(name):
        o = cc.section_outlines(asm, hi.plane_of(name), resolution, initial_capacity=1, segment_capacity=1)
        gpu_outlines.check(o, ref, hi.outlines_traversal(name).evaluations)
        assert o.runs > 1


@pytest.mark.parametrize("name", NAMES)
def test_layer_outlines(hip, name):
    assert landed(hip, name)["layer leaf"] < 256
    asm, resolution, _ = hi.scene(name)
    plane, heights = hi.layers_of(name)
    ref = hi.layers_reference(name)
    for cull in (True, False):
        got = cc.layer_outlines(asm, plane, resolution, heights, cull=cull)
        gpu_layers.check(got, ref, hi.layers_traversal(name, cull).evaluations)
    if small(name):
        got = cc.layer_outlines(asm, plane, resolution, heights, initial_capacity=1, segment_capacity=1)
        gpu_layers.check(got, ref, hi.layers_traversal(name).evaluations)
        assert got.runs > 1


@pytest.mark.parametrize("name", NAMES)
def test_assembly_meshes(hip, name):
    assert landed(hip, name)["mesh leaf"] < 256
    asm, resolution, _ = hi.scene(name)
    instances, corner, step, dims = hi.lattice3(name)
    ref = hi.meshes_reference(name)
    m = cc.assembly_meshes(asm, resolution)
    gpu_meshes.check(m, ref, hi.meshes_traversal(name).evaluations)
    dense = cc.assembly_meshes(asm, resolution, cull=False)
    gpu_meshes.check(dense, ref, mesh_scenes.dense_evaluations(dims, len(instances)))
    if small(name):
        m = cc.assembly_meshes(asm, resolution, initial_capacity=1, triangle_capacity=1)
        gpu_meshes.check(m, ref, hi.meshes_traversal(name).evaluations)
        assert m.runs > 1


@pytest.mark.parametrize("name", NAMES)
def test_assembly_mass_properties(hip, name):
    assert landed(hip, name)["mass leaf"] < 256
    asm, resolution, _ = hi.scene(name)
    for retire in (True, False):
        ref = hi.mass_reference(name, retire)
        for how in [{}] + ([small(name)] if small(name) else []):
            report = cc.assembly_mass_properties(asm, resolution, retire=retire, **how)
            gpu_mass.check_against_dense(report, ref)
            assert report.samples_evaluated == ref.evaluations and (report.traversals > 1) == bool(how)


@pytest.mark.parametrize("name", NAMES)
def test_separation(hip, name):
    """The [wavefront][instance][lane] area and the compaction scratch behind it at 128 and at 64 lanes: 16 B per lane with
    the four instances of a pair, 256 B with heavy_64's."""
    want = landed(hip, name)
    assert want["separation cells"] == want["separation leaf"] == want["separation witness"] == FIGURES[name][3] < 256
    asm, resolution, _ = hi.scene(name)
    dense, traversal = hi.separation_reference(name)
    report = cc.separation(asm, resolution)
    gpu_separation.check(report, dense, traversal)
    assert report.traversals == 1
    if small(name):
        again = cc.separation(asm, resolution, **small(name))
        gpu_separation.check(again, dense, traversal)
        assert again.traversals > 1
        assert again.pairs == report.pairs and again.samples_evaluated == report.samples_evaluated and again.level_rows == report.level_rows


@pytest.mark.parametrize("name", NAMES)
def test_assembly_voxels(hip, name, monkeypatch):
    want = landed(hip, name)
    assert want["voxel cells"] == want["voxel leaf"] == FIGURES[name][2] < 256
    for retire in (True, False):
        ref = hi.voxels_reference(name, retire)
        voxels = gpu_voxels.run(name, monkeypatch, retire=retire)
        gpu_voxels.check_against_dense(voxels, ref)
        assert voxels.part_ids.tobytes() == ref.ids.tobytes()
        assert voxels.samples_evaluated == ref.evaluations and voxels.traversals == 1
        assert all(voxels.counts[k] > 0 for k in hi.HEAVY_INDEX[name])


# ---- every shape, by an over-sized register file -------------------------------------------------------------------------

REGIMES = hi.REGIMES


def pads(lane_bytes, extra, regimes=REGIMES):
    """{regime: pad, a multiple of 16} of `regimes`, and the first pad that no longer fits, from the rule itself."""
    def first(ok):
        return next(p for p in range(0, 4096, 16) if ok(lane_bytes + p, extra))

    out = {
        "128 lanes": lambda: first(lambda b, e: hi.cells_lanes(b, e) == 128),
        "64 lanes": lambda: first(lambda b, e: hi.cells_lanes(b, e) == 64),
        "64 lanes above 64 KiB": lambda: first(lambda b, e: b + e >= 1536),
        "the largest LDS": lambda: max(p for p in range(0, 4096, 16) if (lane_bytes + p + extra) * 64 + 128 <= hi.MAX_LDS),
    }
    out = {regime: out[regime]() for regime in regimes}
    b = {k: lane_bytes + p for k, p in out.items()}
    if "128 lanes" in b:
        assert hi.cells_lanes(b["128 lanes"], extra) == 128 and hi.cells_lds(b["128 lanes"], extra) <= 48 * 1024 + 128
    if "64 lanes" in b:
        assert hi.cells_lanes(b["64 lanes"], extra) == 64 and hi.cells_lds(b["64 lanes"], extra) < 64 * 1024
    if "64 lanes above 64 KiB" in b:
        assert hi.cells_lanes(b["64 lanes above 64 KiB"], extra) == 64 and 64 * 1024 < hi.cells_lds(b["64 lanes above 64 KiB"], extra) < hi.MAX_LDS
    assert hi.cells_lanes(b["the largest LDS"], extra) == 64
    assert hi.MAX_LDS - 16 * 64 < hi.cells_lds(b["the largest LDS"], extra) <= hi.MAX_LDS
    too_large = out["the largest LDS"] + 16
    with pytest.raises(ValueError):
        hi.cells_lds(lane_bytes + too_large, extra)
    return out, too_large


def padded(monkeypatch, pad):
    genuine = _instance_cells.device_table

    def device_table(instances, queue, full_programs=False):
        table, distance_only, lane_bytes = genuine(instances, queue, full_programs)
        return table, distance_only, lane_bytes + pad

    monkeypatch.setattr(_instance_cells, "device_table", device_table)


def at_every_shape(hip, monkeypatch, instances, extra, run, below_256=False):
    """`run()` checks a call against its reference and returns what must not change: unpadded, at every regime's pad,
    refused cleanly one pad further, and unpadded again.  `below_256`: the unpadded run has fewer than 256 lanes already,
    and the regimes are those the rule leaves it (heavy_instances.regimes_of), each with a pad of its own."""
    table, distance_only, lane_bytes = _instance_cells.device_table(list(instances), hip.queue)
    table.release()
    assert hi.cells_lanes(lane_bytes, extra) in ((128, 64) if below_256 else (256, 128))
    wanted = hi.regimes_of(lane_bytes, extra) if below_256 else REGIMES
    regimes, too_large = pads(lane_bytes, extra, wanted)
    if below_256:
        assert (distance_only, lane_bytes) == hi.table_figures(list(instances))
        assert {"64 lanes above 64 KiB", "the largest LDS"} <= set(wanted) and all(p > 0 for p in regimes.values())
    plain = run()
    for regime in wanted:
        padded(monkeypatch, regimes[regime])
        got = run()
        monkeypatch.undo()
        assert got == plain, regime
    padded(monkeypatch, too_large)
    with pytest.raises(RuntimeError, match="live"):
        run()
    monkeypatch.undo()
    assert run() == plain


def test_padded_interference_and_clearance(hip, monkeypatch):
    sc = EDGE_SCENARIOS["crowd33_blended"]
    gap = sc.gaps[1]
    asm = sc.build(gap)
    instances = _instance_cells.visible(asm, sc.resolution)
    references = {}

    def interference():
        r = cc.interference(asm, sc.resolution)
        references.setdefault("pairs", dense_pairs(r))
        assert device_pairs(r) == references["pairs"]
        return r.pairs, r.samples_evaluated

    def clearance():
        r = cc.clearance(asm, sc.resolution, gap)
        references.setdefault("near", dense_near(r))
        assert device_near(r) == references["near"]
        return r.pairs, r.samples_evaluated

    at_every_shape(hip, monkeypatch, instances, 0, interference)
    at_every_shape(hip, monkeypatch, instances, 4 * len(instances), clearance)


@pytest.mark.parametrize("distance", [False, True])
def test_padded_section(hip, monkeypatch, distance):
    asm, plane, resolution, ref = tsh.scenario("random_5_oblique")

    def run():
        cut = cc.section(asm, plane, resolution, distance=distance)
        gpu_section.check(cut, ref, distance)
        return cut.part_ids.tobytes(), cut.inside_count.tobytes(), cut.distance.tobytes() if distance else None, cut.evaluations

    # with distance the tiles keep 4 bytes per instance: they are the kernel the regimes are sized for
    at_every_shape(hip, monkeypatch, ref.instances, 4 * len(ref.instances) if distance else 0, run)


def test_padded_section_outlines(hip, monkeypatch):
    asm, plane, resolution, ref = tso.scenario("boxes_and_ball")

    def run():
        o = gpu_outlines.run("boxes_and_ball")[0]
        return o.segments.tobytes(), o.counts.tolist(), o.evaluations

    at_every_shape(hip, monkeypatch, ref.instances, 8, run)


def test_padded_layer_outlines(hip, monkeypatch):
    ref = layer_scenes.scenario("two_boxes")[4]

    def run():
        got = gpu_layers.run("two_boxes")[0]
        return got.segments.tobytes(), got.layer_counts.tolist(), got.evaluations

    at_every_shape(hip, monkeypatch, ref.instances, 8, run)


def test_padded_assembly_meshes(hip, monkeypatch):
    instances = mesh_scenes.scene("coincident")[2]
    ref = mesh_scenes.reference("coincident")

    def run():
        m = cc.assembly_meshes(mesh_scenes.scene("coincident")[0], mesh_scenes.scene("coincident")[1])
        gpu_meshes.check(m, ref, mesh_scenes.traversal("coincident").evaluations)
        return m.triangles.tobytes(), m.counts.tolist(), m.evaluations

    at_every_shape(hip, monkeypatch, instances, 8, run)


@pytest.mark.parametrize("retire", [True, False])
def test_padded_assembly_mass_properties(hip, monkeypatch, retire):
    asm, resolution, instances, corner, step, dims = mass_scenes.scene("blend")
    ref = mass_scenes.reference("blend", retire)

    def run():
        report = cc.assembly_mass_properties(asm, resolution, retire=retire)
        gpu_mass.check_against_dense(report, ref)
        assert report.samples_evaluated == ref.evaluations
        return [(p.sums, p.owned_sums, p.index_box) for p in report.parts], report.samples_evaluated

    at_every_shape(hip, monkeypatch, instances, 0, run)


PADDED_SEPARATION_SIDE = 256        # random_5 from cells of 256 samples: rows on two levels above the finest one


def test_padded_separation(hip, monkeypatch):
    """random_5 from a top side of 256 (its own is 16, one level): the reference lists rows of side 64, 16 and 4, so the
    k_gap_cells of two levels read bounds an earlier level wrote and compact behind the [instance][lane] area."""
    asm, resolution, instances, corner, step, dims = sep_scenes.scene("random_5")
    dense, traversal = sep_scenes.dense_reference("random_5"), sep_scenes.traversal_reference("random_5", PADDED_SEPARATION_SIDE)
    assert len(traversal.level_rows) == 3 and all(rows > 0 for rows in traversal.level_rows)

    def run():
        report = gpu_separation.sep._separation(asm, resolution, side=PADDED_SEPARATION_SIDE)
        gpu_separation.check(report, dense, traversal)
        return report.pairs, report.samples_evaluated, report.level_rows

    at_every_shape(hip, monkeypatch, instances, 4 * len(instances), run)


def test_padded_separation_of_64_instances(hip, monkeypatch):
    """solids64: 256 B of [instance][lane] area per lane, 16 KiB per wavefront, the largest offsets the kernels form.  It
    starts at 128 lanes; the rule leaves it 64 lanes, 64 lanes above 64 KiB and the largest LDS (the host file says so)."""
    asm, resolution, instances, corner, step, dims = sep_scenes.scene("solids64")
    dense, traversal = sep_scenes.dense_reference("solids64"), sep_scenes.traversal_reference("solids64")
    assert len(instances) == 64

    def run():
        report = cc.separation(asm, resolution)
        gpu_separation.check(report, dense, traversal)
        return report.pairs, report.samples_evaluated, report.level_rows

    at_every_shape(hip, monkeypatch, instances, 4 * len(instances), run, below_256=True)


@pytest.mark.parametrize("retire", [True, False])
def test_padded_assembly_voxels(hip, monkeypatch, retire):
    ref = voxel_scenes.reference("blend", retire)

    def run():
        voxels = cc.assembly_voxels(*mass_scenes.scene("blend")[:2], retire=retire)
        gpu_voxels.check_against_dense(voxels, ref)
        assert voxels.samples_evaluated == ref.evaluations
        return voxels.part_ids.tobytes(), voxels.counts, voxels.samples_evaluated

    at_every_shape(hip, monkeypatch, mass_scenes.scene("blend")[2], 0, run)
