"""assembly_voxels() on the device against the dense definition (assembly_voxels_scenes.reference_voxels): the part ids of
every sample and the counts of every instance are EQUAL to what evaluating every instance over the whole lattice gives,
with and without retirement, and the number of evaluations is EQUAL to the reference traversal's."""
import os

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import rendering, _instance_cells
from codecad_amd.section import Plane

import assembly_mass_scenes as mass_scenes
import assembly_voxels_scenes as scenes
import heavy_instances as hi
from assembly_voxels_scenes import SCENES, scene, reference, EMPTY

pytestmark = pytest.mark.gpu


def run(name, monkeypatch, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    if SCENES[name].side is not None:
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.forced_top_cells(dims, SCENES[name].side))
        assert _instance_cells.top_side(dims) == SCENES[name].side
    voxels = cc.assembly_voxels(asm, resolution, **kwargs)
    monkeypatch.undo()
    assert numpy.array_equal(voxels.corner, corner) and voxels.step == step and list(voxels.dims) == list(dims)
    return voxels


def check_against_dense(voxels, ref):
    assert voxels.part_ids.dtype == numpy.uint8 and voxels.part_ids.shape == ref.ids.shape
    assert numpy.array_equal(voxels.part_ids, ref.ids)
    assert voxels.counts == ref.counts and all(type(c) is int for c in voxels.counts)
    assert voxels.counts == [int(voxels.mask(k).sum()) for k in range(len(voxels.counts))]
    assert len(voxels.instances) == len(ref.counts)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_ids_counts_and_evaluations_equal_the_reference(hip, name, monkeypatch):
    evaluated = {}
    for retire in (True, False):
        ref = reference(name, retire)
        voxels = run(name, monkeypatch, retire=retire)
        print(name, "retire" if retire else "descend", "evaluations", voxels.samples_evaluated, "reference", ref.evaluations)
        check_against_dense(voxels, ref)
        assert voxels.samples_evaluated == ref.evaluations and voxels.traversals == 1
        evaluated[retire] = voxels.samples_evaluated
    if sum(level.retired for level in reference(name, True).levels):
        assert evaluated[True] < evaluated[False]
    else:
        assert evaluated[True] == evaluated[False]


@pytest.mark.parametrize("name", ["boxes", "solids64", "gears"] + ["ownership_%d%d%d" % o for o in mass_scenes.OWNERSHIP_ORDERS])
def test_counts_are_what_the_mass_properties_own(hip, name, monkeypatch):
    asm, resolution = scene(name)[:2]
    voxels = run(name, monkeypatch)
    report = cc.assembly_mass_properties(asm, resolution)
    assert voxels.counts == [part.owned_sums[0] for part in report.parts]
    assert voxels.volumes().tolist() == [c * float(voxels.step) ** 3 for c in voxels.counts]


def test_the_sphere_takes_fewer_evaluations_than_its_mass_properties(hip, monkeypatch):
    asm, resolution = scene("sphere")[:2]
    voxels = run("sphere", monkeypatch)
    assert voxels.samples_evaluated < cc.assembly_mass_properties(asm, resolution).samples_evaluated


@pytest.mark.parametrize("name", ["rims", "boxes"])
def test_every_layer_is_the_section_on_its_plane(hip, name, monkeypatch):
    asm, resolution = scene(name)[:2]
    voxels = run(name, monkeypatch)
    for z in range(int(voxels.dims[2])):
        cut = cc.section(asm, Plane.xy(float(voxels.corner[2] + voxels.step * numpy.float32(z))), resolution)
        assert cut.dims == (int(voxels.dims[0]), int(voxels.dims[1])) and cut.step == voxels.step
        assert cut.corner.tobytes() == numpy.array([voxels.corner[0], voxels.corner[1], voxels.corner[2] + voxels.step * numpy.float32(z)],
                                                   numpy.float32).tobytes()
        ids = numpy.where(cut.part_ids == -1, EMPTY, cut.part_ids).astype(numpy.uint8)      # [j, i]: v = y, u = x
        assert numpy.array_equal(voxels.layer(z), ids.T), z


def test_the_gear_train_survives_overflow_and_rewrites_the_same_volume(hip, monkeypatch):
    first = run("gears", monkeypatch)
    small = run("gears", monkeypatch, initial_capacity=32)
    assert first.traversals == 1 and small.traversals > 1
    assert numpy.array_equal(small.part_ids, first.part_ids) and small.counts == first.counts
    assert small.samples_evaluated == first.samples_evaluated
    check_against_dense(small, reference("gears"))


def test_strictness_a_sample_on_a_face_is_not_inside(hip, monkeypatch):
    check_against_dense(run("strict", monkeypatch), reference("strict"))
    asm, resolution, (right, left, outer), ref = scenes.strict_reversed()
    voxels = cc.assembly_voxels(asm, resolution)
    check_against_dense(voxels, ref)
    assert voxels.samples_evaluated == ref.evaluations
    on_a_face = ((right == 0) & ~(left < 0)) | ((left == 0) & ~(right < 0))
    assert on_a_face.sum() >= 6 * 15 * 15 and (voxels.part_ids[on_a_face] == 2).all()


def test_far_from_the_origin(hip):
    asm = mass_scenes._boxes().translated(1000, -2000, 500)
    instances = _instance_cells.visible(asm, 0.125)
    corner, step, dims = _instance_cells.checked_lattice(instances, 0.125)
    assert max(dims) <= 32 and abs(float(corner[1])) > 1999
    for retire in (True, False):
        ref = scenes.reference_voxels(instances, corner, step, dims, retire)
        assert numpy.array_equal(ref.written, ref.ids) and sum(ref.counts) > 0
        voxels = cc.assembly_voxels(asm, 0.125, retire=retire)
        check_against_dense(voxels, ref)
        assert voxels.samples_evaluated == ref.evaluations


def test_a_heavy_part_runs_the_kernels_at_64_lanes(hip, monkeypatch):
    instances = hi.instances_of("heavy_pair25")
    assert hi.cells_lanes(hi.table_figures(instances)[1]) == 64
    ref = reference("heavy_pair25")
    voxels = run("heavy_pair25", monkeypatch)
    check_against_dense(voxels, ref)
    assert voxels.samples_evaluated == ref.evaluations and voxels.counts[1] > 0


def test_the_layers_are_the_colouring_of_the_volume(hip, tmp_path):
    import PIL.Image
    asm, resolution = scene("boxes")[:2]
    directory = tmp_path / "layers"
    voxels = rendering.render_assembly_voxel_layers(asm, resolution, str(directory))
    check_against_dense(voxels, reference("boxes"))
    assert sorted(os.listdir(directory)) == ["layer_%05d.png" % z for z in range(int(voxels.dims[2]))]
    seen = set()
    for z in range(int(voxels.dims[2])):
        pixels = numpy.asarray(PIL.Image.open(directory / ("layer_%05d.png" % z)))
        assert pixels.shape == (int(voxels.dims[1]), int(voxels.dims[0]), 3)
        assert numpy.array_equal(pixels, rendering.render_assembly_voxel_pixels(voxels, z))
        seen |= {tuple(c) for c in pixels.reshape(-1, 3).tolist()}
    assert len(seen) == 3                                           # two parts and the background
