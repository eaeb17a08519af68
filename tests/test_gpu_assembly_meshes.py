"""assembly_meshes() on the device against the reference meshes of assembly_meshes_scenes.py: every instance evaluated by the
oracle at every ringed sample, crossings in NumPy float32, the case table derived by tools/gen_mc_table.py.  Every
comparison is exact: the sorted records byte for byte, the counts, the evaluations and the runs as integers."""
import os
import sys

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import rendering, shapes, _instance_cells
from codecad_amd.assembly_meshes import TRIANGLE

import assembly_meshes_scenes as scenes
from assembly_meshes_scenes import SCENES, scene, reference, traversal, dense_evaluations, check_mesh_properties

pytestmark = pytest.mark.gpu

am = sys.modules["codecad_amd.assembly_meshes"]        # (the package's attribute of that name is the function)


def check(m, ref, evaluations=None):
    assert list(m.dims) == list(ref.dims) and m.step == ref.step and m.corner.tobytes() == ref.corner.tobytes()
    assert m.triangles.dtype == TRIANGLE and m.triangles.tobytes() == ref.triangles.tobytes()
    assert m.counts.tolist() == ref.counts.tolist()
    assert [i.instance.transform for i in m.instances] == [i.transform for i in ref.instances]
    if evaluations is not None:
        assert m.evaluations == evaluations


def run(name, monkeypatch, cull=True, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    if cull and SCENES[name].side is not None:
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.forced_top_cells(dims + 1, SCENES[name].side))
        assert _instance_cells.top_side(dims + 1) == SCENES[name].side
    m = cc.assembly_meshes(asm, resolution, cull=cull, **kwargs)
    monkeypatch.undo()
    ref = reference(name)
    check(m, ref, traversal(name).evaluations if cull else dense_evaluations(dims, len(instances)))
    return m, ref


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_device_gives_the_reference_mesh(hip, monkeypatch, name):
    m, ref = run(name, monkeypatch)
    assert m.runs == 1                                              # the first lists and the first triangle buffer hold everything


@pytest.mark.parametrize("name", sorted(SCENES))
def test_dense_gives_what_culled_gives(hip, monkeypatch, name):
    dense, ref = run(name, monkeypatch, cull=False)
    assert dense.runs == 1


def test_a_triangle_buffer_that_overflows_is_counted_exactly_and_regrown(hip, monkeypatch):
    ref = reference("coincident")
    seen = []
    traverse = _instance_cells.traverse

    def watched(*args, **kwargs):
        out = traverse(*args, **kwargs)
        seen.append(out[1].copy())
        return out

    monkeypatch.setattr(am.cells, "traverse", watched)
    asm, resolution = scene("coincident")[:2]
    few = cc.assembly_meshes(asm, resolution, triangle_capacity=1)
    monkeypatch.undo()
    check(few, ref, traversal("coincident").evaluations)
    assert few.runs == 2 and len(seen) == 2                         # one retry: the count of the overflowed run was the whole count
    for totals in seen:
        assert totals.tolist() == [len(ref.triangles)] + ref.counts.tolist()
    dense = run("coincident", monkeypatch, cull=False, triangle_capacity=1)[0]
    assert dense.runs == 2


def test_cell_lists_that_overflow_are_regrown(hip, monkeypatch):
    first = run("coarse_64", monkeypatch)[0]
    small = run("coarse_64", monkeypatch, initial_capacity=1)[0]
    both = run("coarse_64", monkeypatch, initial_capacity=1, triangle_capacity=1)[0]
    assert first.runs == 1 and small.runs > 1 and both.runs > small.runs
    assert small.triangles.tobytes() == first.triangles.tobytes() == both.triangles.tobytes()


def test_the_welded_meshes_of_the_device_are_closed_and_as_large_as_their_samples(hip, monkeypatch):
    m, ref = run("gears", monkeypatch)
    assert len(m.instances) == 8 and (m.counts > 0).all()
    check_mesh_properties(m, ref)


def test_one_stl_file_per_instance(hip, tmp_path):
    asm, resolution = scene("gears")[:2]
    ref = reference("gears")
    paths = rendering.render_assembly_stl(asm, str(tmp_path / "parts"), resolution)
    assert len(paths) == 8 == len(set(paths)) and sorted(os.listdir(str(tmp_path / "parts"))) == sorted(os.path.basename(p) for p in paths)
    for k, path in enumerate(paths):
        assert os.path.basename(path).startswith("%02d_" % k) and path.endswith(".stl")
        assert os.path.getsize(path) == 84 + 50 * int(ref.counts[k])


def test_an_assembly_with_no_visible_instance_launches_nothing(hip):
    m = cc.assembly_meshes(cc.assembly("ghosts", [shapes.sphere(1).make_part("ball").hidden()]), 0.1)
    assert m.runs == 0 and m.evaluations == 0 and len(m.triangles) == 0 and m.counts.tolist() == []
