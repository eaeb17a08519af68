"""assembly_components() and cavities() on the device against the flood fill of assembly_components_scenes.py: labels, every
field of every Component, the cavities and the part ids are EQUAL to the reference, with the LDS stage and without it, and
whatever the table's first capacity was."""
import numpy
import pytest

import codecad_amd as cc
from codecad_amd import _instance_cells

import assembly_components_scenes as scenes
from assembly_components_scenes import SCENES, CASES, scene, reference, EMPTY_SPACE, SOLID, NONE

pytestmark = pytest.mark.gpu


def run(name, of, monkeypatch, **kwargs):
    """The ComponentsReport of a scenario (through cavities() for empty space, checked on the way)."""
    asm, resolution, instances, corner, step, dims = scene(name)
    if SCENES[name].side is not None:
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.mass.forced_top_cells(dims, SCENES[name].side))
        assert _instance_cells.top_side(dims) == SCENES[name].side
    if of == EMPTY_SPACE:
        found = cc.cavities(asm, resolution, **kwargs)
        report = found.components_report
        check_cavities(found, reference(name, of), [i.name for i in instances])
    else:
        report = cc.assembly_components(asm, resolution, of=SOLID, **kwargs)
    monkeypatch.undo()
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims) and report.of == of
    return report


def check_cavities(found, ref, names):
    closed = [c for c in ref.components if not c.touches_border]
    assert [(c.label, c.count, c.box, c.index_sums, c.parts) for c in found.cavities] == \
        [(c.label, c.count, c.box, c.index_sums, c.parts) for c in closed]
    assert [c.enclosed_by for c in found.cavities] == [tuple(names[k] for k in c.parts) for c in closed]
    assert not any(c.touches_border for c in found.cavities)
    step = float(found.components_report.step)
    assert found.sealed_volume == sum(c.count * step ** 3 for c in closed)


def check_against_reference(report, ref):
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    assert report.labels.dtype == numpy.uint32 and report.labels.shape == ref.labels.shape and report.labels.flags.c_contiguous
    assert numpy.array_equal(report.labels, ref.labels)
    got = [(c.label, c.count, c.box, c.index_sums, c.touches_border, c.parts) for c in report.components]
    assert got == [tuple(c) for c in ref.components]
    corner, step = [float(v) for v in report.corner], float(report.step)
    for c in report.components:
        assert all(type(v) is int for v in (c.label, c.count) + c.index_sums + c.box[0] + c.box[1] + c.parts)
        assert c.volume == c.count * step ** 3
        assert tuple(c.centroid) == tuple(corner[k] + step * c.index_sums[k] / c.count for k in range(3))
        assert report.mask(c).sum() == c.count


@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("name,of", CASES)
def test_labels_components_cavities_and_ids_equal_the_reference(hip, name, of, local, monkeypatch):
    report = run(name, of, monkeypatch, local=local)
    ref = reference(name, of)
    print(name, of, "local" if local else "global", "components", len(report.components), "reference", len(ref.components))
    check_against_reference(report, ref)
    assert report.traversals == 1 and report.component_capacity_runs == 1


@pytest.mark.parametrize("local", [True, False])
def test_the_table_regrows_and_only_the_statistics_run_again(hip, local, monkeypatch):
    ref = reference("bubbles")
    assert len(ref.components) > 1
    small = run("bubbles", EMPTY_SPACE, monkeypatch, local=local, initial_components=1)
    check_against_reference(small, ref)
    assert small.component_capacity_runs == 2 and small.traversals == 1


def test_a_small_cell_list_repeats_the_traversal_and_changes_nothing(hip, monkeypatch):
    first = run("bubbles", EMPTY_SPACE, monkeypatch)
    small = run("bubbles", EMPTY_SPACE, monkeypatch, initial_capacity=32)
    assert first.traversals == 1 and small.traversals > 1 and small.component_capacity_runs == 1
    check_against_reference(small, reference("bubbles"))
    assert small.samples_evaluated == first.samples_evaluated


def test_one_cup_hidden_leaves_no_cavity(hip, monkeypatch):
    both, one = scene("two_cups"), scene("one_cup")
    found = cc.cavities(both[0], both[1])
    assert [c.enclosed_by for c in found.cavities] == [("lower", "upper")] and found.cavities[0].count == 512
    assert found.sealed_volume == 512 * 0.0625 ** 3
    assert cc.cavities(one[0], one[1]).cavities == []


def test_the_shell_encloses_one_cavity(hip):
    asm, resolution = scene("shell")[:2]
    found = cc.cavities(asm, 1 / 16)
    assert len(found.cavities) == 1 and found.cavities[0].enclosed_by == ("shell",)
    assert found.cavities[0].count == int((found.components_report.labels == found.cavities[0].label).sum())
    assert (found.components_report.labels[found.components_report.part_ids != 255] == NONE).all()
