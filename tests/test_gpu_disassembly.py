"""disassembly() on the device against the reference of disassembly_scenes.py, which is written from the definition: the
distances, the witnesses, the part ids and the counts are EQUAL to the reference, entry for entry, on every scenario, and a
second call on the same assembly gives the same bytes."""
import numpy
import pytest

import codecad_amd as cc

import disassembly_scenes as scenes
from disassembly_scenes import SCENES, NAMES, NEVER, reference, scene

pytestmark = pytest.mark.gpu


def run(name, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    report = cc.disassembly(asm, resolution, **kwargs)
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    assert len(report.instances) == len(instances)
    return report


def check_against_reference(report, ref):
    n = len(ref.counts)
    assert report.part_ids.dtype == numpy.uint8 and numpy.array_equal(report.part_ids, ref.ids)
    assert report.counts == ref.counts and all(type(c) is int for c in report.counts)
    assert report.distance.dtype == numpy.uint32 and report.distance.shape == (3, n, n)
    assert report.witness.dtype == numpy.int32 and report.witness.shape == (3, n, n, 3)
    wrong = numpy.argwhere(report.distance != ref.distance)
    assert len(wrong) == 0, [(tuple(k), int(report.distance[tuple(k)]), int(ref.distance[tuple(k)])) for k in wrong[:8]]
    wrong = numpy.argwhere((report.witness != ref.witness).any(axis=-1))
    assert len(wrong) == 0, [(tuple(k), report.witness[tuple(k)].tolist(), ref.witness[tuple(k)].tolist()) for k in wrong[:8]]


@pytest.mark.parametrize("name", NAMES)
def test_everything_equals_the_reference(hip, name):
    report = run(name)
    ref, sc = reference(name), SCENES[name]
    print(name, "finite entries", int((report.distance != NEVER).sum()), "reference", int((ref.distance != NEVER).sum()),
          "by hand", {k: (int(report.distance[k]), report.witness[k].tolist()) for k in list(sc.by_hand)[:4]})
    check_against_reference(report, ref)
    assert report.traversals == 1
    for (axis, i, j), (d, p) in sc.by_hand.items():
        assert report.steps(i, j, axis, True) == d == report.steps(j, i, axis, False) and tuple(report.witness[axis, i, j]) == tuple(p)
    assert report.order() == scenes.reference_order(ref.distance) and (sc.order is None or report.order() == sc.order)
    again = run(name)                                                               # the same bytes, whatever order anything ran in
    assert again.distance.tobytes() == report.distance.tobytes() and again.witness.tobytes() == report.witness.tobytes()
    assert numpy.array_equal(again.part_ids, report.part_ids) and again.counts == report.counts


def test_the_empty_assembly_launches_nothing(hip):
    report = cc.disassembly(scenes.empty_assembly(), 0.1)
    assert report.traversals == 0 and report.distance.shape == (3, 0, 0) and report.order() == ([], [])

