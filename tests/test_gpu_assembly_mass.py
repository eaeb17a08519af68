"""assembly_mass_properties() on the device against the dense definition (assembly_mass_scenes.reference_mass): the sums of
V_k and O_k and the index box of V_k of every instance are EQUAL to what evaluating every instance over the whole lattice
gives, with and without retirement, and the number of evaluations is EQUAL to the reference traversal's."""
import math

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, _instance_cells

import assembly_mass_scenes as scenes
from assembly_mass_scenes import SCENES, scene, reference

pytestmark = pytest.mark.gpu


def run(name, monkeypatch, **kwargs):
    asm, resolution, instances, corner, step, dims = scene(name)
    if SCENES[name].side is not None:
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", scenes.forced_top_cells(dims, SCENES[name].side))
        assert _instance_cells.top_side(dims) == SCENES[name].side
    report = cc.assembly_mass_properties(asm, resolution, densities=SCENES[name].densities, **kwargs)
    monkeypatch.undo()
    assert numpy.array_equal(report.corner, corner) and report.step == step and list(report.dims) == list(dims)
    return report


def check_against_dense(report, ref):
    assert len(report.parts) == len(ref.sums)
    for k, part in enumerate(report.parts):
        assert part.index == k and part.name == report.instances[k].name
        assert part.sums == ref.sums[k], (k, part.name)
        assert part.owned_sums == ref.owned[k], (k, part.name)
        assert part.index_box == ref.boxes[k], (k, part.name)
        assert part.count == ref.sums[k][0]
    # the O_k partition the samples inside any instance
    assert sum(part.owned_sums[0] for part in report.parts) == ref.union_count
    assert report.union_volume == pytest.approx(ref.union_count * float(report.step) ** 3, rel=1e-12)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_sums_and_evaluations_equal_the_reference(hip, name, monkeypatch):
    evaluated = {}
    for retire in (True, False):
        ref = reference(name, retire)
        report = run(name, monkeypatch, retire=retire)
        print(name, "retire" if retire else "descend", "evaluations", report.samples_evaluated, "reference", ref.evaluations)
        check_against_dense(report, ref)
        assert report.samples_evaluated == ref.evaluations and report.traversals == 1
        evaluated[retire] = report.samples_evaluated
    if sum(level.retired for level in reference(name, True).levels):
        assert evaluated[True] < evaluated[False]
    else:
        assert evaluated[True] == evaluated[False]


def test_the_gear_train_survives_overflow_and_is_reproducible(hip, monkeypatch):
    first = run("gears", monkeypatch)
    small = run("gears", monkeypatch, initial_capacity=32)
    assert first.traversals == 1 and small.traversals > 1
    assert [p.sums for p in small.parts] == [p.sums for p in first.parts]
    assert [p.owned_sums for p in small.parts] == [p.owned_sums for p in first.parts]
    assert [p.index_box for p in small.parts] == [p.index_box for p in first.parts]
    assert small.samples_evaluated == first.samples_evaluated
    check_against_dense(small, reference("gears"))


def _pairs_of_two():
    ball = shapes.sphere(r=1).make_part("ball")
    yield "boxes", scenes._boxes(), 0.125
    yield "blend", scenes._blend(), 0.06
    yield "rims", scenes._rims(), 0.125
    yield "lens", cc.assembly("spheres", [ball, ball.translated(1.2, 0, 0).rotated_z(17)]), 0.05


@pytest.mark.parametrize("name,asm,resolution", list(_pairs_of_two()), ids=lambda v: v if isinstance(v, str) else None)
def test_ownership_is_the_part_less_its_interference(hip, name, asm, resolution):
    """Exact, on the same assembly and resolution: what instance 1 owns is what is inside it less what interference()
    reports of the pair (0, 1)."""
    report = cc.assembly_mass_properties(asm, resolution)
    pairs = cc.interference(asm, resolution).pairs
    assert [(p.i, p.j) for p in pairs] == [(0, 1)]
    pair, part = pairs[0], report.parts[1]
    assert part.owned_sums[0] == part.sums[0] - pair.count
    assert part.owned_sums[1:4] == tuple(part.sums[1 + c] - pair.index_sums[c] for c in range(3))
    assert report.parts[0].owned_sums == report.parts[0].sums


def box_integrals(a, b):
    """The ten integrals of the box with corners a, b at unit density."""
    size = [hi - lo for lo, hi in zip(a, b)]
    c = [(lo + hi) / 2 for lo, hi in zip(a, b)]
    v = size[0] * size[1] * size[2]
    out = {"1": v}
    for k, axis in enumerate("xyz"):
        out[axis] = v * c[k]
        out[axis + axis] = v * (c[k] ** 2 + size[k] ** 2 / 12)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        out["xyz"[i] + "xyz"[j]] = v * c[i] * c[j]
    return out


def properties_of(integrals):
    """(mass, centre, inertia tensor about the centre) of ten integrals, written out independently of the package."""
    m = integrals["1"]
    c = [integrals[a] / m for a in "xyz"]
    second = {k: integrals[k] - m * c["xyz".index(k[0])] * c["xyz".index(k[1])] for k in ("xx", "yy", "zz", "xy", "xz", "yz")}
    tensor = numpy.array([[second["yy"] + second["zz"], -second["xy"], -second["xz"]],
                          [-second["xy"], second["xx"] + second["zz"], -second["yz"]],
                          [-second["xz"], -second["yz"], second["xx"] + second["yy"]]])
    return m, c, tensor


def test_two_boxes_weigh_what_their_closed_forms_say(hip, monkeypatch):
    """Faces on multiples of the step: the cubes around the samples tile the boxes, every float64 sum is exact."""
    report = run("boxes", monkeypatch)
    a, b = box_integrals(*scenes.BOX_A), box_integrals(*scenes.BOX_B)
    both = box_integrals(tuple(max(p, q) for p, q in zip(scenes.BOX_A[0], scenes.BOX_B[0])),
                         tuple(min(p, q) for p, q in zip(scenes.BOX_A[1], scenes.BOX_B[1])))
    rho = scenes.BOX_DENSITIES
    for part, integrals, density in zip(report.parts, (a, b), rho):
        volume, centre, tensor = properties_of(integrals)
        assert part.density == density and part.volume == pytest.approx(volume, abs=1e-9) and part.mass == pytest.approx(density * volume, abs=1e-9)
        assert part.properties.volume == pytest.approx(volume, abs=1e-9)
        assert tuple(part.properties.centroid) == pytest.approx(centre, abs=1e-9)
        assert part.properties.inertia_tensor == pytest.approx(tensor, abs=1e-9 * 8)
    total = {k: rho[0] * a[k] + rho[1] * (b[k] - both[k]) for k in a}              # the overlap belongs to the first box
    mass, centre, tensor = properties_of(total)
    assert mass == rho[0] * 8 + rho[1] * (6 - 1)
    assert report.total_mass == pytest.approx(mass, abs=1e-9) and report.total.volume == pytest.approx(mass, abs=1e-9)
    assert tuple(report.total.centroid) == pytest.approx(centre, abs=1e-9)
    assert report.total.inertia_tensor == pytest.approx(tensor, abs=1e-9 * mass)
    assert report.union_volume == pytest.approx(8 + 6 - 1, abs=1e-9)


def test_the_sphere_weighs_like_a_sphere(hip, monkeypatch):
    report = run("sphere", monkeypatch)
    ball = report.parts[0]
    volume = 4 / 3 * math.pi
    assert ball.volume == pytest.approx(volume, rel=0.02)
    assert tuple(ball.properties.centroid) == pytest.approx((0, 0, 0), abs=1e-6)
    assert numpy.diag(ball.properties.inertia_tensor) == pytest.approx([0.4 * volume] * 3, rel=0.02)
    assert report.total_mass == pytest.approx(volume, rel=0.02)                    # the core inside it adds nothing


def test_one_part_against_mass_properties_of_its_shape(hip):
    """Two definitions of one quantity: the lattice count here, adaptive cells in mass_properties().  They agree within
    the lattice's own error bound, surface area x step / volume (a boundary layer one step thick), worked out from the
    shape's analytic area and volume; the ratio observed is printed, not held to a tolerance of its own."""
    r, h, resolution = 1.0, 1.5, 1 / 16
    shape = shapes.cylinder(h=h, r=r)
    area, volume = 2 * math.pi * r * h + 2 * math.pi * r * r, math.pi * r * r * h
    bound = area * resolution / volume
    part = cc.assembly_mass_properties(cc.assembly("one", [shape.make_part("peg")]), resolution).parts[0]
    single = cc.mass_properties(shape, resolution)
    ratio = part.properties.volume / single.volume
    print("lattice volume / mass_properties volume: %.6f (bound %.4f); analytic %.6f, lattice %.6f, adaptive %.6f"
          % (ratio, bound, volume, part.properties.volume, single.volume))
    assert abs(ratio - 1) <= bound
    assert abs(part.properties.volume / volume - 1) <= bound
    scale = volume * (r * r + h * h)
    assert numpy.abs(part.properties.inertia_tensor - single.inertia_tensor).max() <= bound * scale
    assert max(abs(a - b) for a, b in zip(part.properties.centroid, single.centroid)) <= bound * max(r, h)
