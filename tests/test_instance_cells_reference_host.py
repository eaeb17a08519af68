"""The references and the scenarios of test_gpu_instance_cells_edges.py, checked without a device.

`interference()` and `clearance()` promise, bit for bit, what evaluating every instance over the whole lattice gives
(test_gpu_interference.py dense_pairs, test_gpu_clearance.py dense_near).  This file adds
  * a reference that scales, `windowed_near` / `windowed_pairs`: the same definition evaluated only where two instances'
    windows meet, at points generated per axis as the kernels generate them (corner + step * float32(index), float32,
    not fused) -- shown here to equal the dense one;
  * the SCENARIOS the GPU file runs, each built for an edge of the cell traversal (csrc/instance_pairs.hip,
    _instance_cells.py): the high word of the candidate mask, indices above 32767, the strict thresholds, a lattice
    that needs a top side of 64, coordinates far from the origin.  Every scenario is inspected here: its top side is
    what it says, its windows and top cells are not empty, and the edge it was built for is IN THE REFERENCE -- a scenario
    that loses its edge fails here and does not pass silently on the device.
"""
import collections
import functools
import math
import random
import types

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, nodes, _instance_cells
from codecad_amd._instance_cells import Instance, top_side, cell_rows
from codecad_amd.clearance import half_gap
import oracle

from test_gpu_interference import dense_pairs
from test_gpu_clearance import dense_near, RANDOM, _random_assembly, _gear_train
import heavy_instances


# ---- the references ---------------------------------------------------------------------------------------------------

def lattice_of(asm, resolution, min_gap=0.0):
    """(visible instances, corner, step, dims, t) as `clearance(asm, resolution, min_gap)` lays them out; for
    min_gap = 0 the lattice of `interference(asm, resolution)`."""
    instances = _instance_cells.visible(asm, resolution)
    t = half_gap(min_gap)
    corner, step, dims = _instance_cells.checked_lattice(instances, resolution, grow=float(t))
    return instances, corner, step, dims, t


def as_report(instances, corner, step, dims, min_gap=0.0):
    """What dense_pairs / dense_near read of a report, without a device."""
    return types.SimpleNamespace(instances=[Instance(i.name, i) for i in instances], corner=corner, step=step, dims=dims,
                                 min_gap=min_gap)


def axis_points(corner, step, lo, hi):
    """float32[n, 3] and the index shape: the samples of the index box lo..hi (inclusive), each coordinate computed as
    kernels.hpp sample() and _instance_cells.index_position compute it: corner[k] + step * float32(index), in float32."""
    axes = [numpy.float32(corner[k]) + numpy.float32(step) * numpy.arange(int(lo[k]), int(hi[k]) + 1).astype(numpy.float32)
            for k in range(3)]
    assert all(a.dtype == numpy.float32 for a in axes)
    grid = numpy.stack(numpy.meshgrid(*axes, indexing="ij"), axis=-1)
    return grid.reshape(-1, 3), grid.shape[:3]


def _windowed(instances, corner, step, dims, grow, thr, separation):
    wins = _instance_cells.windows(instances, corner, float(step), dims, grow=float(grow))
    tapes = [nodes.make_program(i.shape()) for i in instances]
    out = {}
    for i in range(len(instances)):
        for j in range(i + 1, len(instances)):
            lo, hi = numpy.maximum(wins[i, 0], wins[j, 0]), numpy.minimum(wins[i, 1], wins[j, 1])
            if (lo > hi).any():
                continue
            points, shape = axis_points(corner, step, lo, hi)
            wi = oracle.evaluate_points(tapes[i], points)[:, 3].reshape(shape)
            wj = oracle.evaluate_points(tapes[j], points)[:, 3].reshape(shape)
            both = (wi < thr) & (wj < thr)
            idx = numpy.argwhere(both)                      # lexicographic, the order of wi[both]
            if not len(idx):
                continue
            idx += lo
            entry = (len(idx), tuple(int(k) for k in idx.sum(axis=0)),
                     (tuple(int(k) for k in idx.min(axis=0)), tuple(int(k) for k in idx.max(axis=0))))
            if separation:
                v = numpy.maximum(wi[both], wj[both])
                sep = v.min()
                witness = tuple(int(k) for k in idx[numpy.nonzero(v == sep)[0][0]])
                entry += (int((sep + numpy.float32(0)).view(numpy.uint32)), witness)
            out[(i, j)] = entry
    return out


def windowed_near_of(instances, corner, step, dims, t):
    """dense_near's dict, from the samples where both windows of a pair meet: the definition of clearance itself (a
    sample is near a pair only inside both windows)."""
    return _windowed(instances, corner, step, dims, t, numpy.float32(t), True)


def windowed_pairs_of(instances, corner, step, dims):
    """dense_pairs' dict, from the samples where both windows (grow = 0) of a pair meet.  Equal to the dense definition
    when every sample inside an instance lies in its window: for parts whose w < 0 only inside their bounding box."""
    return _windowed(instances, corner, step, dims, 0.0, numpy.float32(0), False)


def windowed_near(report):
    return windowed_near_of([i.instance for i in report.instances], report.corner, report.step, report.dims, half_gap(report.min_gap))


def windowed_pairs(report):
    return windowed_pairs_of([i.instance for i in report.instances], report.corner, report.step, report.dims)


# ---- the scenarios ----------------------------------------------------------------------------------------------------

class Scenario(collections.namedtuple("Scenario", "build resolution gaps side windowed per_gap", defaults=(False,))):
    """`build(gap)` -> the assembly checked at `resolution` with min_gap `gap`: one assembly for every gap, unless
    `per_gap` (the lattice has to come out the same size with the gap added, so the parts differ); `gaps`: the
    min_gaps, 0 first; `side`: what top_side() gives on its lattices with nothing forced; `windowed`: the reference is
    the windowed one (the lattice is too large for the dense one)."""

    __slots__ = ()

    def near(self, report):
        return (windowed_near if self.windowed else dense_near)(report)

    def pairs(self, report):
        return (windowed_pairs if self.windowed else dense_pairs)(report)


def _crowd(n_visible, blended):
    """`n_visible` visible instances on a 4 x 4 x 4 arrangement one unit apart, index 16 x + 4 y + z, a few small parts
    randomly rotated so that neighbours overlap or nearly touch; hidden instances BETWEEN visible ones (so that visible
    indices differ from all_instances() indices) and two nested subassemblies, one across the 31 | 32 boundary of the
    mask's words.  `blended`: one part has a rounded blend (the full programs run; else the distance-only ones)."""
    rng = random.Random(64)
    lobes = [shapes.box(0.9, 0.5, 0.5), shapes.sphere(r=0.4).translated_x(0.3)]
    parts = [shapes.sphere(r=0.55).make_part("ball"), shapes.box(0.9, 0.8, 1.0).make_part("block"),
             shapes.cylinder(h=1.1, d=0.7).make_part("peg"), shapes.union(lobes, r=0.15 if blended else -1).make_part("knob")]

    def place(n):
        axis = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.1, 1))
        where = (n // 16 + rng.uniform(-0.1, 0.1), (n // 4) % 4 + rng.uniform(-0.1, 0.1), n % 4 + rng.uniform(-0.1, 0.1))
        return parts[(n + n // 4 + n // 16) % 4].rotated(axis, rng.uniform(-180, 180)).translated(*where)

    placed = [place(n) for n in range(64)][:n_visible]
    ghost = parts[1].translated(1.5, 1.5, 1.5).hidden()
    first = cc.assembly("first", [placed[0], ghost, placed[1], placed[2]]).rotated_z(2).translated(0.02, -0.03, 0.01)
    listed = [first]
    n = 3
    while n < n_visible:
        if n == 30:
            inner = placed[30:35]
            listed.append(cc.assembly("across", inner[:2] + [ghost.translated_x(1)] + inner[2:]).translated(0.01, 0.02, -0.01))
            n += len(inner)
            continue
        listed.append(placed[n])
        if n % 9 == 4:
            listed.append(ghost.translated_y(0.1 * n))
        n += 1
    return cc.assembly("crowd", listed)


def _rods(axis, samples, resolution, gap):
    """Two long boxes side by side along `axis`, overlapping along their whole length, and a small ball inside both at
    the FAR end; the lattice has `samples` along the axis once the boxes are grown by gap / 2, and about 12 x 8 across."""
    length = samples * resolution - gap
    size = [0.08 / 0.01 * resolution] * 3
    size[axis] = length
    rod = shapes.box(*size).make_part("rod")
    shift = [0.0] * 3
    shift[(axis + 1) % 3] = 4 * resolution
    end = [0.7 * resolution, 0.4 * resolution, -0.3 * resolution]
    end[(axis + 1) % 3] += 2 * resolution
    end[axis] = length / 2 - 5.3 * resolution
    ball = shapes.sphere(r=3.1 * resolution).make_part("ball")
    return cc.assembly("rods", [rod, rod.translated(*shift), ball.translated(*end)])


def _dyadic(gap):
    """Boxes with faces on multiples of 2^-4, a lattice of step 2^-4 whose samples lie ON those faces: `outer` (faces at
    +-(1 + 2^-5), so corner = -1 exactly) holds `right` (x in [0, 1]) and `left` (x in [-1, 0]), which touch on x = 0."""
    outer = shapes.box(2.0625).make_part("outer")
    half = shapes.box(1).make_part("half")
    return cc.assembly("dyadic", [outer, half.translated_x(0.5), half.translated_x(-0.5)])


def _plate(gap):
    """About a dozen simple parts in two clusters near opposite corners of a 120 x 120 x 1.2 plate: at 0.05 the lattice
    is about 2400 x 2400 x 24, more than 32768 cells of 16 samples."""
    rng = random.Random(2400)
    parts = [shapes.sphere(r=0.6).make_part("ball"), shapes.box(1.2, 1.0, 0.8).make_part("block"),
             shapes.cylinder(h=1.0, d=1.0).make_part("peg")]
    placed = [parts[0].translated(0.6, 0.6, 0.0), parts[0].translated(119.4, 119.4, 0.0)]       # the plate's extent
    for corner in (0.0, 113.0):
        for k in range(5):
            where = (corner + rng.uniform(1.5, 5.5), corner + rng.uniform(1.5, 5.5), rng.uniform(-0.1, 0.1))
            placed.append(parts[k % 3].rotated_z(rng.uniform(-180, 180)).translated(*where))
    return cc.assembly("plate", placed)


def far_translation(resolution):
    """A translation along every axis that puts coordinates where one float32 ulp is step / 8 to step / 4."""
    ulp = 2.0 ** math.floor(math.log2(resolution / 4))
    return 1.5 * ulp * 2 ** 23


def _far(asm, resolution):
    """`asm` turned and moved far from the origin through its OWN transform (asm.transform in _instance_cells.visible)."""
    d = far_translation(resolution)
    return asm.rotated((1, 2, 3), 25).translated(d, -d, d)


def per_instance(asm):
    """The same placement with the assembly's transform applied to each of its listed instances instead."""
    return cc.assembly(asm.part.name, [i._transformed(asm.transform) for i in asm])


@functools.lru_cache(maxsize=None)
def _random_far():
    return _far(_random_assembly(*RANDOM[1]), FAR_RANDOM_RESOLUTION)


@functools.lru_cache(maxsize=None)
def _gears_far():
    return _far(_gear_train(), FAR_GEARS_RESOLUTION)


FAR_RANDOM_RESOLUTION = 0.14
FAR_GEARS_RESOLUTION = 0.15
ROD = 0.01                  # 62000 samples of it: rods 620 long
EXACT = 2.0 ** -7           # 65536 samples of it: 512

SCENARIOS = {
    "crowd64_blended": Scenario(lambda gap: _crowd(64, True), 0.065, (0.0, 0.39), 16, False),
    "crowd64_plain": Scenario(lambda gap: _crowd(64, False), 0.065, (0.0, 0.39), 16, False),
    "crowd33_blended": Scenario(lambda gap: _crowd(33, True), 0.065, (0.0, 0.39), 16, False),
    "rods_x": Scenario(lambda gap: _rods(0, 62000, ROD, 0.0), ROD, (0.0, 0.04), 16, False),
    "rods_y": Scenario(lambda gap: _rods(1, 62000, ROD, 0.0), ROD, (0.0, 0.04), 16, False),
    "rods_z": Scenario(lambda gap: _rods(2, 62000, ROD, 0.0), ROD, (0.0, 0.04), 16, False),
    "rods_y_65536": Scenario(lambda gap: _rods(1, 65536, EXACT, gap), EXACT, (0.0, 8 * EXACT), 16, False, True),
    "dyadic": Scenario(_dyadic, 0.0625, (0.0, 0.25), 16, False),
    "plate": Scenario(_plate, 0.05, (0.0, 0.3), 64, True),
    "far_random": Scenario(lambda gap: _random_far(), FAR_RANDOM_RESOLUTION, (0.0, 4 * FAR_RANDOM_RESOLUTION), 16, False),
    "far_gears": Scenario(lambda gap: _gears_far(), FAR_GEARS_RESOLUTION, (0.0, 0.5), 16, False),
}
SCENARIOS.update(heavy_instances.pair_scenarios(Scenario))       # parts with wide register files among light ones


# the cases of the forced-depth runs: the random assemblies, two spheres and two boxes, on lattices of 65 to 128 samples
def depth_cases():
    ball = shapes.sphere(r=1).make_part("ball")
    block = shapes.box(1, 1, 1).make_part("a")
    cases = {"random%d" % seed: (functools.partial(_random_assembly, seed, k, blended), None, 8) for seed, k, blended in RANDOM}
    cases["spheres"] = (lambda: cc.assembly("spheres", [ball, ball.translated(2.3, 0, 0)]), 0.05, 10)
    cases["boxes"] = (lambda: cc.assembly("boxes", [block, block.translated_x(1.25)]), 0.025, 16)
    return cases


def depth_case(name):
    """(assembly, resolution, [min_gaps]) of a forced-depth case."""
    build, resolution, gap_steps = depth_cases()[name]
    asm = build()
    if resolution is None:
        resolution = max(asm.shape().bounding_box().size()) / 90
    return asm, resolution, [0.0, gap_steps * resolution]


def forced_top_cells(dims, side):
    """The _MAX_TOP_CELLS that makes top_side(dims) return `side` (64 or 256) on a lattice that would take 16."""
    return int(numpy.prod(-(-numpy.asarray(dims, dtype=numpy.int64) // side)))


# ---- the tests ----------------------------------------------------------------------------------------------------------

def _same_bits(a, b):
    return numpy.array_equal(numpy.asarray(a, dtype=numpy.float32).view(numpy.uint32), numpy.asarray(b, dtype=numpy.float32).view(numpy.uint32))


@pytest.mark.parametrize("corner,step,dims", [
    ((-1.0, -0.5, -0.75), 2.0 ** -4, (40, 24, 30)),                          # dyadic: every product and sum exact
    ((-1.2345678, 0.7071068, -3.1415927), 0.0371234, (37, 29, 41)),         # products and sums that round
    ((10000.123, -9999.877, 10001.5), 0.0123, (64, 48, 33)),                # an ulp of the corner is 8 % of the step
])
def test_points_generated_per_axis_are_the_samples_of_grid_eval(corner, step, dims):
    corner, step = numpy.array(corner, dtype=numpy.float32), numpy.float32(step)
    centre = corner.astype(numpy.float64) + float(step) * numpy.array(dims) / 2
    ball = shapes.sphere(r=0.3).translated(*centre)
    knob = shapes.union([shapes.box(0.5, 0.3, 0.4), shapes.sphere(r=0.25).translated_x(0.2)], r=0.1).rotated((1, 2, 3), 33).translated(*centre)
    points, shape = axis_points(corner, step, (0, 0, 0), numpy.array(dims) - 1)
    assert shape == dims
    for shape_ in (ball, knob):
        tape = nodes.make_program(shape_)
        dense = oracle.grid_eval(tape, corner, step, dims, threads=4)[..., 3]
        assert (dense < 0).any() and (dense > 0).any()
        assert _same_bits(oracle.evaluate_points(tape, points)[:, 3].reshape(dims), dense)


@pytest.mark.parametrize("gap_steps", [0, 8])
@pytest.mark.parametrize("seed,k,blended", RANDOM)
def test_windowed_references_equal_the_dense_ones(seed, k, blended, gap_steps):
    asm = _random_assembly(seed, k, blended)
    resolution = max(asm.shape().bounding_box().size()) / 90
    gap = gap_steps * resolution
    instances, corner, step, dims, t = lattice_of(asm, resolution, gap)
    report = as_report(instances, corner, step, dims, gap)
    near = dense_near(report)
    assert near and windowed_near_of(instances, corner, step, dims, t) == near == windowed_near(report)
    if gap_steps == 0:
        pairs = dense_pairs(report)
        assert pairs and windowed_pairs_of(instances, corner, step, dims) == pairs == windowed_pairs(report)


@functools.lru_cache(maxsize=None)
def _inspected(name, gap):
    """(instances, corner, step, dims, t, wins, near reference, pairs reference) of a scenario's run."""
    sc = SCENARIOS[name]
    instances, corner, step, dims, t = lattice_of(sc.build(gap), sc.resolution, gap)
    report = as_report(instances, corner, step, dims, gap)
    wins = _instance_cells.windows(instances, corner, float(step), dims, grow=float(t))
    return instances, corner, step, dims, t, wins, sc.near(report), sc.pairs(report)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_every_scenario_has_its_top_side_and_something_to_find(name):
    sc = SCENARIOS[name]
    assert sc.gaps[0] == 0.0 and len(sc.gaps) >= 2 and all(g > 0 for g in sc.gaps[1:])
    for gap in sc.gaps:
        instances, corner, step, dims, t, wins, near, pairs = _inspected(name, gap)
        assert top_side(dims) == sc.side
        assert (wins[:, 1] >= wins[:, 0]).all()
        assert len(cell_rows(wins, dims, sc.side)) > 0
        assert len(_instance_cells.top_cells(instances, corner, float(step), dims, sc.side)) > 0
        assert near and pairs
        if gap == 0:
            assert {k: v[:3] for k, v in near.items()} == pairs
        else:
            assert all(pairs[k][0] < near[k][0] for k in pairs) and set(pairs) <= set(near)


@pytest.mark.parametrize("name", ["crowd64_blended", "crowd64_plain", "crowd33_blended"])
def test_crowds_have_pairs_in_both_words_of_the_mask(name):
    sc = SCENARIOS[name]
    asm = sc.build(0.0)
    n = 33 if "33" in name else 64
    every = list(asm.all_instances())
    visible_at = [k for k, i in enumerate(every) if i.visible]
    assert len(visible_at) == n and visible_at != list(range(n)) and every[0].visible and every[-1].visible      # hidden ones in between
    assert sum(isinstance(i, cc.assemblies.AssemblyTransform3D) for i in asm) == 2
    # the knobs are the blended ones or the plain ones (which programs then run is the device's choice: the GPU file)
    knobs = [nodes.make_program(i.part.data) for i in every if i.name == "knob"]
    other = [nodes.make_program(i.part.data) for i in _crowd(n, "blended" not in name).all_instances() if i.name == "knob"]
    assert len(knobs) >= 8 and not any(_same_bits(a, b) for a, b in zip(knobs, other))
    for gap in sc.gaps:
        instances, corner, step, dims, t, wins, near, pairs = _inspected(name, gap)
        assert len(instances) == n and max(dims) <= 96 + 8
        for found in (near, pairs):
            assert any(j < 32 for i, j in found)
            assert any(i < 32 <= j for i, j in found)
            assert any(j == n - 1 for i, j in found)
            if n == 64:
                assert any(i >= 32 for i, j in found)
        # a forced top side of 64 is possible on this lattice
        assert forced_top_cells(dims, 64) < int(numpy.prod(-(-dims // 16)))


@pytest.mark.parametrize("name", ["rods_x", "rods_y", "rods_z", "rods_y_65536"])
def test_rods_reach_the_last_indices_of_their_axis(name):
    sc = SCENARIOS[name]
    axis = "xyz".index(name[5])
    for gap in sc.gaps:
        instances, corner, step, dims, t, wins, near, pairs = _inspected(name, gap)
        assert dims[axis] == 65536 if name.endswith("65536") else 62000 <= dims[axis] <= 62001 + round(gap / sc.resolution)
        assert 8 <= dims[(axis + 1) % 3] <= 20 and 8 <= dims[(axis + 2) % 3] <= 20
        assert set(near) == {(0, 1), (0, 2), (1, 2)} == set(pairs)
        for found in (near, pairs):
            count, sums, (lo, hi) = found[(0, 1)][:3]
            assert lo[axis] <= 8 and hi[axis] >= dims[axis] - 9     # the whole length
            assert sums[axis] > 2 ** 32                       # the index sums need their 64 bits
            for pair in ((0, 2), (1, 2)):
                assert found[pair][2][0][axis] > 60000        # the whole index box of the pairs with the ball
        for pair in near:
            assert near[pair][3] >> 31, "overlapping pairs: a negative separation"
        assert near[(0, 2)][4][axis] > 60000 and near[(1, 2)][4][axis] > 60000       # the witnesses
        if name.endswith("65536"):
            assert near[(0, 1)][2][1][axis] == 65535 == pairs[(0, 1)][2][1][axis] + round(gap / sc.resolution / 2)


def _fields(name, gap):
    instances, corner, step, dims, t, wins, near, pairs = _inspected(name, gap)
    w = [oracle.grid_eval(nodes.make_program(i.shape()), corner, step, dims, threads=4)[..., 3] for i in instances]
    inwin = []
    for lo, hi in wins:
        m = numpy.zeros(tuple(dims), dtype=bool)
        m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
        inwin.append(m)
    return w, inwin


def test_dyadic_lattice_has_samples_exactly_on_the_thresholds():
    sc = SCENARIOS["dyadic"]
    for gap in sc.gaps:
        instances, corner, step, dims, t, wins, near, pairs = _inspected("dyadic", gap)
        # corner, step and t are exact: the lattice is the multiples of 2^-4
        assert step == 0.0625 and float(t) == gap / 2 and corner.tolist() == [-1.0 - gap / 2] * 3
        assert dims.tolist() == [33 + round(gap / 0.0625)] * 3
        w, inwin = _fields("dyadic", gap)
        outer, right, left = w
        zero = [(f == 0) for f in w]
        # samples ON the faces of the two halves, inside `outer`: w == 0 exactly, so not inside (interference) ...
        assert zero[1].sum() >= 6 * 15 * 15 and zero[2].sum() >= 6 * 15 * 15 and not zero[0].any()
        assert ((outer < 0) & zero[1]).sum() == zero[1].sum()
        signs = {bool(numpy.signbit(f[z]).any()) for f, z in zip(w[1:], zero[1:])} | {not bool(numpy.signbit(f[z]).all()) for f, z in zip(w[1:], zero[1:])}
        assert True in signs                                      # (which signs of zero the arithmetic gives: see below)
        # ... the strict count: 15^3 samples strictly inside a half whose 17^3 samples include its faces
        assert pairs[(0, 1)][0] == 15 ** 3 == pairs[(0, 2)][0] and (1, 2) not in pairs
        assert int(((outer < 0) & (right <= 0)).sum()) == 17 ** 3
        if gap == 0:
            assert (1, 2) not in near                             # they touch: v = 0 on the shared face, not < 0
            continue
        # samples at exactly t from a half, near `outer` and in both windows: excluded from "near"
        for k in (1, 2):
            at_t = (w[k] == t) & (outer < t) & inwin[0] & inwin[k]
            assert at_t.sum() >= 6 * 17 * 17
            assert near[(0, k)][0] == int(((w[k] < t) & (outer < t) & inwin[0] & inwin[k]).sum())
            assert near[(0, k)][0] + int(at_t.sum()) == int(((w[k] <= t) & (outer < t) & inwin[0] & inwin[k]).sum())
        # the two halves touch: the least v is exactly zero, on the 17 x 17 samples of the shared face (cells of 4^3
        # samples hold at most 4 x 4 of them), reported as +0.0 at the lexicographically first of them
        v = numpy.maximum(right, left)
        both = (right < t) & (left < t) & inwin[1] & inwin[2]
        assert v[both].min() == 0 and int((v[both] == 0).sum()) == 17 * 17
        count, sums, box, bits, witness = near[(1, 2)]
        first = tuple(int(k) for k in numpy.argwhere(both & (v == 0))[0])
        assert bits == 0 and witness == first == (18, 10, 10)


def test_dyadic_zero_signs():
    """Which zeros the box arithmetic produces on a face (both signs are compared bit for bit by order_key's one key
    for them): at least +0.0; a -0.0 is covered if present, and the reference canonicalises it."""
    w, _ = _fields("dyadic", 0.25)
    zeros = numpy.concatenate([f[f == 0] for f in w[1:]])
    assert len(zeros) and (~numpy.signbit(zeros)).any()


def test_plate_needs_a_top_side_of_64_on_its_own():
    sc = SCENARIOS["plate"]
    assert _instance_cells._MAX_TOP_CELLS == 1 << 15
    for gap in sc.gaps:
        instances, corner, step, dims, t, wins, near, pairs = _inspected("plate", gap)
        assert len(instances) == 12 and 2385 <= dims[0] <= 2420 and 2385 <= dims[1] <= 2420 and 17 <= dims[2] <= 32
        assert int(numpy.prod(-(-dims // 16))) > 1 << 15 >= int(numpy.prod(-(-dims // 64)))
        assert _instance_cells.levels(64, 1, None)[0] == [64, 16]
        # pairs in both clusters, at both ends of the index range
        assert any(box[1][0] < 200 and box[1][1] < 200 for _, _, box, *_ in near.values())
        assert any(box[0][0] > 2200 and box[0][1] > 2200 for _, _, box, *_ in near.values())
        assert any(box[1][0] < 200 for _, _, box in pairs.values()) and any(box[0][0] > 2200 for _, _, box in pairs.values())


@pytest.mark.parametrize("name", ["far_random", "far_gears"])
def test_far_scenarios_have_a_coarse_float32_and_one_placement(name):
    sc = SCENARIOS[name]
    asm = sc.build(0.0)
    assert asm.transform != cc.util.Transformation.zero() and asm.transform.quaternion.w != 1
    for gap in sc.gaps:
        instances, corner, step, dims, t, wins, near, pairs = _inspected(name, gap)
        for k in range(3):
            for coordinate in (corner[k], numpy.float32(corner[k] + step * numpy.float32(dims[k] - 1))):
                ulp = float(numpy.spacing(numpy.float32(abs(coordinate))))
                assert float(step) / 16 <= ulp <= float(step) / 4, (coordinate, ulp, step)
        # the assembly's transform applied to each listed instance instead: the same tapes, the same lattice
        other = lattice_of(per_instance(asm), sc.resolution, gap)
        assert [i.name for i in other[0]] == [i.name for i in instances]
        assert all(_same_bits(nodes.make_program(a.shape()), nodes.make_program(b.shape())) for a, b in zip(other[0], instances))
        assert _same_bits(other[1], corner) and other[2] == step and other[3].tolist() == dims.tolist()


@pytest.mark.parametrize("name", sorted(depth_cases()))
def test_depth_cases_can_be_forced_to_64_and_256(name, monkeypatch):
    asm, resolution, gaps = depth_case(name)
    for gap in gaps:
        dims = lattice_of(asm, resolution, gap)[3]
        assert 65 <= max(dims) <= 128 and top_side(dims) == 16
        for side, sides in ((64, [64, 16]), (256, [256, 64, 16])):
            monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", forced_top_cells(dims, side))
            assert top_side(dims) == side and _instance_cells.levels(side, 1, None)[0] == sides
            monkeypatch.undo()
