"""interference() and clearance() on the device at the edges of the cell traversal (csrc/instance_pairs.hip,
csrc/instance_cells.hpp, codecad_amd/_instance_cells.py), against the CPU oracle, bit for bit: counts, u64 index sums,
index boxes, the float32 bits of the separation and the witness.  No tolerance anywhere.

The scenarios and their references live in test_instance_cells_reference_host.py, which also proves without a device that
each scenario holds the edge it was built for:
  a. forced depth: top sides of 64 and 256 on small lattices (a child list feeding a child list), and an overflow of a
     middle level;
  b. 64 and 33 instances: the high word of the candidate mask, pairs across its two words, hidden instances between
     visible ones, nested subassemblies, full and distance-only programs;
  c. indices up to 65535 on each axis: the packing of cell rows and of the witness, the u64 index sums;
  d. strict thresholds on a dyadic lattice: samples with w == 0 and w == t exactly, a least separation of exactly zero
     with ties over many cells;
  e. a lattice that needs a top side of 64 on its own (about 2400 x 2400 x 24), against the windowed reference;
  f. far from the origin, through the assembly's own transform: a float32 ulp of a coordinate is a real part of a step.
"""
import functools

import pytest

import codecad_amd as cc
from codecad_amd import _instance_cells
from codecad_amd._instance_cells import top_side

from test_gpu_interference import dense_pairs, device_pairs
from test_gpu_clearance import dense_near, device_near, _same_as_interference
from test_instance_cells_reference_host import (SCENARIOS, depth_cases, depth_case, forced_top_cells, lattice_of, per_instance)

pytestmark = pytest.mark.gpu


def _check_both(asm, resolution, gap, near_reference, pairs_reference, side=None, **how):
    """clearance at `gap` (and, at gap 0, interference, which clearance must then equal) against the references ->
    (clearance report, interference report or None)."""
    near = cc.clearance(asm, resolution, gap, **how)
    if side is not None:
        assert top_side(near.dims) == side
    assert device_near(near) == near_reference(near)
    inter = None
    if gap == 0:
        inter = cc.interference(asm, resolution, **how)
        assert top_side(inter.dims) == top_side(near.dims)
        assert device_pairs(inter) == pairs_reference(inter)
        _same_as_interference(near, inter)
    return near, inter


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_matches_its_reference(hip, name):
    sc = SCENARIOS[name]
    for gap in sc.gaps:
        asm = sc.build(gap)
        near, inter = _check_both(asm, sc.resolution, gap, sc.near, sc.pairs, side=sc.side)
        assert near.pairs and near.traversals >= 1
        if sc.per_gap and gap != 0:                        # an assembly of its own for this gap: interference on it too
            inter = cc.interference(asm, sc.resolution)
            assert device_pairs(inter) == sc.pairs(inter) and inter.pairs


@pytest.mark.parametrize("name", ["crowd64_blended", "crowd64_plain"])
def test_sixty_four_instances_through_a_forced_level(hip, name, monkeypatch):
    """The high word of the mask through a k_instance_cells level more (top side 64)."""
    sc = SCENARIOS[name]
    gap = sc.gaps[1]
    asm = sc.build(gap)
    plain = cc.clearance(asm, sc.resolution, gap)
    monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", forced_top_cells(plain.dims, 64))
    assert top_side(plain.dims) == 64
    forced, _ = _check_both(asm, sc.resolution, gap, dense_near, dense_pairs, side=64)
    # with the blend the full programs run, without it every instance's distance-only one
    table, distance_only, lane_bytes = _instance_cells.device_table([i.instance for i in forced.instances], hip.queue)
    table.release()
    assert distance_only == (0 if "blended" in name else 1) and lane_bytes > 0
    assert forced.pairs == plain.pairs
    assert any(p.i >= 32 for p in forced.pairs) and any(p.i < 32 <= p.j for p in forced.pairs)


@functools.lru_cache(maxsize=None)
def _unforced(name):
    """[(gap, clearance report, its dense reference, interference report and reference at gap 0)] of a depth case."""
    asm, resolution, gaps = depth_case(name)
    out = []
    for gap in gaps:
        near = cc.clearance(asm, resolution, gap)
        inter = cc.interference(asm, resolution) if gap == 0 else None
        assert top_side(near.dims) == 16 and near.traversals <= 1
        out.append((gap, near, dense_near(near), inter, dense_pairs(inter) if inter else None))
    return asm, resolution, out


@pytest.mark.parametrize("overflow", [False, True], ids=["roomy", "overflowing"])
@pytest.mark.parametrize("side", [64, 256])
@pytest.mark.parametrize("name", sorted(depth_cases()))
def test_forced_depth(hip, name, side, overflow, monkeypatch):
    """Top sides of 64 (levels [64, 16]) and 256 ([256, 64, 16]) on lattices that take 16: the dense reference and the
    unforced run, pair for pair; then with first capacities of 3 rows, which every level with pairs below it overflows."""
    asm, resolution, runs = _unforced(name)
    how = {"initial_capacity": 3} if overflow else {}
    for gap, plain, near_reference, plain_inter, pairs_reference in runs:
        monkeypatch.setattr(_instance_cells, "_MAX_TOP_CELLS", forced_top_cells(plain.dims, side))
        assert top_side(plain.dims) == side
        near, inter = _check_both(asm, resolution, gap, lambda r: near_reference, lambda r: pairs_reference, side=side, **how)
        assert near.pairs == plain.pairs and near.dims.tolist() == plain.dims.tolist()
        if inter is not None:
            assert inter.pairs == plain_inter.pairs
        if overflow:
            for got in (near, inter):
                if got is not None and got.pairs:
                    assert got.traversals > 1
        monkeypatch.undo()


@pytest.mark.parametrize("name", ["far_random", "far_gears"])
def test_assembly_transform_equals_transforming_each_instance(hip, name):
    sc = SCENARIOS[name]
    for gap in sc.gaps:
        asm = sc.build(gap)
        whole, parts = cc.clearance(asm, sc.resolution, gap), cc.clearance(per_instance(asm), sc.resolution, gap)
        assert whole.pairs and whole.pairs == parts.pairs and whole.corner.tolist() == parts.corner.tolist()
        assert [i.name for i in whole.instances] == [i.name for i in lattice_of(asm, sc.resolution, gap)[0]]
    whole, parts = cc.interference(asm, sc.resolution), cc.interference(per_instance(asm), sc.resolution)
    assert whole.pairs and whole.pairs == parts.pairs
