"""The scenes of test_gpu_cells_workgroup_shapes.py, inspected without a device: the slot counts of the heavy parts, the
register file hu_instance_table gives every scene, the workgroup each kernel over an assembly's cells lands on
(heavy_instances.cells_lanes restates host.hpp hu_workgroup), and that each scene's reference holds what it is there for --
the heavy instance overlaps light ones, has a near pair that does not overlap, is cut on two layers or more and changes
every family's reference when it is taken out."""
import ctypes

import numpy
import pytest

from codecad_amd import nodes, _instance_cells
from codecad_amd.hip_util import _lib

import assembly_mass_scenes as mass_scenes
import cells_abi
import assembly_picture_scenes as aps
import heavy_instances as hi

L128, L64 = 128, 64


def test_the_knot_of_the_picture_scenes_is_level_four():
    assert numpy.array_equal(nodes.make_program(hi.knot(4, 0.1).scaled(0.15)), nodes.make_program(aps.knot()))
    assert aps.n_slots(nodes.make_program(aps.knot())) == 9


@pytest.mark.parametrize("level,floats,full,plain", [(4, 551, 9, (8, 4)), (5, None, 11, (10, 5)), (6, 2279, 13, (12, 6)), (7, 4583, 15, (14, 7))])
def test_slots_of_the_knots(level, floats, full, plain):
    rounded, straight = nodes.make_program(hi.knot(level, 0.1)), nodes.make_program(hi.knot(level, -1))
    assert floats is None or len(rounded) == len(straight) == floats
    assert hi.slots(rounded) == (full, None)                         # a rounded blend has no distance-only program
    assert hi.slots(straight) == (full, plain)
    assert aps.n_slots(rounded) == full


def test_the_plain_knot_passes_192_bytes_at_level_six():
    per_lane = {level: 16 * p + 4 * r for level in (5, 6) for p, r in [hi.slots(nodes.make_program(hi.knot(level, -1)))[1]]}
    assert per_lane == {5: 180, 6: 216}


def test_a_part_with_25_slots_within_5000_floats():
    tape = nodes.make_program(hi.knot25())
    assert len(tape) <= 5000 and hi.slots(tape) == (25, None)
    assert hi.slots(nodes.make_program(hi.knot(5, 0.1, "xyz")))[0] == 21 and hi.slots(nodes.make_program(hi.knot(6, 0.1, "xy")))[0] == 19


def test_the_workgroup_rule():
    assert [hi.cells_lanes(b) for b in (0, 192, 196, 384, 388, 2558)] == [256, 256, 128, 128, 64, 64]
    assert hi.cells_lanes(144, 256) == 64 and hi.cells_lanes(208, 8) == 128
    assert hi.cells_lds(192) == 48 * 1024 + 128 and hi.cells_lds(2558) == 160 * 1024
    with pytest.raises(ValueError):
        hi.cells_lds(2560)


# scene -> (distance_only, lane_bytes, lanes of every kernel but the six with 4 bytes per instance, lanes of those six)
FIGURES = {
    "heavy_pair": (0, 208, L128, L128),
    "heavy_plain": (1, 216, L128, L128),
    "heavy_pair25": (0, 400, L64, L64),
    "heavy_64": (0, 208, L128, L64),
}
PER_INSTANCE = {"clearance leaf", "clearance witness", "section tiles with distance",
                "separation cells", "separation leaf", "separation witness"}
# the kernels of separation() and assembly_voxels(), spelled out for every scene from the rule (208 + 16 and 216 + 16 B per
# lane: 128 lanes; 208 + 256: 64; 400 and more: 64)
NEW_KERNELS = {
    "heavy_pair": {"separation cells": L128, "separation leaf": L128, "separation witness": L128, "voxel cells": L128, "voxel leaf": L128},
    "heavy_plain": {"separation cells": L128, "separation leaf": L128, "separation witness": L128, "voxel cells": L128, "voxel leaf": L128},
    "heavy_pair25": {"separation cells": L64, "separation leaf": L64, "separation witness": L64, "voxel cells": L64, "voxel leaf": L64},
    "heavy_64": {"separation cells": L64, "separation leaf": L64, "separation witness": L64, "voxel cells": L128, "voxel leaf": L128},
}


def expected_lanes(name):
    """THE TABLE: {kernel: lanes} of a scene."""
    distance_only, lane_bytes, most, per_instance = FIGURES[name]
    return {kernel: per_instance if kernel in PER_INSTANCE else most for kernel in hi.kernel_extras(1)}


@pytest.mark.parametrize("name", sorted(hi.SCENES))
def test_lanes_of_every_kernel(name):
    instances = hi.instances_of(name)
    assert hi.table_figures(instances) == FIGURES[name][:2]
    assert len(instances) == (64 if name == "heavy_64" else 4)
    assert hi.lanes_table(instances) == expected_lanes(name)
    assert set(hi.kernel_extras(len(instances))) == set(expected_lanes(name)) and len(expected_lanes(name)) == 22
    assert {k: expected_lanes(name)[k] for k in NEW_KERNELS[name]} == NEW_KERNELS[name]
    extras = hi.kernel_extras(len(instances))
    assert [extras[k] for k in sorted(NEW_KERNELS[name])] == [4 * len(instances)] * 3 + [0, 0]


def test_every_kernel_reaches_128_and_64_lanes_through_a_genuine_register_file():
    for lanes in (L128, L64):
        reached = {k for name in FIGURES for k, v in expected_lanes(name).items() if v == lanes}
        assert reached == set(hi.kernel_extras(1))


def test_a_scene_without_its_heavy_part_fails_the_table():
    light = _instance_cells.visible(hi.without_heavy("heavy_pair"), hi.PAIR_RESOLUTION)
    assert len(light) == 4 and hi.lanes_table(light) != expected_lanes("heavy_pair")
    assert set(hi.lanes_table(light).values()) == {256}


LIMITS = {"heavy_64": 48}          # samples a side; the pair scenes stay within 40


def shares_cells(rows, heavy, mask_of=lambda row: row[-1]):
    """Some listed cell holds a heavy candidate and a light one."""
    bits = sum(1 << k for k in heavy)
    return any(mask_of(row) & bits and mask_of(row) & ~bits for row in rows)


@pytest.mark.parametrize("name", sorted(hi.SCENES))
def test_a_scene_keeps_its_edge(name):
    asm, resolution, gap = hi.scene(name)
    heavy = set(hi.HEAVY_INDEX[name])
    instances = hi.instances_of(name)
    assert [k for k, i in enumerate(instances) if i.name == "knot"] == sorted(heavy)
    pairs, near0, dims = hi.pairs_reference(name, 0.0)
    _, near, dims_gap = hi.pairs_reference(name, gap)
    assert max(dims) <= LIMITS.get(name, 40) and max(dims_gap) <= LIMITS.get(name, 40) + 2
    # overlap samples of a heavy part with light ones; a pair of a heavy and a light part within the gap that does not overlap
    mixed = [k for k in pairs if (k[0] in heavy) != (k[1] in heavy)]
    assert len(mixed) >= 2 and all(pairs[k][0] >= 1 for k in mixed) and sum(pairs[k][0] for k in mixed) >= 16
    apart = [k for k in near if (k[0] in heavy) != (k[1] in heavy) and k not in pairs]
    assert apart and all(not near[k][3] >> 31 for k in apart)                             # positive separations
    # cut area, segments and triangles of its own, on at least two layers and in at least two top cells
    cut = hi.section_reference(name)
    assert max(cut.dims) <= 64
    assert all(cut.acc[(k, k)][0] >= 4 for k in heavy) and any((k[0] in heavy) != (k[1] in heavy) for k in cut.acc if k[0] != k[1])
    assert all(hi.outlines_reference(name).counts[k] >= 8 for k in heavy)
    layers = hi.layers_reference(name)
    assert len(layers.heights) == 3 and all((layers.layer_counts[:, k] > 0).sum() >= 2 for k in heavy)
    meshes = hi.meshes_reference(name)
    side = _instance_cells.top_side(numpy.asarray(meshes.dims) + 1)
    for k in heavy:
        own = meshes.triangles[meshes.triangles["k"] == k]
        assert len(own) >= 100
        assert len({(int(a) // side, int(b) // side, int(c) // side) for a, b, c in zip(own["a"], own["b"], own["c"])}) >= 2
    mass = hi.mass_reference(name)
    assert all(mass.sums[k][0] >= 50 for k in heavy) and any(mass.owned[k][0] < mass.sums[k][0] for k in range(len(instances)))
    # in every traversal reference a heavy instance is a candidate in cells that also hold light ones
    assert shares_cells(hi.meshes_traversal(name).rows[-1], heavy) and shares_cells(hi.outlines_traversal(name).rows[-1], heavy)
    assert shares_cells(hi.layers_traversal(name).rows[-1], heavy)
    corner, step, lattice = hi.lattice3(name)[1:]
    top = _instance_cells.top_side(lattice)
    assert shares_cells(_instance_cells.top_cells(instances, corner, float(step), lattice, top), heavy, lambda r: int(r[2]) | int(r[3]) << 32)
    assert shares_cells(mass_scenes.top_rows(instances, corner, step, lattice, top), heavy)


@pytest.mark.parametrize("name", sorted(hi.SCENES))
def test_removing_the_heavy_parts_changes_every_reference(name):
    asm, resolution, gap = hi.scene(name)
    light = hi.without_heavy_references(name)
    assert light["near"] != hi.pairs_reference(name, gap)[1]
    assert light["section"] != hi.section_reference(name).acc
    assert light["outlines"] != hi.outlines_reference(name).counts.tolist()
    assert light["layers"] != hi.layers_reference(name).layer_counts.tolist()
    assert light["meshes"] != hi.meshes_reference(name).counts.tolist()
    assert light["mass"] != hi.mass_reference(name).sums
    assert light["voxels"] != hi.voxels_reference(name).counts
    (light_dense, light_traversal), (dense, traversal) = light["separation"], hi.separation_reference(name)
    assert not numpy.array_equal(light_dense.keys, dense.keys) and not numpy.array_equal(light_traversal.keys, traversal.keys)
    assert light_traversal.evaluations != traversal.evaluations


@pytest.mark.parametrize("name", sorted(hi.SCENES))
def test_the_separation_traversal_of_a_heavy_scene_is_the_dense_minimum(name):
    """The branch and bound assumes distances of Lipschitz constant at most 1 (codecad_amd/separation.py): the scaled knots
    keep it, on every scene the traversal loses no minimum and no witness, and a heavy part's pairs are among them."""
    dense, traversal = hi.separation_reference(name)
    n = len(hi.instances_of(name))
    assert numpy.array_equal(dense.keys, traversal.keys) and dense.witness == traversal.witness
    assert set(dense.witness) == {(i, j) for i in range(n) for j in range(i + 1, n)}
    heavy = set(hi.HEAVY_INDEX[name])
    mixed = [pair for pair in dense.witness if (pair[0] in heavy) != (pair[1] in heavy)]
    assert any(dense.keys[pair] < 0x80000000 for pair in mixed) and any(dense.keys[pair] > 0x80000000 for pair in mixed)   # overlapping, apart
    assert traversal.level_rows[-1] > 0 and traversal.evaluations > 0


def test_the_voxel_references_of_the_heavy_scenes_write_the_dense_volume():
    for name in sorted(hi.SCENES):
        for retire in (True, False):
            ref = hi.voxels_reference(name, retire)
            assert numpy.array_equal(ref.written, ref.ids) and ref.traversal_counts == ref.counts and ref.premise_broken == 0
            assert all(ref.counts[k] > 0 for k in hi.HEAVY_INDEX[name])


def test_the_regimes_a_larger_register_file_reaches():
    """random_5 (12 instances, 32 B per lane) starts at 256 lanes and reaches all four; solids64's separation (64 instances:
    20 + 256 B per lane) starts at 128 lanes and reaches the three below it; the mass scene `blend` all four."""
    import separation_scenes
    # neither scene of few instances lists two levels above the finest one from its own top side, 16: the padded run forces 256
    for name in ("random_5", "gears"):
        assert separation_scenes.traversal_reference(name).side == 16 and len(separation_scenes.traversal_reference(name).level_rows) == 1
    forced = separation_scenes.traversal_reference("random_5", 256)
    assert len(forced.level_rows) == 3 and all(rows > 0 for rows in forced.level_rows)
    five, solids, blend = (mass_scenes.scene(name)[2] for name in ("random_5", "solids64", "blend"))
    assert hi.table_figures(five) == (0, 32) and len(five) == 12 and hi.regimes_of(32, 48) == hi.REGIMES
    assert hi.table_figures(solids) == (1, 20) and len(solids) == 64 and hi.cells_lanes(20, 256) == 128
    assert hi.regimes_of(20, 256) == ["64 lanes", "64 lanes above 64 KiB", "the largest LDS"]
    assert hi.cells_lds(2292, 256) == 64 * 2548 + 128 <= hi.MAX_LDS        # solids64's largest: 20 + 2272 B of registers per lane
    with pytest.raises(ValueError):
        hi.cells_lds(2308, 256)
    assert hi.table_figures(blend) == (0, 32) and hi.regimes_of(32, 0) == hi.REGIMES
    assert hi.regimes_of(400, 0) == ["64 lanes above 64 KiB", "the largest LDS"] and hi.regimes_of(1600, 0) == ["the largest LDS"]


def test_lane_bytes_that_are_no_multiple_of_four_are_refused():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    for lane_bytes in (2, 66, 209):
        launch = cells_abi.launch(distance_only=0, lane_bytes=lane_bytes, **cells_abi.held(p, (8, 8, 8)))
        assert lib.hu_interference_leaf_indirect(launch, p) == -3
        assert "multiple of 4" in lib.hu_last_error().decode()
