"""The launch record of a level (include/hip_util.h hu_level_launch) at the entry points themselves: what its list length
(n_parents_dev NULL or on the device) and its ownership (world, rank) select, for hu_subdivision_level and
hu_mass_properties_level alike, on one level of sponge(2): four parents of 8^3 cells of 1/24 -- the cube's central hole, the
hole of a face, the sub-sponge of an edge and the sub-sponge of a corner -- through the interpreter, against the oracle."""
import ctypes
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

Q, INT_STEP, DIMS = 1 / 72, 3, (8, 8, 8)
S = INT_STEP * Q
ORIGIN = (-0.5, -0.5, -0.5)
PARENTS = [(24, 24, 24), (24, 24, 0), (24, 0, 0), (0, 0, 0)]
FORMS = ("subdivision", "mass")


def parent_rows(mass):
    """The parents as the form's rows, tagged 5..8: integer corners, or fp64 corners."""
    rows = np.zeros((len(PARENTS), 4), np.float64 if mass else np.int32)
    rows[:, :3] = np.array(PARENTS, np.float64) * Q + np.array(ORIGIN) if mass else PARENTS
    rows[:, 3] = np.arange(len(PARENTS)) + 5
    return rows


@functools.lru_cache(maxsize=None)
def scene():
    """(the tape, the thresholds, the oracle's results): `natural` is a cell's half diagonal, under which every parent lists a
    part of its cells and the two sub-sponges have cells inside; `all_of_last` is just above the largest |distance| of the last
    parent's samples, under which ALL its cells are listed and those of the holes still are not."""
    import codecad_amd as cc
    tape = cc.nodes.make_program(cc.examples.sponge(2))
    step = np.float32(S)
    samples = [np.array([(p[c] + INT_STEP / 2) * Q + ORIGIN[c] for c in range(3)], np.float64).astype(np.float32) for p in PARENTS]
    assert [s.tolist() for s in samples] == [(r[:3] + S / 2).astype(np.float32).tolist() for r in parent_rows(True)]
    last = np.abs(oracle.grid_eval_pymcubes(tape, samples[-1], step, DIMS)).max()
    thresholds = {"natural": np.float32(S * 3 ** 0.5 / 2), "all_of_last": np.nextafter(np.float32(last), np.float32(1))}
    want = {}
    for name, thr in thresholds.items():
        for mass in (False, True):
            rows, counts, listed, sums = parent_rows(mass), [], [], []
            for row, corner in zip(rows, samples):
                if mass:
                    per_parent, n, cells = oracle.mass_properties(tape, corner, step, thr, DIMS)
                    sums.append(per_parent.tolist())
                    listed += [(row[0] + i * S, row[1] + j * S, row[2] + k * S, row[3]) for i, j, k, _ in cells.tolist()]
                else:
                    n, cells = oracle.subdivision_step(tape, corner, step, thr, DIMS)
                    listed += [tuple(int(row[c] + v * INT_STEP) for c, v in enumerate((i, j, k))) + (int(row[3]),) for i, j, k, _ in cells.tolist()]
                counts.append(n)
            want[name, mass] = (counts, sorted(listed), sums)
    return tape, thresholds, want


@pytest.fixture(scope="module")
def handle(hip):
    from codecad_amd import hip_util
    return hip_util.Tape(scene()[0], policy="0")


def classify(hip, handle, mass, rows, thr, count_dev=None, world=1, rank=0):
    """One launch over `rows` with room for every cell -> (the counter, the children's rows sorted, the sums or None);
    count_dev: the number of parents on the device (the launch covers all of `rows`), None: the direct form."""
    import torch
    from codecad_amd.hip_util import check
    from codecad_amd.hip_util._lib import LevelLaunch
    parents = torch.from_numpy(rows).cuda()
    capacity = len(rows) * 512
    children = torch.full((capacity, 4), -1, dtype=parents.dtype, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    n_parents = None if count_dev is None else torch.tensor([count_dev], dtype=torch.int32, device="cuda")
    sums = torch.zeros((len(rows), 10), dtype=torch.int32, device="cuda")
    launch = LevelLaunch(tape=handle.device_ptr, parents_dev=parents.data_ptr(), n_parents_dev=None if n_parents is None else n_parents.data_ptr(),
                         counter_dev=counter.data_ptr(), children_dev=children.data_ptr(), stream=None, max_parents=len(rows),
                         capacity=capacity, world=world, rank=rank, dims=DIMS, step=np.float32(S), thr=thr)
    torch.cuda.synchronize()
    if mass:
        check(hip.lib.hu_mass_properties_level(launch, S, sums.data_ptr()), "hu_mass_properties_level")
    else:
        check(hip.lib.hu_subdivision_level(launch, INT_STEP, 3, Q, (ctypes.c_double * 3)(*ORIGIN)), "hu_subdivision_level")
    torch.cuda.synchronize()
    got = int(counter.item())
    assert got <= capacity
    return got, sorted(map(tuple, children[:got].cpu().numpy().tolist())), sums.cpu().numpy().view(np.uint32) if mass else None


@pytest.mark.parametrize("form", FORMS)
def test_world_one_with_a_device_count_is_the_direct_form(hip, handle, form):
    """world = 1, rank = 0 and the count on the device against a NULL n_parents_dev and max_parents = 4: the same counter, the same
    set of child rows, byte-equal sums -- the oracle's."""
    mass = form == "mass"
    _, thresholds, want = scene()
    counts, listed, sums = want["natural", mass]
    assert all(0 < n < 512 for n in counts) and (not mass or any(any(s) for s in sums))
    counted = classify(hip, handle, mass, parent_rows(mass), thresholds["natural"], count_dev=4, world=1, rank=0)
    direct = classify(hip, handle, mass, parent_rows(mass), thresholds["natural"])
    assert counted[0] == direct[0] == sum(counts) and counted[1] == direct[1] == listed
    if mass:
        assert counted[2].tobytes() == direct[2].tobytes() and direct[2].tolist() == sums


@pytest.mark.parametrize("world", (2, 3))
@pytest.mark.parametrize("form", FORMS)
def test_a_direct_list_with_ownership_partitions_the_level(hip, handle, form, world):
    """n_parents_dev = NULL with world >= 2, which no entry point could say before the record: the ranks' child lists are pairwise
    disjoint, their union is the world = 1 list, and their sums add up to its sums exactly, in uint32."""
    mass = form == "mass"
    _, thresholds, want = scene()
    whole = classify(hip, handle, mass, parent_rows(mass), thresholds["natural"])
    assert whole[1] == want["natural", mass][1]
    shares = [classify(hip, handle, mass, parent_rows(mass), thresholds["natural"], world=world, rank=rank) for rank in range(world)]
    sets = [set(share[1]) for share in shares]
    assert all(len(s) == share[0] == len(share[1]) > 0 for s, share in zip(sets, shares))
    assert all(not (sets[a] & sets[b]) for a in range(world) for b in range(a + 1, world))
    assert set().union(*sets) == set(whole[1]) and sum(share[0] for share in shares) == whole[0]
    if mass:
        added = np.add.reduce(np.stack([share[2] for share in shares]), axis=0, dtype=np.uint32)
        assert added.dtype == np.uint32 and added.tobytes() == whole[2].tobytes() and whole[2].any()


@pytest.mark.parametrize("form", FORMS)
def test_a_device_count_ends_the_list_before_its_capacity(hip, handle, form):
    """A device count of 3 in a list of max_parents = 4 whose fourth row is a parent ALL of whose cells would be listed: the result
    of a direct launch of the first three rows, and nothing summed for the fourth."""
    mass = form == "mass"
    _, thresholds, want = scene()
    counts, listed, sums = want["all_of_last", mass]
    assert counts[3] == 512 and 0 < sum(counts[:3]) < 3 * 512
    rows = parent_rows(mass)
    counted = classify(hip, handle, mass, rows, thresholds["all_of_last"], count_dev=3)
    direct = classify(hip, handle, mass, rows[:3].copy(), thresholds["all_of_last"])
    assert counted[0] == direct[0] == sum(counts[:3])
    assert counted[1] == direct[1] == [row for row in listed if row[3] != 8]
    if mass:
        assert counted[2][:3].tobytes() == direct[2].tobytes() and direct[2].tolist() == sums[:3] and not counted[2][3].any()
    whole = classify(hip, handle, mass, rows, thresholds["all_of_last"], count_dev=4)
    assert whole[0] == sum(counts) and whole[1] == listed        # (with its count the fourth parent does list all of its cells)
