"""The in-range flag of the fast square root on the device, at its limit (host side: test_inrange_flag_host.py, which also
shows that the grids used here lie on the side of the limit they claim).  A launch of per-tape code whose largest |sample
coordinate| is below the tape's coordinate limit B skips the range test of every rectangle and extrusion corner; these tests
put grids within a few binary32 ulps of B, just beyond it and far beyond it (sums of squares past 2^100, the IEEE branch),
for every op family the analysis bounds, through every launch family that decides the flag: dense grids in both layouts,
ragged grids, slabs, leaf blocks, the classification kernels and the level kernels.  Every float must be the oracle's."""
import ctypes
import math

import numpy as np
import pytest

import inrange_scenes as sc
import oracle
from test_gpu_bricks import check_blocks, check_classify, check_dense, check_slab

pytestmark = pytest.mark.gpu

CLASSIFIED = ("box_scaled_down", "box_rot_general", "cyl")     # these carry every kernel family, the rest grids and blocks
_handles = {}


@pytest.fixture(scope="module")
def spec(hip):
    """name -> (handle, tape): one specialisation per scene for the whole module"""
    from codecad_amd import hip_util

    def get(name):
        if name not in _handles:
            tape = sc.BY_NAME[name].device_tape()
            handle = hip_util.Tape(tape)
            handle.specialize(hip_util.SPEC_ALL if name in CLASSIFIED else hip_util.SPEC_DENSE | hip_util.SPEC_BLOCKS)
            _handles[name] = (handle, tape)
        return _handles[name]
    yield get
    for handle, _ in _handles.values():
        handle.release()
    _handles.clear()


@pytest.mark.parametrize("name", sc.FINITE)
def test_dense_grids_at_the_limit(hip, spec, name):
    """Brick-shaped and ragged grids whose outermost samples are the last for which the flag is set, their twins at four
    times the distance (no flag; sums of squares beyond 2^100), and a grid through the origin at the limit's scale.
    `repetition`: x and y small and off the repetition's lattice, z at the limit; its twin at eight times the distance."""
    handle, tape = spec(name)
    for dims in ((16, 16, 32), (13, 10, 9)):
        for above in (False, True):
            check_dense(hip, handle, tape, *sc.far_grid(name, dims, above))
    check_dense(hip, handle, tape, *sc.origin_grid(name))


@pytest.mark.parametrize("name", ("box", "box_scaled_down", "box_rot_general", "box_translated", "cyl"))
def test_slabs_at_the_limit(hip, spec, name):
    """Planes 8.. of the grid lie at or beyond B: a slab of the planes below it (the launch's reach is the whole grid's, so the
    flag is off), and a slab of the planes beyond.  And with the flag ON: slabs of the last grid below the limit."""
    handle, tape = spec(name)
    corner, step, dims = sc.far_grid(name, (16, 16, 32))
    check_slab(hip, handle, tape, corner, step, dims, 4, 8)
    check_slab(hip, handle, tape, corner, step, dims, 8, 8)
    corner, step, dims = sc.crossing_x(name, 8)
    check_slab(hip, handle, tape, corner, step, dims, 0, 8)
    check_slab(hip, handle, tape, corner, step, dims, 8, 8)
    check_slab(hip, handle, tape, corner, step, dims, 4, 8)


@pytest.mark.parametrize("name", ("box", "box_scaled_down", "box_rot_general", "nested", "cyl", "mirror_symm"))
def test_leaf_blocks_across_the_limit(hip, spec, name):
    """Two blocks of one launch, one either side of B along x (corner * resolution + origin); edges 16 and 17."""
    handle, tape = spec(name)
    b = sc.limit_of(name)
    q = sc.quantum(b)
    m = math.ceil(b / q)
    origin = (m * q, (m - 60) * q, (m - 60) * q)
    corners = [(-20, 0, 0), (4, 0, 0), (-20, 8, 24), (4, -8, 3)]
    for edge in (16, 17):
        x = np.array([c[0] for c in corners], np.float64) * q + origin[0]
        assert np.any(x + (edge - 1) * q < b) and np.any(x >= b)
        check_blocks(hip, handle, tape, corners, q, origin, edge)


def _classify_with(hip, handle, tape, corner, step, dims, thr):
    """subdivision_step and mass_properties at a threshold of the caller's: count, index set and sums exact"""
    from codecad_amd import hip_util
    c4 = np.zeros(4, np.float32)
    c4[:3] = corner
    cells = dims[0] * dims[1] * dims[2]
    counter = hip_util.Buffer(np.uint32, 1)
    lst = hip_util.Buffer(hip_util.Buffer.quad_dtype(np.uint8), cells)
    sums = hip_util.Buffer(np.uint32, 10)
    want_n, want = oracle.subdivision_step(tape, corner, step, thr, dims)
    assert 0 < want_n < cells
    ev = counter.enqueue_fill(0)
    hip.k.subdivision_step(dims, None, handle, c4, step, thr, counter, lst, wait_for=[ev]).wait()
    got_n = int(counter.read()[0])
    assert got_n == want_n
    assert sorted(map(tuple, lst.read().view(np.uint8).reshape(-1, 4)[:got_n].tolist())) == sorted(map(tuple, want.tolist()))
    want_sums, want_n, want = oracle.mass_properties(tape, corner, step, thr, dims)
    sums.enqueue_fill(0)
    counter.enqueue_fill(0)
    hip.k.mass_properties(dims, None, handle, c4, step, thr, sums, counter, lst).wait()
    assert sums.read().tolist() == want_sums.tolist()
    got_n = int(counter.read()[0])
    assert got_n == want_n
    assert sorted(map(tuple, lst.read().view(np.uint8).reshape(-1, 4)[:got_n].tolist())) == sorted(map(tuple, want.tolist()))
    for b in (counter, lst, sums):
        b.release()


@pytest.mark.parametrize("name", CLASSIFIED)
def test_classification_at_the_limit(hip, spec, name, monkeypatch):
    """check_classify's thresholds are a cell's half diagonal (about 2^26 where the distances are 2^48 to 2^50): out there its
    lists are empty and its sums zero, so it would only catch a grossly wrong distance.  The grids at the limit are
    therefore classified once more at the median |distance| of the grid, where about half the cells are listed and the list
    turns on the distances' last bits."""
    handle, tape = spec(name)
    monkeypatch.setenv("HU_CLASSIFY_BOX_MIN", "1")     # (over boxes, as test_classification_over_boxes)
    for above in (False, True):
        corner, step, dims = sc.far_grid(name, (16, 16, 32), above)
        check_classify(hip, handle, tape, corner, step, dims)
        thr = np.float32(np.median(np.abs(oracle.grid_eval_pymcubes(tape, corner, step, dims))))
        _classify_with(hip, handle, tape, corner, step, dims, thr)
    check_classify(hip, handle, tape, *sc.origin_grid(name))


def _level_parents(name):
    b = sc.limit_of(name)
    q = sc.quantum(b)
    m = math.ceil(b / q)
    return q, (m * q, (m - 60) * q, (m - 60) * q), [(-40, 0, 0), (-20, 4, 8), (4, 0, 0), (24, -4, 2)]


@pytest.mark.parametrize("name", CLASSIFIED)
def test_subdivision_level_across_the_limit(hip, spec, name, monkeypatch):
    """hu_subdivision_level: four parents of 8^3 cells straddling B along x, against the oracle's subdivision_step per parent.
    (The threshold is a distance from the middle of the field, so that about half the cells are listed and the list depends
    on the distances' last bits; out there nothing is within a cell's diagonal of the surface.)"""
    import torch
    from codecad_amd.hip_util import check
    from codecad_amd.hip_util._lib import LevelLaunch
    handle, tape = spec(name)
    monkeypatch.setenv("HU_CLASSIFY_BOX_MIN", "1")
    q, origin, parents = _level_parents(name)
    int_step, dims = 2, (8, 8, 8)
    step = np.float32(int_step * q)
    sample = [np.array([(p[c] + int_step / 2) * q + origin[c] for c in range(3)], np.float64).astype(np.float32) for p in parents]
    thr = np.float32(np.median(np.abs(oracle.grid_eval_pymcubes(tape, sample[1], step, dims))))
    rows = np.zeros((len(parents), 4), np.int32)
    rows[:, :3] = parents
    rows[:, 3] = np.arange(len(parents)) + 5
    want = []
    for row, corner in zip(rows, sample):
        n, cells = oracle.subdivision_step(tape, corner, step, thr, dims)
        want += [(int(row[0] + i * int_step), int(row[1] + j * int_step), int(row[2] + k * int_step), int(row[3])) for i, j, k, _ in cells.tolist()]
        assert n == len(cells)
    assert 0 < len(want) < len(parents) * 512
    cap = len(parents) * 512
    parents_dev = torch.from_numpy(rows).cuda()
    children = torch.full((cap, 4), -1, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    launch = LevelLaunch(tape=handle.device_ptr, parents_dev=parents_dev.data_ptr(), n_parents_dev=None, counter_dev=counter.data_ptr(),
                         children_dev=children.data_ptr(), stream=None, max_parents=len(parents), capacity=cap, world=1, rank=0, dims=dims,
                         step=step, thr=thr)
    check(hip.lib.hu_subdivision_level(launch, int_step, 3, float(q), (ctypes.c_double * 3)(*origin)), "hu_subdivision_level")
    torch.cuda.synchronize()
    got_n = int(counter.item())
    assert got_n == len(want)
    assert sorted(map(tuple, children[:got_n].cpu().numpy().tolist())) == sorted(want)


@pytest.mark.parametrize("name", CLASSIFIED)
def test_mass_properties_level_across_the_limit(hip, spec, name, monkeypatch):
    """hu_mass_properties_level (its parents are fp64 corners on the device, so its launches never set the flag): the same
    four parents against the oracle's mass_properties per parent -- the ten sums, the count and the children."""
    import torch
    from codecad_amd.hip_util import check
    from codecad_amd.hip_util._lib import LevelLaunch
    handle, tape = spec(name)
    monkeypatch.setenv("HU_CLASSIFY_BOX_MIN", "1")
    q, origin, parents = _level_parents(name)
    s, dims = 2 * q, (8, 8, 8)
    step = np.float32(s)
    rows = np.zeros((len(parents), 4), np.float64)
    rows[:, :3] = np.array(parents, np.float64) * q + np.array(origin)
    rows[:, 3] = np.arange(len(parents)) + 5
    sample = [(r[:3] + s / 2).astype(np.float32) for r in rows]
    thr = np.float32(np.median(np.abs(oracle.grid_eval_pymcubes(tape, sample[1], step, dims))))
    want_sums, want = [], []
    for r, corner in zip(rows, sample):
        sums, n, cells = oracle.mass_properties(tape, corner, step, thr, dims)
        want_sums.append(sums.tolist())
        want += [(r[0] + i * s, r[1] + j * s, r[2] + k * s, r[3]) for i, j, k, _ in cells.tolist()]
        assert n == len(cells)
    assert 0 < len(want) < len(parents) * 512
    cap = len(parents) * 512
    parents_dev = torch.from_numpy(rows).cuda()
    children = torch.full((cap, 4), float("nan"), dtype=torch.float64, device="cuda")
    sums_dev = torch.zeros((len(parents), 10), dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    launch = LevelLaunch(tape=handle.device_ptr, parents_dev=parents_dev.data_ptr(), n_parents_dev=None, counter_dev=counter.data_ptr(),
                         children_dev=children.data_ptr(), stream=None, max_parents=len(parents), capacity=cap, world=1, rank=0, dims=dims,
                         step=step, thr=thr)
    check(hip.lib.hu_mass_properties_level(launch, float(s), sums_dev.data_ptr()), "hu_mass_properties_level")
    torch.cuda.synchronize()
    got_n = int(counter.item())
    assert got_n == len(want)
    assert sums_dev.cpu().numpy().view(np.uint32).tolist() == want_sums
    assert sorted(map(tuple, children[:got_n].cpu().numpy().tolist())) == sorted(want)


@pytest.mark.parametrize("name", ("thin_ok", "thin_bad", "thin_worse"))
def test_thin_features(hip, spec, name):
    """A 4 x 4 x 8 grid stepping one binary32 ulp of 2^-25 (2^-48), centred on a corner of the thin box, and one whose x steps
    across a face while y and z stay inside the box's extent: the smallest corner distances there are."""
    handle, tape = spec(name)
    half = {"thin_ok": sc.THIN_OK_HALF, "thin_bad": sc.THIN_BAD_HALF, "thin_worse": sc.THIN_WORSE_HALF}[name]
    step = np.float32(2.0 ** -48 if name != "thin_worse" else 2.0 ** -50)
    h = np.array(half, np.float64)
    corner = h - float(step) * np.array([2, 2, 4])
    assert corner.astype(np.float32).astype(np.float64).tolist() == corner.tolist()
    check_dense(hip, handle, tape, corner, step, (4, 4, 8))
    face = np.array([corner[0], -float(step) * 2, -float(step) * 4])
    check_dense(hip, handle, tape, face, step, (4, 4, 8))
    check_dense(hip, handle, tape, -corner - float(step) * np.array([3, 3, 7]), step, (4, 4, 8))     # the opposite corner


@pytest.mark.parametrize("name", [s.name for s in sc.SCENES if s.expect != "finite" and not s.name.startswith("thin")])
def test_tapes_without_a_limit_and_without_corners(hip, spec, name):
    """Limit 0 (an op the analysis does not bound feeds an extrusion: no launch sets the flag) and +inf (no rectangle, no
    extrusion: every launch does) on a grid at coordinates around 2^60 and on a tiny one."""
    handle, tape = spec(name)
    far = 2.0 ** 60
    check_dense(hip, handle, tape, np.array([far, -far, far / 2]), np.float32(2.0 ** 40), (16, 16, 32))
    check_dense(hip, handle, tape, np.array([-8.0, -8.0, -16.0]) * 2.0 ** -40, np.float32(2.0 ** -40), (16, 16, 32))
    check_dense(hip, handle, tape, np.array([-0.47, -0.51, -0.49]) * 8, np.float32(0.61), (13, 10, 9))
