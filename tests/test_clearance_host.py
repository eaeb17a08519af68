"""What the clearance check (codecad_amd/clearance.py) decides without a device: its argument checks, its lattice and
windows, its top-level cells and the argument checks of its entry points (the ISA of its kernels: test_assemblies.py)."""
import numpy
import pytest

import cells_abi
import codecad_amd as cc
from codecad_amd import shapes
from codecad_amd.interference import lattice as interference_lattice
from codecad_amd._instance_cells import top_cells as _top_cells, top_side as _top_side, cell_rows as _cell_rows, visible as _visible
from codecad_amd.clearance import half_gap, lattice, windows


def test_clearance_argument_checks_need_no_device():
    disc = shapes.circle(1).make_part("disc")
    with pytest.raises(ValueError, match="3D"):
        cc.clearance(cc.assembly("flat", [disc, disc.translated_x(1)]), 0.1, 0.1)
    ball = shapes.sphere(1).make_part("ball")
    crowd = cc.assembly("crowd", [ball.translated_x(i) for i in range(65)])
    with pytest.raises(ValueError, match="64"):
        cc.clearance(crowd, 0.1, 0.1)
    pair = cc.assembly("pair", [ball, ball.translated_x(1)])
    for bad in (0, -0.1, float("nan"), float("inf"), "0.1", None):
        with pytest.raises(ValueError, match="resolution"):
            cc.clearance(pair, bad, 0.1)
    with pytest.raises(ValueError, match="65536"):
        cc.clearance(pair, 1e-5, 0.1)
    with pytest.raises(ValueError, match="65536"):
        cc.clearance(pair, 1e-3, 100.0)             # the lattice grows with the gap
    with pytest.raises(ValueError, match="assembly"):
        cc.clearance(shapes.sphere(1), 0.1, 0.1)
    for bad in (-0.1, float("nan"), float("inf"), "0.1", None):
        with pytest.raises(ValueError, match="min_gap"):
            cc.clearance(pair, 0.1, bad)
    # one instance, or none visible: nothing to pair, no device work
    r = cc.clearance(cc.assembly("one", [ball, ball.hidden()]), 0.1, 0.5)
    assert r.pairs == [] and r.traversals == 0 and r.samples_evaluated == 0 and r.min_gap == 0.5


def test_clearance_lattice_and_windows():
    ball = shapes.sphere(2).make_part("ball")                  # radius 1
    far = cc.assembly("far", [ball, ball.translated_x(10)])   # boxes 8 apart along x
    inst = _visible(far, 0.25)
    # min_gap = 0: the interference lattice, windows and top cells
    corner, step, dims = lattice(inst, 0.25, half_gap(0))
    want = interference_lattice(inst, 0.25)
    assert corner.tolist() == want[0].tolist() and step == want[1] and dims.tolist() == want[2].tolist()
    wins = windows(inst, corner, step, dims, half_gap(0))
    assert _top_side(dims) == 16
    assert len(_cell_rows(wins, dims, 16)) == 0 == len(_top_cells(inst, corner, float(step), dims, 16))
    # min_gap = 7: both grown windows reach the top cells x 32..47 (they abut, 37 | 38, without overlapping)
    t = half_gap(7)
    corner, step, dims = lattice(inst, 0.25, t)
    assert corner.tolist() == [-4.375] * 3 and dims.tolist() == [76, 36, 36]
    wins = windows(inst, corner, step, dims, t)
    assert wins[:, :, 0].tolist() == [[0, 37], [38, 75]]
    rows = _cell_rows(wins, dims, _top_side(dims))
    assert len(rows) == 9 and set(rows[:, 2].tolist()) == {3} and set((rows[:, 0] & 0xffff).tolist()) == {32}
    # min_gap = 8: the windows overlap
    t = half_gap(8)
    corner, step, dims = lattice(inst, 0.25, t)
    wins = windows(inst, corner, step, dims, t)
    assert wins[0, 1, 0] >= wins[1, 0, 0]

    # by hand: unit spheres 3 apart, min_gap 0.5 -> t = 0.25, the union [-1, 4] x [-1, 1]^2 grown to [-1.25, 4.25] x ...
    two = cc.assembly("two", [shapes.sphere(r=1).make_part("a"), shapes.sphere(r=1).make_part("b").translated_x(3)])
    inst = _visible(two, 0.25)
    t = half_gap(0.5)
    assert t == numpy.float32(0.25)
    corner, step, dims = lattice(inst, 0.25, t)
    assert corner.tolist() == [-1.125] * 3 and dims.tolist() == [22, 10, 10]
    # lo = floor((A - t - corner - step) / step): (-1 - 0.25 + 1.125 - 0.25) / 0.25 = -1.5 -> -2 -> 0, (2 - ...) -> 10;
    # hi = ceil((B + t - corner + step) / step): (1 + 0.25 + 1.125 + 0.25) / 0.25 = 10.5 -> 11, (4 + ...) -> 23 -> 21
    assert windows(inst, corner, step, dims, t).tolist() == [[[0, 0, 0], [11, 9, 9]], [[10, 0, 0], [21, 9, 9]]]


def test_clearance_entry_points_reject_bad_arguments():
    """Every argument check comes before any device work.  max_parents = 0 throughout, so that not even a check that
    let something through could launch a kernel over the made-up pointers."""
    from codecad_amd.hip_util import _lib
    lib = _lib.load()
    fake = cells_abi.FAKE
    big = (8, 8, 65537)
    nan, inf = float("nan"), float("inf")

    def cells(thr=0.5, counter=fake, **broken):
        return lib.hu_clearance_cells_indirect(cells_abi.launch(**broken), cells_abi.children(thr=thr, counter_dev=counter))

    def finest(name, t=0.25, pairs=fake, **broken):
        return getattr(lib, name)(cells_abi.launch(**broken), t, pairs)

    bad = [cells(n=0), cells(n=65), cells(table_dev=None), cells(windows_dev=None), cells(counter=None), cells(dims=big),
           cells(step=-0.1), cells(step=nan), cells(step=inf), cells(thr=-1.0), cells(thr=nan)]
    for name in ("hu_clearance_leaf_indirect", "hu_clearance_witness_indirect"):
        bad += [finest(name, n=0), finest(name, n=65), finest(name, table_dev=None), finest(name, windows_dev=None),
                finest(name, pairs=None), finest(name, dims=big), finest(name, step=-0.1), finest(name, step=inf),
                finest(name, t=-0.25), finest(name, t=nan), finest(name, t=inf)]
    assert bad == [-3] * len(bad)
    nulls = cells_abi.launch(table_dev=None, windows_dev=None, parents_dev=None, n_parents_dev=None, evaluations_dev=None)
    assert lib.hu_clearance_leaf_indirect(nulls, 0.25, None) == -3
    assert b"NULL" in lib.hu_last_error()
    assert finest("hu_clearance_witness_indirect", t=nan) == -3 and b"t must be" in lib.hu_last_error()
