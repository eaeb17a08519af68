"""Host proofs of the coordinate limit (csrc/specialise.hpp coordinate_limit, read through hu_tape_coordinate_limit): a launch
whose sample coordinates stay below it skips the range tests of the fast square root in every `perp_w_x`, so the limit has
to keep every sum of squares inside [2^-100, 2^100] -- for every op family a tape can pass through on its way to a rectangle
or an extrusion.  The operands are computed here in NumPy float64 from the shapes' definitions (inrange_scenes.py), never
from library code; the grids that test_gpu_inrange_flag.py launches are shown to lie on the side of the limit they claim."""
import ctypes
import math

import numpy as np
import pytest

import inrange_scenes as sc
import oracle

TOP = 2.0 ** 49          # what coordinate_limit promises for every operand
FAST_HI = 2.0 ** 100     # interp.hpp kFastHi
FAST_LO = 2.0 ** -100


def _source(tape):
    from codecad_amd.hip_util import _lib
    lib = _lib.load()
    p = tape.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    needed = ctypes.c_size_t(0)
    assert lib.hu_tape_source(p, tape.size, None, 0, ctypes.byref(needed)) == 0
    buf = ctypes.create_string_buffer(needed.value)
    assert lib.hu_tape_source(p, tape.size, buf, needed.value, ctypes.byref(needed)) == 0
    return buf.value.decode()


@pytest.mark.parametrize("name", [s.name for s in sc.SCENES if s.frame is not sc._none])
def test_the_scenes_are_what_this_file_says(name):
    """The float64 distance built from a scene's operands equals the oracle's float32 distance at ordinary samples: the frames,
    the half extents and the order of the transformations in inrange_scenes.py are the tape's."""
    scene = sc.BY_NAME[name]
    n = 6
    step = np.float32(scene.near * (0.75 if name.startswith("thin") else 1.75))
    corner = -step * np.float32(n / 2) + np.float32(scene.near * 0.31)
    corner = np.array([corner, corner * np.float32(0.9), corner * np.float32(1.1)], np.float32)
    if name == "box_translated":
        corner = corner + sc.FAR.astype(np.float32)
    if name == "nested":
        corner = corner + (np.array([5.0, 0.0, 0.0]) @ sc.ROT_X.T * 2.0 ** -8).astype(np.float32)
    got = oracle.grid_eval(scene.tape(), corner, step, (n, n, n))[..., 3].reshape(-1).astype(np.float64)
    want = scene.distance(sc.grid_points(corner, step, (n, n, n)))
    scale = max(float(np.max(np.abs(want))), scene.near)
    if name == "box_translated":
        scale = 2.0 ** 40          # (binary32 samples 2^40 from the origin: the shape's own frame is known to 2^17)
    assert np.max(np.abs(got - want)) <= 1e-5 * scale, (name, np.max(np.abs(got - want)), scale)


@pytest.mark.parametrize("name", [s.name for s in sc.SCENES])
def test_zero_infinity_and_the_companion_tapes(name):
    scene = sc.BY_NAME[name]
    b = sc.limit_of(name)
    if scene.expect == "zero":
        assert b == 0.0
    elif scene.expect == "inf":
        assert b == math.inf
    else:
        assert 0.0 < b < math.inf
    # the tape the device tests launch: the deferred form (the only one that reads the flag), with the same limit
    device = scene.device_tape()
    assert "deferred directions" in _source(device)
    assert sc.coordinate_limit(device) == b


def test_pins():
    box, down, up = sc.limit_of("box"), sc.limit_of("box_scaled_down"), sc.limit_of("box_scaled_up")
    # perp(|z| - 2, perp(|x| - 1, |y| - 1.5)): the rectangle's distance is bounded by 2 B + 2.5, so B = (2^49 - 2.5) / 2
    assert box == (TOP - 2.5) / 2
    assert box * 2.0 ** -20 / 2 <= down <= box * 2.0 ** -20 * 2
    assert box * 2.0 ** 20 / 2 <= up <= box * 2.0 ** 20 * 2
    assert sc.limit_of("union_of_scales") == min(down, up) == down
    # rotations can only lower it (a local coordinate reaches up to sqrt(3) B), by no more than that factor
    for name in ("box_rot_axis", "box_rot_general"):
        assert box / math.sqrt(3) * 0.999 <= sc.limit_of(name) < box
    assert sc.limit_of("box_rot_general") < sc.limit_of("box_rot_axis")
    assert sc.limit_of("box_translated") == (TOP - (2.0 ** 40 + 2.5)) / 2
    # a remainder bounds x and y, z is free: the plain small box's limit at least
    assert sc.limit_of("repetition") >= (TOP - 0.5) / 2
    # an equal bound passes: a half extent of exactly 2^-25 carries each perp_w_x of thin_ok, and the limit is the plain one
    assert sc.limit_of("thin_ok") == (TOP - (sc.H + sc.H_BELOW)) / 2 == 2.0 ** 48


def test_error_paths_of_the_accessor():
    from codecad_amd.hip_util import _lib
    lib = _lib.load()
    t = sc.BY_NAME["box"].tape()
    p = t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    out = ctypes.c_double(-7.0)
    assert lib.hu_tape_coordinate_limit(None, t.size, ctypes.byref(out)) == -3 and b"NULL" in lib.hu_last_error()
    assert lib.hu_tape_coordinate_limit(p, t.size, None) == -3 and b"NULL" in lib.hu_last_error()
    bad_source = ctypes.c_size_t(0)
    for n in (0, 3, t.size - 1):       # truncated tapes fail as they do in hu_tape_source, and write nothing
        rc = lib.hu_tape_coordinate_limit(p, n, ctypes.byref(out))
        assert rc != 0 and rc == lib.hu_tape_source(p, n, None, 0, ctypes.byref(bad_source)) and b"malformed" in lib.hu_last_error()
    assert out.value == -7.0
    assert lib.hu_tape_coordinate_limit(p, t.size, ctypes.byref(out)) == 0 and out.value == sc.limit_of("box")


@pytest.mark.parametrize("name", sc.FINITE)
def test_sound_above_and_not_vacuous(name):
    """At the corners of [-B', B']^3 (B' the largest binary32 below the limit; a coordinate of a rotated frame is largest at
    one of them) every operand of every perp_w_x is below 2^49 and every sum of squares below 2^100 -- and the largest operand
    is at least 2^45: a bound looser than 2^4 could not be told from no bound by a device test near the range's end."""
    scene = sc.BY_NAME[name]
    pts = sc.corners(sc.below32(sc.limit_of(name)))
    largest = 0.0
    for a, b in scene.operands(pts):
        assert np.max(a) < TOP and np.max(b) < TOP
        both = (a > 0) & (b > 0)
        assert np.all((a * a + b * b)[both] < FAST_HI)
        largest = max(largest, float(np.max(np.maximum(a, b))))
    print("%s: limit 2^%.3f, largest operand 2^%.3f" % (name, math.log2(sc.limit_of(name)), math.log2(largest)))
    assert largest >= 2.0 ** 45


def _ulp_steps(centre, n):
    """the 2 n + 1 binary32 numbers around centre"""
    out = [np.float32(centre)]
    for _ in range(n):
        out.insert(0, np.nextafter(out[0], np.float32(0)))
        out.append(np.nextafter(out[-1], np.float32(1)))
    return np.array(out, np.float32).astype(np.float64)


def _smallest_corner_sum(name):
    scene = sc.BY_NAME[name]
    half = {"thin_ok": sc.THIN_OK_HALF, "thin_bad": sc.THIN_BAD_HALF, "thin_worse": sc.THIN_WORSE_HALF}[name]
    ax = [_ulp_steps(h, 6) for h in half]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    smallest, n = math.inf, 0
    for a, b in scene.operands(pts):
        both = (a > 0) & (b > 0)
        n += int(both.sum())
        smallest = min(smallest, float(np.min((a * a + b * b)[both])))
    assert n > 100
    return smallest


def test_sound_below():
    """Samples stepping in binary32 ulps across the faces of the thin boxes (six either side of each face, all three axes at
    once, so every corner region is met at its tightest).  thin_ok: wherever both operands are positive the sum of squares
    stays at or above 2^-100.  thin_worse (half extents one ulp below 2^-27): a sample with a sum BELOW 2^-100 exists, which
    is why a tape with such extents and no larger one must have limit 0.

    thin_bad (one ulp below 2^-25) has limit 0 as well, but no such sample: the smallest positive |x| - h is a whole ulp of
    h, 2^-49, not the half ulp the analysis allows for, so the smallest sum is 2^-97.  The side condition h >= 2^-25 is
    conservative by a factor of four in h (2^-27 would do); recorded in DESIGN.md, nothing is wrong on the device."""
    assert _smallest_corner_sum("thin_ok") >= FAST_LO
    assert _smallest_corner_sum("thin_worse") < FAST_LO
    assert _smallest_corner_sum("thin_bad") == 2.0 ** -97
    assert sc.limit_of("thin_bad") == 0.0 and sc.limit_of("thin_worse") == 0.0


def _exact32(points):
    return np.array_equal(points, points.astype(np.float32).astype(np.float64))


def _twin_leaves_the_fast_range(scene, points):
    for a, b in scene.operands(points):
        both = (a > 0) & (b > 0)
        if np.any((a * a + b * b)[both] >= FAST_HI):
            return True
    return False


@pytest.mark.parametrize("name", sc.FINITE)
def test_the_device_grids_bite(name):
    """The grids of test_gpu_inrange_flag.py lie where they claim: below the limit by grid_reach's own rule (the flag is set),
    at the limit within four binary32 ulps, every coordinate an exact binary32; the twin's reach is beyond the limit and at
    least one of its samples has both operands positive and a sum of squares of 2^100 or more (the IEEE branch is taken)."""
    scene, b = sc.BY_NAME[name], sc.limit_of(name)
    for dims in ((16, 16, 32), (13, 10, 9)):
        corner, step, dims = sc.far_grid(name, dims)
        pts = sc.grid_points(corner, step, dims)
        assert _exact32(pts) and _exact32(np.asarray(corner))
        reach = sc.grid_reach(corner, step, dims)
        assert reach < b and b - reach <= 2 * float(step)
        assert float(np.max(np.abs(pts))) >= b - 3 * float(step)
        if name in sc.LATTICE_BOUND:
            # (x and y stay small and off the repetition's lattice: the extrusion's corner is live below the limit, flag set)
            live = sc.in_corner_region(scene, pts)[-1]
            a, bb = scene.operands(pts)[-1]
            assert live.sum() >= 100 and np.all((a * a + bb * bb)[live] < FAST_HI) and np.max(a[live]) >= 2.0 ** 45
        corner, step, dims = sc.far_grid(name, dims, above=True)
        pts = sc.grid_points(corner, step, dims)
        assert _exact32(pts)
        assert sc.grid_reach(corner, step, dims) >= b
        assert _twin_leaves_the_fast_range(scene, pts), name
    corner, step, dims = sc.origin_grid(name)
    pts = sc.grid_points(corner, step, dims)
    assert _exact32(pts) and np.any(np.all(pts == 0.0, axis=1))
    assert b / 4 <= sc.grid_reach(corner, step, dims) < b
    # the slab cases: planes 8.. of the grid lie at or beyond the limit, the rest below; the whole grid's reach is beyond
    corner, step, dims = sc.crossing_x(name, 8)
    x = sc.grid_points(corner, step, dims).reshape(dims + (3,))[:, 0, 0, 0]
    assert np.all(x[:8] < b) and np.all(x[8:] >= b) and sc.grid_reach(corner, step, dims) >= b
    pts = sc.grid_points(corner, step, dims)
    assert _exact32(pts) and np.max(pts[:, 1:]) < b


def test_list_launches_at_the_limit_keep_the_range_test():
    """A launch over a device list knows its corners only as 32-bit integers times the resolution (list_reach counts 2^31
    resolutions): with samples within a few ulps of B the resolution is at least one binary32 ulp of B, and 2^31 of those
    alone are far beyond B, whatever the origin.  So the block and level launches of the device tests at the limit all run
    WITH the range test, whichever side their samples are on; what they check is that the reach errs on that side."""
    for name in sc.FINITE:
        b = sc.limit_of(name)
        ulp = sc.quantum(b) / 4
        assert 2147483648.0 * ulp >= b
        assert sc.list_reach(ulp, (0.0, 0.0, 0.0), 0.0) >= b
