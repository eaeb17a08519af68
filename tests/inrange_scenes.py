"""Scenes and grids for the tests of the fast square root's in-range flag (test_inrange_flag_host.py, test_gpu_inrange_flag.py).

Per-tape code takes the square root of every rectangle and extrusion corner (`perp_w_x`) without its range test when the
launch's largest |sample coordinate| is below the tape's coordinate limit B (csrc/specialise.hpp coordinate_limit,
hu_tape_coordinate_limit).  Every scene here is simple enough that a few lines of NumPy float64 give the operands of each
`perp_w_x` of its tape at a world sample, from the shape's definition alone: `operands(points)` -> [(a, b), ...], one pair of
arrays per statement, and `distance(points)`, which the host tests hold against the oracle so that a wrong frame convention
in this file cannot go unnoticed.

Only the deferred form of per-tape code reads the flag, and a tape of ONE primitive is built in the plain form.  `device_shape`
therefore intersects a scene with a half space 2^100 away: the tape then has two primitives, the half space never wins the
maximum, has no square root, and leaves the limit where it was (the host tests pin that too).
"""
import ctypes
import math

import numpy as np

H = 2.0 ** -25                                       # the smallest half extent the analysis accepts
H_BELOW = float(np.nextafter(np.float32(H), np.float32(0)))
Q_BELOW = float(np.nextafter(np.float32(2.0 ** -27), np.float32(0)))


def perp(a, b):
    """interp.hpp perp_w: the distance to a corner region where both slab distances are positive, else the larger"""
    return np.where((a > 0) & (b > 0), np.hypot(a, b), np.maximum(a, b))


def rotation(axis, degrees):
    """Rodrigues: the matrix that turns a vector by `degrees` about `axis` (right-handed)"""
    k = np.array(axis, np.float64)
    k = k / np.linalg.norm(k)
    t = math.radians(degrees)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * kx + (1 - math.cos(t)) * (kx @ kx)


def _box(local, half):
    """a box in its own frame: the rectangle's corner, then the extrusion's -> (operand pairs, distance)"""
    ax, ay, az = (np.abs(local[:, c]) - half[c] for c in range(3))
    rect = perp(ax, ay)
    return [(ax, ay), (az, rect)], perp(az, rect)


class Scene:
    def __init__(self, name, build, frame, expect, near=1.0):
        self.name, self.build, self.frame, self.expect, self.near = name, build, frame, expect, near

    def shape(self):
        return self.build()

    def tape(self):
        from codecad_amd import nodes
        return np.ascontiguousarray(nodes.make_program(self.shape()), np.float32)

    def device_shape(self):
        import codecad_amd as cc
        return self.shape() & cc.shapes.half_space().translated(0, -2.0 ** 100, 0)

    def device_tape(self):
        from codecad_amd import nodes
        return np.ascontiguousarray(nodes.make_program(self.device_shape()), np.float32)

    def operands(self, points):
        return self.frame(np.asarray(points, np.float64).reshape(-1, 3))[0]

    def distance(self, points):
        return self.frame(np.asarray(points, np.float64).reshape(-1, 3))[1]


def _s():
    import codecad_amd as cc
    return cc.shapes


def _base():
    return _s().box(2, 3, 4)


BASE_HALF = (1.0, 1.5, 2.0)
ROT_Z = rotation((0, 0, 1), 30)
ROT_G = rotation((1, 2, 3), 40)
ROT_X = rotation((1, 0, 0), 90)
FAR = np.array([2.0 ** 40, 0.0, -2.0 ** 39])


def _scaled(s):
    def frame(p):
        ops, d = _box(p / s, BASE_HALF)
        return ops, d * s
    return frame


def _nested(p):
    # world = 2^-8 Rx(90) (2^-10 local + (5, 0, 0))
    local = ((p * 2.0 ** 8) @ ROT_X - np.array([5.0, 0.0, 0.0])) * 2.0 ** 10
    ops, d = _box(local, BASE_HALF)
    return ops, d * 2.0 ** -18


def _cyl(p):
    slab, circle = np.abs(p[:, 2]) - 1.5, np.hypot(p[:, 0], p[:, 1]) - 1.0
    return [(slab, circle)], perp(slab, circle)


def _revolved(p):
    a, b = np.abs(np.hypot(p[:, 0], p[:, 2]) - 3.0) - 0.5, np.abs(p[:, 1]) - 1.0
    return [(a, b)], perp(a, b)


def _offset_shell(p):
    ops, d = _box(p, (1.0, 1.0, 1.0))
    return ops, np.abs(d - 0.5) - 0.1           # (a shell of wall thickness t lies t / 2 either side of the surface)


def _mirror_symm(p):
    local = np.stack([np.abs(p[:, 0]) - 2.0, -p[:, 1], p[:, 2]], axis=1)
    return _box(local, (0.5, 1.0, 1.5))


def _repetition(p):
    r = p.copy()
    r[:, :2] = p[:, :2] - 2.0 * np.rint(p[:, :2] / 2.0)     # the IEEE remainder (ties to even), exact here
    return _box(r, (0.25, 0.25, 0.25))


def _union_of_scales(p):
    a, da = _scaled(2.0 ** -20)(p)
    b, db = _scaled(2.0 ** 20)(p)
    return a + b, np.minimum(da, db)


def _thin(half):
    return lambda p: _box(p, half)


def _none(p):
    return [], np.full(len(p), np.nan)


THIN_OK_HALF = (H, H_BELOW, H)           # every perp_w_x of the tape leans on a half extent of exactly 2^-25
THIN_BAD_HALF = (H_BELOW, H_BELOW, H_BELOW)
THIN_WORSE_HALF = (Q_BELOW, Q_BELOW, Q_BELOW)


def _thin_box(half):
    return lambda: _s().box(2 * half[0], 2 * half[1], 2 * half[2])


def _gear():
    from codecad_amd.shapes import gears
    return gears.InvoluteGear(20, 0.5).extruded(1)


SCENES = [
    Scene("box", _base, _scaled(1.0), "finite"),
    Scene("box_scaled_down", lambda: _base().scaled(2.0 ** -20), _scaled(2.0 ** -20), "finite", near=2.0 ** -20),
    Scene("box_scaled_up", lambda: _base().scaled(2.0 ** 20), _scaled(2.0 ** 20), "finite", near=2.0 ** 20),
    Scene("box_rot_axis", lambda: _base().rotated_z(30), lambda p: _box(p @ ROT_Z, BASE_HALF), "finite"),
    Scene("box_rot_general", lambda: _base().rotated((1, 2, 3), 40), lambda p: _box(p @ ROT_G, BASE_HALF), "finite"),
    Scene("box_translated", lambda: _base().translated(2.0 ** 40, 0, -2.0 ** 39), lambda p: _box(p - FAR, BASE_HALF), "finite"),
    Scene("nested", lambda: _base().scaled(2.0 ** -10).translated(5, 0, 0).rotated_x(90).scaled(2.0 ** -8), _nested, "finite",
          near=2.0 ** -6),
    Scene("cyl", lambda: _s().cylinder(h=3, d=2), _cyl, "finite"),
    Scene("rect_revolved", lambda: _s().rectangle(1, 2).translated_x(3).revolved(), _revolved, "finite"),
    Scene("offset_shell", lambda: _s().box(2).offset(0.5).shell(0.2), _offset_shell, "finite"),
    Scene("mirror_symm", lambda: _s().box(1, 2, 3).translated_x(2).symmetrical_x().mirrored_y(), _mirror_symm, "finite"),
    Scene("repetition", lambda: _s().unsafe.Repetition(_s().box(0.5), (2, 2, None)), _repetition, "finite"),
    Scene("union_of_scales", lambda: _base().scaled(2.0 ** -20) | _base().scaled(2.0 ** 20), _union_of_scales, "finite"),
    Scene("thin_ok", _thin_box(THIN_OK_HALF), _thin(THIN_OK_HALF), "finite", near=H),
    Scene("thin_bad", _thin_box(THIN_BAD_HALF), _thin(THIN_BAD_HALF), "zero", near=H),
    Scene("thin_worse", _thin_box(THIN_WORSE_HALF), _thin(THIN_WORSE_HALF), "zero", near=H / 4),
    Scene("outside_analysis_polygon", lambda: _s().polygon2d([(0, 0), (4, 6), (4, -2), (-4, -2), (-4, 6)]).extruded(1), _none, "zero"),
    Scene("outside_analysis_gear", _gear, _none, "zero"),
    Scene("no_perp_sphere", lambda: _s().sphere(3), _none, "inf"),
    Scene("no_perp_half_sphere", lambda: _s().half_space() & _s().sphere(3), _none, "inf"),
]
BY_NAME = {s.name: s for s in SCENES}
FINITE = [s.name for s in SCENES if s.expect == "finite"]


def coordinate_limit(tape):
    """hu_tape_coordinate_limit of raw tape floats (host only)"""
    from codecad_amd.hip_util import _lib
    lib = _lib.load()
    t = np.ascontiguousarray(tape, np.float32)
    out = ctypes.c_double(-1.0)
    rc = lib.hu_tape_coordinate_limit(t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), t.size, ctypes.byref(out))
    assert rc == 0, lib.hu_last_error()
    return out.value


_limits = {}


def limit_of(name):
    if name not in _limits:
        _limits[name] = coordinate_limit(BY_NAME[name].tape())
    return _limits[name]


# ---- samples and grids at the limit ---------------------------------------------------------------------------------
def below32(b):
    """the largest binary32 number below b"""
    f = np.float32(b)
    return float(f) if float(f) < b else float(np.nextafter(f, np.float32(0)))


def corners(b):
    """the eight corners of [-b, b]^3: a linear form of the coordinates is largest at one of them, whatever its signs"""
    return np.array([[sx * b, sy * b, sz * b] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


def largest_operand(scene, points):
    return np.max([np.maximum(a, b) for a, b in scene.operands(points)], axis=0)


def worst_octant(name):
    """the signs of the corner of [-B, B]^3 at which the scene's largest operand is largest"""
    c = corners(below32(limit_of(name)))
    return np.sign(c[int(np.argmax(largest_operand(BY_NAME[name], c)))])


def quantum(b):
    """the step of the grids at the limit: four binary32 ulps of the numbers just below b (a power of two)"""
    return 2.0 ** (math.floor(math.log2(below32(b))) - 21)


def grid_reach(corner, step, dims):
    """csrc/hip_util.hip grid_reach: the larger of |corner| and |corner + step * n| over the axes, in fp64"""
    c = np.array(np.asarray(corner, np.float32), np.float64)
    return float(np.max(np.maximum(np.abs(c), np.abs(c + float(np.float32(step)) * np.array(dims, np.float64)))))


def list_reach(resolution, origin, extent):
    """csrc/hip_util.hip list_reach: any 32-bit integer corner times the resolution, plus the origin, plus the block"""
    return 2147483648.0 * abs(resolution) + max(abs(o) for o in origin) + abs(extent)


# Scenes in which a repetition bounds x and y: their grids at the limit keep x and y small and OFF the repetition's lattice
# (a sample at 0.3125 lies outside the bars' cross-section, so the extrusion's corner is live) and only z goes out to B.  In
# binary32 only the first sample of such an axis is off the lattice: 0.3125 + k * step rounds to k * step for k >= 1.
LATTICE_BOUND = {"repetition": 0.3125}


def far_grid(name, dims, above=False):
    """(corner, step, dims) of a grid in the scene's worst octant whose outermost samples are the last grid points for which
    grid_reach stays below the limit B -- every coordinate a multiple of the step, so an exact binary32 number; `above`: its
    twin, the same grid moved out by three times that distance along every axis (to about 4 B: sums of squares beyond 2^100).
    LATTICE_BOUND scenes: x and y start at the small offset instead, and the twin lies at 8 B with twice the step (z alone
    has to carry the sum past 2^100, and 4 B' is still below 2^50)."""
    b = limit_of(name)
    q = quantum(b)
    top = (math.ceil(b / q) - 2) * q             # top + q < b: grid_reach counts one step past the last sample
    small = LATTICE_BOUND.get(name)
    if above:
        top, q = (8 * top, 2 * q) if small is not None else (4 * top, q)
    sign = worst_octant(name)
    corner = np.where(sign > 0, top - q * (np.array(dims) - 1), -top).astype(np.float64)
    if small is not None:
        corner[:2] = small
    return corner, np.float32(q), tuple(dims)


def in_corner_region(scene, points):
    """per perp_w_x of the scene: the samples at which both operands are positive (its square root is taken there)"""
    return [(a > 0) & (b > 0) for a, b in scene.operands(points)]


def grid_points(corner, step, dims):
    """the samples of a grid as the kernels compute them: corner + step * index in binary32 (exact for the grids here)"""
    c = np.asarray(corner, np.float32)
    ax = [(c[k] + np.float32(step) * np.arange(dims[k], dtype=np.float32)).astype(np.float32) for k in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return g.astype(np.float64)


def origin_grid(name, dims=(16, 16, 32)):
    """a grid through exact zeros at the limit's scale: step = P / 32 with P the largest power of two <= B; x and y run
    over [-P/4, P/4), z over [-P/2, P/2) -- not quite the [-B/2, B/2] one might want: the step has to be a power of two, a
    grid has one step for its three axes and 16 x 16 x 32 samples, and grid_reach has to stay below B with z the longest axis"""
    p = 2.0 ** math.floor(math.log2(limit_of(name)))
    step = p / 32
    return np.array([-8 * step, -8 * step, -16 * step]), np.float32(step), tuple(dims)


def crossing_x(name, first_beyond):
    """a 16 x 16 x 32 grid at the limit whose planes x >= first_beyond lie at or beyond B; y and z stay below it"""
    b = limit_of(name)
    q = quantum(b)
    m = math.ceil(b / q)                        # m * q >= b > (m - 1) * q
    corner = np.array([(m - first_beyond) * q, (m - 40) * q, (m - 60) * q])
    return corner, np.float32(q), (16, 16, 32)
