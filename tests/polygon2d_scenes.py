"""Synthetic float4 corner fields for the 2D contouring kernel (reference rendering/polygon2d.cl), shared by
tests/test_polygon2d_reference_host.py (oracle against the executed reference) and
tests/test_gpu_polygon2d_fields.py (HIP kernel against the oracle and the recorded reference).

A scene is (name, corners float32 (gx, gy, 4), box_corner (x, y), box_step); every field is a pure function of
its seed, so the fixture tests/golden/polygon2d_ref.npz stores outputs only.  Also here: a NumPy restatement of
place_vertex in a chosen precision, which tells threshold cells apart, and the hand-made cells that sit on the
two break constants."""
import collections
import os

import numpy as np

Scene = collections.namedtuple("Scene", "name corners corner step")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polygon2d_ref.npz")
EMPTY = 0xffffffff
PLACEMENTS = (("unit", (0.0, 0.0), 1.0), ("offset", (-3.03, 2.97), 0.37))
NOISE_GRIDS = ((2, 2), (2, 3), (3, 2), (2, 130), (130, 2), (9, 9), (17, 33), (65, 66), (67, 67))
# the two largest noise grids are executed where oracle/_ref is built and left out of the fixture (its size limit)
NOT_IN_FIXTURE = ((65, 66), (67, 67))
# seeds for which at most 2 % of a scene's non-empty cells come near a break threshold (checked on the reference
# alone by test_polygon2d_reference_host.py::test_few_cells_of_a_scene_sit_near_a_threshold)
NOISE_SEEDS = {(2, 2): 1, (2, 3): 1, (3, 2): 1, (2, 130): 1, (130, 2): 1, (9, 9): 1, (17, 33): 1, (65, 66): 1, (67, 67): 1}
EDGE_GRID = (19, 14)


def noise_field(grid, seed):
    """Unit normals at random angles, w uniform in +-1."""
    rng = np.random.default_rng([seed, grid[0], grid[1]])
    angle = rng.uniform(0.0, 2.0 * np.pi, grid)
    c = np.zeros(grid + (4,), dtype=np.float32)
    c[..., 0], c[..., 1] = np.cos(angle), np.sin(angle)
    c[..., 3] = rng.uniform(-1.0, 1.0, grid)
    return c


def boundary_ring(gx, gy):
    """The boundary samples of a (gx, gy) corner grid in order round the block, each once."""
    ring = [(x, 0) for x in range(gx)] + [(gx - 1, y) for y in range(1, gy)]
    ring += [(x, gy - 1) for x in range(gx - 2, -1, -1)] + [(0, y) for y in range(gy - 2, 0, -1)]
    assert len(ring) == 2 * ((gx - 1) + (gy - 1))
    return ring


def edge_fields():
    """name -> corner field; the edges of the kernel's comparisons and of the starts list."""
    g = EDGE_GRID
    out = {}
    rng = np.random.default_rng(77)
    c = noise_field(g, 11)
    pick = rng.uniform(size=g)
    c[..., 3][pick < 0.25] = 0.0     # w <= 0: an exact zero is inside
    c[..., 3][pick > 0.85] = -0.0
    out["zeros"] = c
    c = noise_field(g, 12)
    pick = rng.uniform(size=g)
    c[..., 3][pick < 0.15] = np.nan  # NaN <= 0 is false: outside
    c[..., 3][(pick > 0.4) & (pick < 0.5)] = np.inf
    c[..., 3][pick > 0.9] = -np.inf
    out["nonfinite"] = c
    c = noise_field(g, 13)
    c[..., :2] = 0.0                 # gradientLengthSquared = 0 < 1e-8: the vertex stays at the weighted average
    out["zero_normals"] = c
    c = noise_field(g, 14)
    c[..., :2] *= rng.uniform(0.1, 3.0, g + (1,)).astype(np.float32)
    out["nonunit_normals"] = c
    for name, grid in (("alternating", g), ("alternating_2x2", (2, 2)), ("alternating_2x9", (2, 9))):
        c = noise_field(grid, 15)
        for i, (x, y) in enumerate(boundary_ring(*grid)):
            c[x, y, 3] = abs(c[x, y, 3]) * (1 if i % 2 else -1) + (0.01 if i % 2 else -0.01)
        out[name] = c
    c = noise_field(g, 16)
    c[..., 3] = np.abs(c[..., 3]) + 0.05
    for x, y in ((0, 0), (0, g[1] - 1), (g[0] - 1, 0), (g[0] - 1, g[1] - 1),
                 (g[0] // 2, 0), (g[0] // 2, g[1] - 1), (0, g[1] // 2), (g[0] - 1, g[1] // 2)):
        c[x, y, 3] = -c[x, y, 3]
    out["corners_and_sides"] = c
    return out


def scenes():
    out = []
    for pname, corner, step in PLACEMENTS:
        for grid in NOISE_GRIDS:
            out.append(Scene("noise_%dx%d_%s" % (grid + (pname,)), noise_field(grid, NOISE_SEEDS[grid]), corner, np.float32(step)))
        for name, c in edge_fields().items():
            out.append(Scene("%s_%s" % (name, pname), c, corner, np.float32(step)))
    return out


def fixture_scenes():
    skip = tuple("noise_%dx%d_" % g for g in NOT_IN_FIXTURE)
    return [s for s in scenes() if not s.name.startswith(skip)]


def load_fixture():
    with np.load(FIXTURE) as f:
        return {name: f[name] for name in f.files}


def recorded(fixture, name):
    """(vertices, links, starts in launch order) as the executed reference gave them."""
    return fixture[name + "/v"].view(np.float32), fixture[name + "/l"], fixture[name + "/s"]


def cell_types(corners):
    """cellType of polygon2d.cl:94-101 per half cell -> uint array (gx-1, gy-1, 2)."""
    inside = (corners[..., 3] <= 0).astype(np.uint32)
    a, b = inside[:-1, :-1], inside[1:, 1:]
    third = np.stack([inside[:-1, 1:], inside[1:, :-1]], -1)   # offsets (t, 1-t): t=0 -> (0,1), t=1 -> (1,0)
    return (a[..., None] << 2) | (b[..., None] << 1) | third


def cell_inputs(scene, dtype):
    """Corner positions (cells, 3, 2) in binary32 as the kernel forms them, and values (cells, 3, 4), as `dtype`."""
    c = scene.corners
    gx, gy = c.shape[:2]
    x, y, t = np.meshgrid(np.arange(gx - 1), np.arange(gy - 1), np.arange(2), indexing="ij")
    x, y, t = x.reshape(-1), y.reshape(-1), t.reshape(-1)   # cell index t + 2*(y + (gy-1)*x)
    ox = np.stack([np.zeros_like(t), np.ones_like(t), t], -1)
    oy = np.stack([np.zeros_like(t), np.ones_like(t), 1 - t], -1)
    px, py = x[:, None] + ox, y[:, None] + oy
    corner = np.asarray(scene.corner, dtype=np.float64).astype(np.float32)
    pos = np.stack([corner[0] + px.astype(np.float32) * np.float32(scene.step),
                    corner[1] + py.astype(np.float32) * np.float32(scene.step)], -1)
    return pos.astype(dtype), c[px, py].astype(dtype)


def place_vertex(pos, val, dtype, rel=1e-4):
    """place_vertex (polygon2d.cl:38-80) over all cells at once, in `dtype`, in the kernel's operation order.
    -> (vertices (cells, 2), near (cells,): residualSum or gradientLengthSquared came within a relative `rel` of
    its threshold in some iteration the cell reached, residual (cells, 8), g2 (cells, 8); NaN where not reached)."""
    one = dtype(1)
    n = len(pos)
    with np.errstate(all="ignore"):
        ax = np.zeros(n, dtype)
        ay = np.zeros(n, dtype)
        weight = np.zeros(n, dtype)
        for i in range(3):
            w = one / (one + np.abs(val[:, i, 3]))
            ax = ax + pos[:, i, 0] * w
            ay = ay + pos[:, i, 1] * w
            weight = weight + w
        px, py = ax / weight, ay / weight
        active = np.ones(n, bool)
        near = np.zeros(n, bool)
        res_log = np.full((n, 8), np.nan)
        g2_log = np.full((n, 8), np.nan)
        for it in range(8):
            gx = np.zeros(n, dtype)
            gy = np.zeros(n, dtype)
            residual = np.zeros(n, dtype)
            for j in range(3):
                nx, ny = val[:, j, 0], val[:, j, 1]
                tmp = (nx * (px - pos[:, j, 0]) + ny * (py - pos[:, j, 1])) + val[:, j, 3]
                residual = residual + tmp * tmp
                gx = gx + nx * tmp
                gy = gy + ny * tmp
            res_log[active, it] = residual[active]
            near |= active & (np.abs(residual.astype(np.float64) - 1e-3) <= rel * 1e-3)
            active = active & ~(residual.astype(np.float64) < 1e-3)    # the literals are doubles in OpenCL C
            g2 = gx * gx + gy * gy
            g2_log[active, it] = g2[active]
            near |= active & (np.abs(g2.astype(np.float64) - 1e-8) <= rel * 1e-8)
            active = active & ~(g2.astype(np.float64) < 1e-8)
            k = residual / g2
            px = np.where(active, px - gx * k, px)
            py = np.where(active, py - gy * k, py)
    return np.stack([px, py], -1), near, res_log, g2_log


# Hand-made 2x2 fields (placement: corner (0, 0), step 1) whose half cell 0 lands exactly on a break constant in
# its first iteration, found by scanning consecutive floats of one w: (name, corner field as uint32 bits (2, 2, 4),
# which quantity, the binary32 value it takes).  Binary32 1e-3f = 0x3a83126f lies ABOVE the double 1e-3 and 1e-8f =
# 0x322bcc77 BELOW the double 1e-8, so `x < 1e-3` decides alike for every binary32 x whichever type the literal
# has, while `x < 1e-8` is true and `x < 1e-8f` false for exactly one input, x = 1e-8f.
ON_CONSTANT = (
    ("residual_at_1e-3f", "residual", 0x3a83126f,
     (0x3cf5c28f, 0x00000000, 0x00000000, 0xbcfde752, 0x3cf5c28f, 0x00000000, 0x00000000, 0xbcdd2f1b,
      0x00000000, 0x3f800000, 0x00000000, 0x3f800000, 0x3cf5c28f, 0x00000000, 0x00000000, 0x3b449ba6)),
    ("residual_below_1e-3f", "residual", 0x3a83126e,
     (0x3cf5c28f, 0x00000000, 0x00000000, 0xbcfdf808, 0x3cf5c28f, 0x00000000, 0x00000000, 0xbcdd2f1b,
      0x00000000, 0x3f800000, 0x00000000, 0x3f800000, 0x3cf5c28f, 0x00000000, 0x00000000, 0x3b45436c)),
    ("gradient_at_1e-8f", "gradient", 0x322bcc77,
     (0x3a03126f, 0x00000000, 0x00000000, 0x3dbc0074, 0x00000000, 0x00000000, 0x00000000, 0xbdcccccd,
      0x00000000, 0x3f800000, 0x00000000, 0x3f800000, 0x3c23d70a, 0x3b070111, 0x00000000, 0x3c4ccccd)),
    ("gradient_above_1e-8f", "gradient", 0x322bcc78,
     (0x3a03126f, 0x00000000, 0x00000000, 0x3da3876f, 0x00000000, 0x00000000, 0x00000000, 0xbdcccccd,
      0x00000000, 0x3f800000, 0x00000000, 0x3f800000, 0x3c23d70a, 0x00000000, 0x00000000, 0x3c4ccccd)),
    ("gradient_below_1e-8f", "gradient", 0x322bcc76,
     (0x3a03126f, 0x00000000, 0x00000000, 0x3da3876d, 0x00000000, 0x00000000, 0x00000000, 0xbdcccccd,
      0x00000000, 0x3f800000, 0x00000000, 0x3f800000, 0x3c23d70a, 0x00000000, 0x00000000, 0x3c4ccccd)),
)


def on_constant_scenes():
    return [Scene("on_" + name, np.array(bits, dtype=np.uint32).view(np.float32).reshape(2, 2, 4), (0.0, 0.0), np.float32(1.0))
            for name, _which, _value, bits in ON_CONSTANT]
