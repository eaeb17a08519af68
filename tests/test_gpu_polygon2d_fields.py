"""The HIP contouring kernel (k_process_polygon behind hu_process_polygon and hu_process_polygon_blocks) on
synthetic corner fields, uploaded directly: the scenes of tests/polygon2d_scenes.py, grids at the 512 limit of the
link encoding, batches of blocks with far-away integer corners, and the argument checks.  Exact against
oracle.process_polygon, and against the executed reference as recorded in tests/golden/polygon2d_ref.npz
(differing vertex cells against the recording: 0 in every scene, asserted)."""
import ctypes

import numpy as np
import pytest

import oracle
import polygon2d_scenes as ps

pytestmark = pytest.mark.gpu

SCENES = {s.name: s for s in ps.scenes() + ps.on_constant_scenes()}
RECORDED = {s.name for s in ps.fixture_scenes() + ps.on_constant_scenes()}
LARGE = {"noise_512x2": (512, 2), "noise_2x512": (2, 512), "noise_512x3": (512, 3), "noise_512x512": (512, 512)}
SENTINEL = 0xa5a5a5a5
HU_ERR_BAD_ARG = -3


@pytest.fixture(scope="module")
def fixture():
    return ps.load_fixture()


def upload(hip_util, array, dtype=np.float32):
    a = np.ascontiguousarray(array, dtype=dtype)
    buf = hip_util.Buffer(dtype, a.shape)
    buf.enqueue_write(a)
    return buf


def single_block(hip, corners, corner, step):
    """hu_process_polygon on one uploaded field -> (vertex bits (cells, 2), links, starts as written, counter,
    the words behind the starts list's capacity)."""
    from codecad_amd import hip_util
    gx, gy = corners.shape[:2]
    cells, cap = (gx - 1) * (gy - 1) * 2, (gx - 1) + (gy - 1)
    c = upload(hip_util, corners)
    vertices = hip_util.Buffer(np.uint32, (cells, 2))
    links = hip_util.Buffer(np.uint32, cells)
    starts = hip_util.Buffer(np.uint32, cap + 8)
    counter = hip_util.Buffer(np.uint32, 1)
    vertices.enqueue_fill(0xff)
    starts.enqueue_fill(0xa5)
    counter.enqueue_fill(0)
    ev = hip.k.process_polygon((gx - 1, gy - 1, 2), None, np.asarray(corner, np.float64).astype(np.float32), step, c, vertices,
                               links, starts, counter)
    out = (vertices.read(wait_for=[ev]).copy(), links.read().copy(), starts.read().copy(), int(counter.read()[0]))
    for b in (c, vertices, links, starts, counter):
        b.release()
    return out[0], out[1], out[2][:cap], out[3], out[2][cap:]


def check_against(got, want, scene_step=None):
    """got: single_block's tuple; want: (vertices float32, links, starts) of the oracle or the reference."""
    v, l, s, n, tail = got
    wv, wl, ws = want
    assert np.array_equal(l, wl)
    live = wl != ps.EMPTY
    assert live.any()
    wbits = wv.view(np.uint32)
    same = (v == wbits) | (np.isnan(v.view(np.float32)) & np.isnan(wv))
    assert np.count_nonzero(~same[live]) == 0
    assert np.all(v[~live] == 0xffffffff)    # empty cells are not written
    assert n == len(ws)
    assert np.array_equal(np.sort(s[:n]), np.sort(ws))
    assert np.all(s[n:] == SENTINEL) and np.all(tail == SENTINEL)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_single_block_matches_the_oracle_and_the_recorded_reference(hip, fixture, name):
    s = SCENES[name]
    got = single_block(hip, s.corners, s.corner, s.step)
    check_against(got, oracle.process_polygon(s.corners, s.corner, s.step))
    gx, gy = s.corners.shape[:2]
    if name.startswith("alternating"):
        assert got[3] == (gx - 1) + (gy - 1)    # the starts list is full, and nothing behind it was touched
    if name in RECORDED:
        # bit for bit, so the rule for threshold cells (test_polygon2d_reference_host.differing_cells) excuses nothing
        check_against(got, ps.recorded(fixture, name))


def limit_field(grid):
    """Noise with a sign change between the last two samples of every 512-long border: a chain enters and another
    leaves at row 510, the top of the overflow field."""
    c = ps.noise_field(grid, 21)
    w = c[..., 3]
    if grid[0] == 512:
        for y in (0, grid[1] - 1):
            w[510, y], w[511, y] = abs(w[510, y]) + 0.01, -abs(w[511, y]) - 0.01
    if grid[1] == 512:
        for x in (0, grid[0] - 1):
            w[x, 510], w[x, 511] = abs(w[x, 510]) + 0.01, -abs(w[x, 511]) - 0.01
    return c


@pytest.mark.parametrize("name", sorted(LARGE))
def test_single_block_at_the_limit_of_the_link_encoding(hip, name):
    """512 corner samples a side: 522 242 half cells, the largest index the link encoding is asked to hold, and
    row 510, the top of the overflow field, in links and in starts."""
    grid = LARGE[name]
    corners = limit_field(grid)
    corner, step = (-3.03, 2.97), np.float32(0.37)
    got = single_block(hip, corners, corner, step)
    want = oracle.process_polygon(corners, corner, step)
    check_against(got, want)
    for axis, flag in ((0, 0xc0000000), (1, 0x80000000)):   # 512 samples along x: the row of a y border is x
        if grid[axis] == 512:
            for words in (want[1][want[1] != ps.EMPTY], want[2]):
                assert ((words[words & 0xc0000000 == flag] >> 20) & 0x1ff).max() == 510
    if grid == (512, 512):
        inner = want[1][(want[1] & 0x80000000) == 0]
        assert len(want[1]) == 522242 and inner.max() > 522242 - 4 * 511   # links into the last column of cells


def run_blocks(hip, fields, int_corners, resolution, origin, step, prefill_starts=True):
    """hu_process_polygon_blocks over len(fields) blocks of equal dims -> per-block arrays (vertex bits, links,
    starts rows with the sentinel where nothing was written, counters)."""
    from codecad_amd import hip_util
    n = len(fields)
    gx, gy = fields[0].shape[:2]
    cells, cap = (gx - 1) * (gy - 1) * 2, (gx - 1) + (gy - 1)
    c = upload(hip_util, np.stack(fields))
    blocks = np.zeros((n, 4), np.int32)
    blocks[:, :2] = int_corners
    blocks[:, 3] = 1
    b = upload(hip_util, blocks, np.int32)
    vertices = hip_util.Buffer(np.uint32, (n, cells, 2))
    links = hip_util.Buffer(np.uint32, (n, cells))
    starts = hip_util.Buffer(np.uint32, (n + 1, cap))   # one row more: nothing may be written behind the last block
    counters = hip_util.Buffer(np.uint32, n)
    vertices.enqueue_fill(0xff)
    starts.enqueue_fill(0xa5)
    counters.enqueue_fill(0)
    d = (ctypes.c_uint32 * 2)(gx, gy)
    o = (ctypes.c_double * 3)(origin[0], origin[1], 0.0)
    rc = hip.lib.hu_process_polygon_blocks(c.device_ptr, b.device_ptr, n, float(resolution), o, np.float32(step), d,
                                           vertices.device_ptr, links.device_ptr, starts.device_ptr, counters.device_ptr,
                                           hip.queue.handle)
    assert rc == 0, hip.lib.hu_last_error()
    hip.queue.synchronize()
    out = vertices.read().copy(), links.read().copy(), starts.read().copy(), counters.read().copy()
    for buf in (c, b, vertices, links, starts, counters):
        buf.release()
    return out


RES, ORIGIN = 0.37, (0.123, -4.56)


def block_corner(ic):
    return (np.float32(np.float64(ic[0]) * RES + ORIGIN[0]), np.float32(np.float64(ic[1]) * RES + ORIGIN[1]))


@pytest.mark.parametrize("n", [1, 3, 300])
def test_batches_of_blocks_match_the_oracle_block_by_block(hip, n):
    """Different noise fields per block, integer corners up to +-2^20; every block against the oracle at the float
    corner (float)(int_corner * resolution + origin), the first and the last also against the single-block call."""
    grid = (9, 7)
    cap = (grid[0] - 1) + (grid[1] - 1)
    rng = np.random.default_rng(n)
    fields = [ps.noise_field(grid, 100 + i) for i in range(n)]
    ics = rng.integers(-(1 << 20), (1 << 20) + 1, (n, 2))
    ics[0] = (-(1 << 20), 1 << 20)
    ics[-1] = ((1 << 20), -(1 << 20)) if n > 1 else ics[-1]
    step = np.float32(RES)
    v, l, s, c = run_blocks(hip, fields, ics, RES, ORIGIN, step)
    for i in range(n):
        want = oracle.process_polygon(fields[i], block_corner(ics[i]), step)
        check_against((v[i], l[i], s[i], int(c[i]), s[i][:0]), want)
    assert np.all(s[n] == SENTINEL)
    for i in {0, n - 1}:
        sv, sl, ss, sn, _ = single_block(hip, fields[i], block_corner(ics[i]), step)
        assert np.array_equal(sv, v[i]) and np.array_equal(sl, l[i])
        assert sn == int(c[i]) and np.array_equal(np.sort(ss[:sn]), np.sort(s[i][:sn]))
    assert cap >= int(c.max())


def test_an_empty_block_and_a_full_starts_list_keep_to_their_own_rows(hip):
    """Block 1 is empty: its counter stays zero and its starts row untouched.  Block 3's boundary alternates in
    sign all the way round: its starts row is full and the rows of blocks 2 and 4 hold only their own starts."""
    grid = ps.EDGE_GRID
    cap = (grid[0] - 1) + (grid[1] - 1)
    empty = ps.noise_field(grid, 31)
    empty[..., 3] = np.abs(empty[..., 3]) + 0.5
    quiet = []
    for seed in (32, 33):   # a closed contour in the middle, nothing at the boundary
        f = ps.noise_field(grid, seed)
        f[..., 3] = np.abs(f[..., 3]) + 0.1
        f[5:9, 4:8, 3] *= -1
        quiet.append(f)
    fields = [ps.noise_field(grid, 30), empty, quiet[0], ps.edge_fields()["alternating"], quiet[1]]
    ics = np.array([(0, 0), (18, 0), (-36, 13), (54, 0), (1 << 20, -(1 << 20))])
    step = np.float32(RES)
    v, l, s, c = run_blocks(hip, fields, ics, RES, ORIGIN, step)
    assert c[1] == 0 and np.all(s[1] == SENTINEL) and np.all(l[1] == ps.EMPTY) and np.all(v[1] == 0xffffffff)
    assert c[3] == cap and not np.any(s[3] == SENTINEL)
    assert c[2] == 0 and c[4] == 0 and np.all(s[2] == SENTINEL) and np.all(s[4] == SENTINEL) and np.all(s[5] == SENTINEL)
    for i in range(5):
        if i != 1:
            check_against((v[i], l[i], s[i], int(c[i]), s[i][:0]), oracle.process_polygon(fields[i], block_corner(ics[i]), step))


def test_bad_arguments_fail_on_the_host(hip):
    """Every call here returns before a launch: the pointers given are small live buffers or NULL."""
    from codecad_amd import hip_util
    buf = hip_util.Buffer(np.uint32, 64)
    p, stream = buf.device_ptr, hip.queue.handle
    corner = (ctypes.c_float * 4)(0, 0, 0, 0)
    origin = (ctypes.c_double * 3)(0, 0, 0)

    def grid(a, b):
        return (ctypes.c_uint32 * 2)(a, b)

    def bad(rc, text):
        assert rc == HU_ERR_BAD_ARG
        assert text in hip.lib.hu_last_error(), hip.lib.hu_last_error()

    single, batch = hip.lib.hu_process_polygon, hip.lib.hu_process_polygon_blocks
    # the single-block entry point takes the launch size (gx-1, gy-1)
    bad(single(corner, 1.0, p, grid(0, 4), p, p, p, p, stream), b"at least 2x2")
    bad(single(corner, 1.0, p, grid(4, 0), p, p, p, p, stream), b"at least 2x2")
    bad(single(corner, 1.0, p, grid(0xffffffff, 4), p, p, p, p, stream), b"at least 2x2")
    bad(single(corner, 1.0, p, grid(512, 4), p, p, p, p, stream), b"above 512")
    bad(single(corner, 1.0, p, grid(4, 512), p, p, p, p, stream), b"above 512")
    for i in range(2, 8):
        args = [corner, 1.0, p, grid(2, 2), p, p, p, p, stream]
        args[i] = None
        bad(single(*args), b"NULL")
    bad(single(None, 1.0, p, grid(2, 2), p, p, p, p, stream), b"NULL")
    # the batched one takes the corner grid (gx, gy)
    bad(batch(p, p, 1, 0.37, origin, 0.37, grid(1, 4), p, p, p, p, stream), b"at least 2x2")
    bad(batch(p, p, 1, 0.37, origin, 0.37, grid(4, 1), p, p, p, p, stream), b"at least 2x2")
    bad(batch(p, p, 1, 0.37, origin, 0.37, grid(513, 4), p, p, p, p, stream), b"above 512")
    bad(batch(p, p, 1, 0.37, origin, 0.37, grid(4, 513), p, p, p, p, stream), b"above 512")
    bad(batch(p, p, 65536, 0.37, origin, 0.37, grid(3, 3), p, p, p, p, stream), b"65535")
    for i in (0, 1, 4, 6, 7, 8, 9, 10):
        args = [p, p, 1, 0.37, origin, 0.37, grid(3, 3), p, p, p, p, stream]
        args[i] = None
        bad(batch(*args), b"NULL")
    assert batch(p, p, 0, 0.37, origin, 0.37, grid(3, 3), p, p, p, p, stream) == 0
    assert batch(None, None, 0, 0.37, origin, 0.37, grid(3, 3), None, None, None, None, stream) == 0
    buf.release()
