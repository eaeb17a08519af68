"""Raw part-id volumes and raw uint16 volumes for the entry points that walk the id volume, called alone: the thickness passes,
hu_blocking_lines, the overhang kernels and the component kernels (test_gpu_thickness_passes.py, test_gpu_blocking_raw.py,
test_gpu_overhang_raw.py, test_gpu_components_raw.py).  test_raw_volumes_host.py proves on the CPU that every case holds the
edge it is named for.  Everything is seeded; the references are those of thin_walls_scenes, disassembly_scenes,
overhangs_scenes and assembly_components_scenes, which take raw ids.

A device buffer is uint8 (or uint16) [nx][ny][pz], pz = ceil16(nz) unless a caller asks for a wider pitch (pitched_buffers.py);
the PADDING z in [nz, pz) belongs to nobody.  `padded` and
`padded16` fill it with a POISON chosen per consumer: values that would change the consumer's answer if a kernel read them as
data."""
import collections
import functools

import numpy

import thin_walls_scenes as thin
import disassembly_scenes as dis
import overhangs_scenes as over
import assembly_components_scenes as comp
from assembly_components_scenes import SOLID, EMPTY_SPACE, EMPTY, NONE

SOLID_CODE = 255                # `of` as the entry points take SOLID


def ceil16(n):
    return -(-int(n) // 16) * 16


def code(of):
    return SOLID_CODE if of == SOLID else int(of)


def _fill(dtype, values, poison, pitch=None):
    nx, ny, nz = values.shape
    pz = ceil16(nz) if pitch is None else int(pitch)
    assert pz % 16 == 0 and nz <= pz <= 65536
    out = numpy.empty((nx, ny, pz), dtype=dtype)
    out[:, :, :nz] = values
    if pz > nz:
        x, y, z = numpy.meshgrid(numpy.arange(nx), numpy.arange(ny), numpy.arange(nz, pz), indexing="ij")
        out[:, :, nz:] = poison(x, y, z)
    return out, pz


def padded(ids, poison, pitch=None):
    """(uint8[nx][ny][pz], pz): `ids`, and poison(x, y, z) (index arrays -> values) over the whole padding [nz, pz); pz is
    `pitch`, any multiple of 16 from nz on, or ceil16(nz) without one."""
    return _fill(numpy.uint8, ids, poison, pitch)


def padded16(values, fill, pitch=None):
    """The same for a uint16 volume."""
    return _fill(numpy.uint16, values, fill, pitch)


def alternating(a, b):
    """A poison that alternates a and b from sample to sample along every axis."""
    return lambda x, y, z: numpy.where((x + y + z) % 2 == 0, a, b)


def constant(v):
    return lambda x, y, z: numpy.full(x.shape, v)


# ---- the thickness passes: along z -----------------------------------------------------------------------------------------

Z_LATTICES = collections.OrderedDict([("3x5x130", ((3, 5, 130), 144)), ("2x3x64", ((2, 3, 64), 64)), ("2x3x65", ((2, 3, 65), 80)),
                                      ("1x1x1", ((1, 1, 1), 16))])
Z_OFS = (SOLID, 0, 63)
Z_PARAMS = ((0, 1), (1, 2), (8, 70), (63, 3970), (64, 4097), (65, 4226), (255, 65535))          # (K, cap)
RADIUS_SQ = 1000                # transform 2 of the z pass: the core is depth_sq > RADIUS_SQ
# the planted columns (x, y) of 3x5x130, per `of`: FAR is all in S (z = 64 lies 65 samples from the nearest background, which
# is outside the lattice), EDGE has its only background at z = 0 (z = 64 takes 64 * 64 from a tap in the segment below)
Z_FAR = {SOLID: (1, 2), 63: (1, 2), 0: (2, 4)}
Z_EDGE = {SOLID: (0, 2), 63: (0, 2), 0: (0, 3)}


@functools.lru_cache(maxsize=None)
def z_ids(name):
    """Ids from 0..63 with about 2 % background, and on 3x5x130 the planted columns."""
    shape = Z_LATTICES[name][0]
    rng = numpy.random.default_rng(1301 + sum(shape))
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.02] = EMPTY
    if name == "3x5x130":
        ids[1, 2, :], ids[2, 4, :] = 63, 0
        ids[0, 2, :], ids[0, 3, :] = 63, 0
        ids[0, 2, 0] = ids[0, 3, 0] = EMPTY
    elif name == "2x3x65":                                                        # S up to z = nz - 1 for of = 63 and of = 0 as well
        ids[1, 1, 60:], ids[0, 1, 60:] = 63, 0
    ids.setflags(write=False)
    return ids


def z_ids_poison(of):
    """Id 0 lowers nothing where it is in S, but it raises what `outside` = 0 would give; where `of` is another part it
    alternates with that part, so that the padding read as data changes the answer for every `of`."""
    return constant(0) if of in (SOLID, 0) else alternating(0, of)


def z_input_1(ids, of, cap):
    """The input of the z pass of transform 1."""
    return numpy.where(thin.in_set_of(ids, of), cap, 0)


@functools.lru_cache(maxsize=None)
def z_depth(name):
    """uint16 values around RADIUS_SQ, about 2 % above it (the core), RADIUS_SQ and RADIUS_SQ + 1 themselves among them; on
    3x5x130 column (1, 2) has no core and column (0, 1) its only core at z = 0."""
    shape = Z_LATTICES[name][0]
    rng = numpy.random.default_rng(977 + sum(shape))
    depth = rng.integers(RADIUS_SQ - 500, RADIUS_SQ + 1, size=shape)
    core = rng.random(shape) < 0.02
    depth[core] = rng.integers(RADIUS_SQ + 1, RADIUS_SQ + 500, size=int(core.sum()))
    if name == "3x5x130":
        depth[1, 2, :] = RADIUS_SQ
        depth[0, 1, :] = RADIUS_SQ - 1
        depth[0, 1, 0], depth[0, 1, 1] = RADIUS_SQ + 1, RADIUS_SQ
    elif depth.size > 1:
        depth[0, 0, 0], depth[-1, -1, -1] = RADIUS_SQ + 1, RADIUS_SQ
    else:
        depth[...] = RADIUS_SQ + 1
    depth = depth.astype(numpy.uint16)
    depth.setflags(write=False)
    return depth


Z_DEPTH_POISON = alternating(0, 65535)          # 65535 is core: as data it gives the input 0, the lowest there is


def z_input_2(depth, cap):
    """The input of the z pass of transform 2."""
    return numpy.where(depth.astype(numpy.int64) > RADIUS_SQ, 0, cap)


# ---- the thickness passes: along y and x -----------------------------------------------------------------------------------

AxisVolume = collections.namedtuple("AxisVolume", "shape pitch axis")
AXIS_VOLUMES = collections.OrderedDict([("y300", AxisVolume((3, 300, 21), 32, 1)), ("x300", AxisVolume((300, 5, 21), 32, 0)),
                                        ("x130", AxisVolume((130, 3, 16), 16, 0))])
AXIS_PARAMS = ((0, 65400, 256, 1), (96, 12000, 64, 1), (97, 12000, 64, 0), (255, 65535, 1, 0), (255, 65535, 7, 0), (255, 65535, 64, 0),
               (255, 65535, 300, 0), (255, 65535, 4096, 0), (10, 200, 236, 1), (10, 200, 5, 1))      # (K, cap, tile, lds)
OUTSIDES = ("zero", "cap", "half")
TOP = 65200                     # most inputs lie in [TOP, 65535]: TOP > 255 * 255, so no tap of them ever wins below the cap
# the planted columns, by (the other lateral index, z): ALONE holds one small value, 0, at position ALONE_AT(n), LATE one at
# position 2, EDGES zeros right before the edges of the tiles 64 and 236
ALONE, LATE, EDGES = (0, 3), (1, 5), (2, 7)
EDGE_POSITIONS = (63, 127, 191, 235)


def alone_at(n):
    return 54 if n >= 300 else 2


def outside_of(which, cap):
    return {"zero": 0, "cap": cap, "half": cap // 2}[which]


def lines_first(values, axis):
    """[n][other][z]: the pass's axis first."""
    return values if axis == 0 else numpy.swapaxes(values, 0, 1)


@functools.lru_cache(maxsize=None)
def axis_input(name):
    v = AXIS_VOLUMES[name]
    rng = numpy.random.default_rng(4242 + sum(v.shape))
    values = rng.integers(TOP, 65536, size=v.shape)
    small = rng.random(v.shape) < 0.02
    values[small] = rng.integers(0, 60, size=int(small.sum()))
    lines = lines_first(values, v.axis)                                            # a view
    n = lines.shape[0]
    for column in (ALONE, LATE, EDGES):
        lines[(slice(None),) + column] = rng.integers(TOP, 65536, size=n)
    lines[(alone_at(n),) + ALONE] = 0
    lines[(2,) + LATE] = 0
    for p in EDGE_POSITIONS:
        if p < n:
            lines[(p,) + EDGES] = 0
    values = values.astype(numpy.uint16)
    values.setflags(write=False)
    return values


def own_and_other_tile(values, axis, K, cap, outside, tile):
    """(own, other) int64 like `values`: the least in(i + k) + k * k over the taps |k| <= K that lie in the sample's own tile or
    outside the lattice, and over those that lie in another tile."""
    f = numpy.moveaxis(values.astype(numpy.int64), axis, 0)
    n = f.shape[0]
    big = numpy.int64(1) << 40
    own, other = numpy.full(f.shape, big), numpy.full(f.shape, big)
    at = numpy.arange(n)
    expand = (slice(None),) + (None,) * (f.ndim - 1)
    for k in range(-min(K, n + 1), min(K, n + 1) + 1):
        j = at + k
        inside = (j >= 0) & (j < n)
        tap = numpy.where(inside[expand], f[numpy.clip(j, 0, n - 1)], outside) + k * k
        same = (~inside | (j // tile == at // tile))[expand]
        own = numpy.where(same, numpy.minimum(own, tap), own)
        other = numpy.where(same, other, numpy.minimum(other, tap))
    return numpy.moveaxis(own, 0, axis), numpy.moveaxis(other, 0, axis)


def planted_far_tap(n, K, cap, outside):
    """Whether the zero planted in ALONE or in LATE decides the sample K positions above it: K * K must lie below the cap and
    below what the tap that leaves the lattice gives there.  On 300 positions it cannot for K = 255 unless `outside` is the cap:
    every sample is at most 150 from an end, and 150 * 150 + cap / 2 < 255 * 255."""
    for j in (alone_at(n), 2):
        i = j + K
        if K >= 1 and i < n and K * K < min(cap, outside + min(i + 1, n - i) ** 2):
            return True
    return False


AXIS_COUNTED_POISON = constant(65535)           # under a finishing pass: as data it reaches every cap and is counted
FINISH_PARAMS = ((10, 200, 236, 1), (96, 12000, 64, 1), (97, 12000, 64, 0))          # (K, cap, tile, lds) on x300
FINISH_OFS = (SOLID, 63)


@functools.lru_cache(maxsize=None)
def finish_ids():
    """64 parts and some 5 % of empty samples on the lattice of x300; part 63 is a fifth of the rest, so that of = 63 counts."""
    shape = AXIS_VOLUMES["x300"].shape
    rng = numpy.random.default_rng(6363)
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.2] = 63
    ids[rng.random(shape) < 0.05] = EMPTY
    ids.setflags(write=False)
    return ids


def finish_reference(K, cap, outside, of):
    """(out int64, core counts per id, thin ids, thin counts per id) of the x pass over axis_input("x300") and finish_ids()."""
    ids = finish_ids()
    out = thin.min_plus_1d(axis_input("x300"), 0, K, cap, outside)
    reached = out == cap
    thin_set = reached & thin.in_set_of(ids, of)
    return (out, [int((reached & (ids == p)).sum()) for p in range(64)], numpy.where(thin_set, ids, EMPTY).astype(numpy.uint8),
            [int((thin_set & (ids == p)).sum()) for p in range(64)])


# ---- hu_blocking_lines -------------------------------------------------------------------------------------------------------

BLOCK_SMALL = (5, 7, 130)
BLOCK_POISON = alternating(0, 1)
WIDE_NA = (1, 3, 8, 9, 17)
WIDE_LINES, WIDE_NZ, WIDE_PARTS = 5000, 70, 4
GRID_WAVEFRONTS = 4 * 2048      # id_volume.hpp: walking_blocks bounds the grid at 2048 workgroups of four wavefronts


@functools.lru_cache(maxsize=None)
def block_small_ids():
    rng = numpy.random.default_rng(5713)
    ids = rng.integers(0, 64, size=BLOCK_SMALL).astype(numpy.uint8)
    ids[rng.random(BLOCK_SMALL) < 0.3] = EMPTY
    ids[ids < 2] += 2                                                             # parts 0 and 1 own one sample each, on no common
    ids[0, 0, 10], ids[4, 6, 100] = 0, 1                                          # line: only the padding could pair them
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def block_small_reference(n):
    """(distance, witness) from the definition; ids from n up count as empty."""
    ids = block_small_ids()
    return dis.reference_blocking(numpy.where(ids < n, ids, EMPTY).astype(numpy.uint8), n)


def wide_shape(axis, na):
    return (na, WIDE_LINES, WIDE_NZ) if axis == 0 else (WIDE_LINES, na, WIDE_NZ)


def wide_units(axis, na):
    """(units of k_block_lines, segments)"""
    segments = -(-WIDE_NZ // 64)
    return WIDE_LINES * segments, segments


@functools.lru_cache(maxsize=None)
def wide_ids(axis, na):
    """The lines a wavefront walks FIRST (units below GRID_WAVEFRONTS) hold parts 0 and 1 only, those it walks second parts 2
    and 3 only: a second unit meets parts its first did not, and no line holds a pair of one part of each kind."""
    units, segments = wide_units(axis, na)
    first_lines = GRID_WAVEFRONTS // segments
    rng = numpy.random.default_rng(800 + 10 * axis + na)
    shape = (na, WIDE_LINES, WIDE_NZ)
    pick = rng.integers(0, 3, size=shape)
    low = numpy.array([0, 1, EMPTY], dtype=numpy.uint8)[pick]
    high = numpy.array([2, 3, EMPTY], dtype=numpy.uint8)[pick]
    ids = numpy.where((numpy.arange(WIDE_LINES) < first_lines)[None, :, None], low, high)
    ids = numpy.ascontiguousarray(ids if axis == 0 else numpy.swapaxes(ids, 0, 1))
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def wide_reference(axis, na):
    return dis.reference_blocking(wide_ids(axis, na), WIDE_PARTS)


def _walk(lines, n, last, axis, line0, keys):
    """k_block_lines' walk up `lines` [na][lines][z] from the last indices `last` [n][lines][z] (-1: none): lowers `keys`
    [n][n] and returns the last indices the walk leaves behind.  D is taken in 32 bits, as the kernel takes it."""
    na = lines.shape[0]
    prev = numpy.full(lines.shape[1:], EMPTY, dtype=numpy.uint8)
    last = last.copy()
    for t in range(na + 1):
        now = lines[t] if t < na else numpy.full(lines.shape[1:], EMPTY, dtype=numpy.uint8)     # (past the end: a run ends)
        changed = now != prev
        u, v = numpy.nonzero(changed & (prev != EMPTY))
        last[prev[u, v], u, v] = t - 1
        started = changed & (now != EMPTY)
        for i in range(n):
            u, v = numpy.nonzero(started & (last[i] >= 0) & (now != i))
            if len(u) == 0:
                continue
            p = last[i, u, v].astype(numpy.uint64)
            d = ((numpy.uint64(t) - p) & numpy.uint64(0xffffffff)) << numpy.uint64(48)
            line = (u + line0).astype(numpy.uint64)
            x, y = (p, line) if axis == 0 else (line, p)
            key = d | x << numpy.uint64(32) | y << numpy.uint64(16) | v.astype(numpy.uint64)
            numpy.minimum.at(keys[i], now[u, v], key)
        prev = now
    return last


def walked_keys(ids, axis, n, stale):
    """uint64[n, n]: the key table of axis 0 or 1 as k_block_lines' wavefronts find it.  `stale`: a wavefront's second unit
    starts from the last indices its first unit left in LDS, as it would if nothing reset the mask of the parts seen."""
    lines = ids if axis == 0 else numpy.swapaxes(ids, 0, 1)                       # [na][lines][z]
    segments = -(-ids.shape[2] // 64)
    assert GRID_WAVEFRONTS % segments == 0                                        # a wavefront's units are the same z of two lines
    first_lines = min(lines.shape[1], GRID_WAVEFRONTS // segments)
    keys = numpy.full((n, n), numpy.uint64(0xffffffffffffffff), dtype=numpy.uint64)
    none = numpy.full((n,) + lines.shape[1:], -1, dtype=numpy.int64)
    left = _walk(lines[:, :first_lines], n, none[:, :first_lines], axis, 0, keys)
    second = lines.shape[1] - first_lines
    assert second <= first_lines                                                  # no wavefront walks a third unit
    if second:
        _walk(lines[:, first_lines:], n, left[:, :second] if stale else none[:, :second], axis, first_lines, keys)
    return keys


# ---- the overhang kernels ----------------------------------------------------------------------------------------------------

OVER_VOLUMES = collections.OrderedDict([("noise", ((5, 7, 130), 144)), ("empty", ((5, 7, 130), 144)), ("line64", ((1, 1, 64), 64))])
OVER_REACH = (0, 1, 2, 4, 5, 8)
OVER_OFS = (SOLID, 0, 63)
OVER_POISON = alternating(EMPTY, 63)


@functools.lru_cache(maxsize=None)
def over_ids(name):
    shape = OVER_VOLUMES[name][0]
    rng = numpy.random.default_rng(4501 + sum(shape))
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.2] = 63                                             # enough of part 63 for of = 63
    ids[rng.random(shape) < 0.1] = 0
    ids[rng.random(shape) < (1.0 if name == "empty" else 0.55)] = EMPTY
    if name == "noise":                                                           # overhangs in the layer z = nz - 1 whose lateral tap
        ids[1, 3:6, 129] = ids[1, 4, 128] = EMPTY                                 # at z = nz would meet a 63 of the padding: along +x
        ids[2:5, 2, 129] = ids[3, 2, 128] = EMPTY                                 # ... and along -y
        ids[2, 4, 129] = ids[3, 1, 129] = 63
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def over_reference(name, axis, up, reach_sq, of):
    return over.reference_overhangs(over_ids(name), axis, up, reach_sq, of, 64)


# ---- the reach kernels and hu_contact_faces ---------------------------------------------------------------------------------

DRAIN_POISON = alternating(63, EMPTY)           # read as data, it would open ways out and lay floors
CONTACT_POISON = alternating(0, 1)              # ... it would make contacts


def ground_poison(of):
    """Empty and an id of S: read as data, it would ground, join and close starts."""
    return alternating(63 if of == SOLID else of, EMPTY)


# ---- the component kernels ---------------------------------------------------------------------------------------------------

COMP_VOLUMES = collections.OrderedDict([("noise", ((9, 17, 33), 48)), ("line130", ((1, 1, 130), 144))])
COMP_POISON = alternating(EMPTY, 63)


@functools.lru_cache(maxsize=None)
def comp_ids(name):
    shape = COMP_VOLUMES[name][0]
    rng = numpy.random.default_rng(9173 + sum(shape))
    ids = rng.integers(0, 64, size=shape).astype(numpy.uint8)
    ids[rng.random(shape) < 0.5] = EMPTY
    ids[0, 0, 5:8] = 63, EMPTY, 0                                                 # bit 63 and bit 0 of `parts` under either `solid`
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def comp_reference(name, solid):
    return comp.reference_components(comp_ids(name), SOLID if solid else EMPTY_SPACE)
