"""Raw volumes PAST THE GRID'S CAP: more units than the GRID_WAVEFRONTS wavefronts that id_volume.hpp's walking_blocks launches with
one unit a wavefront, so that HU_FOR_UNITS gives a wavefront a SECOND unit (and on 129 x 128 x 70 some a third).  For the column
walks of instance_geodesic.hip and instance_reach.hip and the line walks of instance_reach.hip and instance_tool.hip
(test_gpu_geodesic_raw.py, test_gpu_drainage.py, test_gpu_islands.py, test_gpu_tool_raw.py); test_wide_volumes_host.py proves on
the CPU that the cases bite and that their cheap references are the definitions'.

A wavefront w walks the units w, w + G, w + 2 G (G = GRID_WAVEFRONTS): KIND 0 are the units it walks first and third, KIND 1 those
it walks second.  The kinds differ so that anything a wavefront carried from one unit into the next would change the answer:
columns of kind 0 have both ends in R, flagged, with parts 0..31; half the columns of kind 1 begin outside R, the others begin
in R unflagged, with parts 32..62 (part 63 is in both, for `of` = 63).

THE REACH CASES DECOMPOSE.  R lies only in the columns with x + y even, so no two samples of R are lateral neighbours along z:
every layer component is one sample, its label its own index (own_labels), which the host test holds against layer_labels on a
small twin and on a crop.  What the flags become is then taken from the definitions at full size: `risen` is the least fixed
point grown by shifted arrays from ANY seeds (escape_set and grounded_set from theirs), drainage_scenes.floors the floors.  THE
FLAGS ARE CRAFTED: under the flags that the real seeds leave, no sample of R at the start of a column is ever unflagged when
something could be handed to it, and no carry could show.  Along x and y (hu_ground_seed) R is whole z lines of every second
line, so a component is a line and its root the sample at z = 0.

THE WALKS, emulated sample by sample over the words of a column (z >= nz is in nothing), once as written and once STALE, with the
state of unit u carried into unit u + G: geo_sweep, rise, floor, mark_starts, line_keys, line_rest; seeded_lines with the base
of the first unit reused.  The prefetched `next` word of k_reach_rise<true> has no emulation: carried over, the first word of a
second column would be walked under the labels of the LAST word of the column before, which the comparison of the whole label
buffer after the rise catches on every shape (test_gpu_drainage.py and test_gpu_islands.py, test_a_wavefront_walks_a_second_column).
WHAT CANNOT DIFFER, and is therefore no case: at nz = 70 the last word is ragged, so the carry bit of k_reach_rise<true> leaves
a column as 0 upwards and enters padding downwards -- 91 x 91 x 128 is there for it; NO state of k_ground_mark<true> can be carried
at any nz: its word loop takes one step beyond the last word, with empty ballots, which clears the carry and the due_* words
before the unit ends, and the due_* words are read only after they were assigned (mark_starts takes that step, so its stale walk
equals the honest one; the device cases guard the kernel's second unit as a whole, not a hoisted variable); and the holder of
k_tool_rest<false> alone, since under tops that hu_tool_tops wrote a sample is undercut only below a sample of S of its own
line -- its case carries the holder together with top, cut and crowd."""
import collections
import functools

import numpy

import raw_volume_scenes as raw
import drainage_scenes as drain
import islands_scenes as isl
import flow_length_scenes as flow
import tool_access_scenes as tool
from raw_volume_scenes import GRID_WAVEFRONTS, WIDE_NA, WIDE_LINES, WIDE_NZ, SOLID, EMPTY, NONE

FLAG = 0x80000000
COLUMN_SHAPES = collections.OrderedDict([("100x100x70", (100, 100, 70)), ("129x128x70", (129, 128, 70))])
REACH_SHAPES = collections.OrderedDict(list(COLUMN_SHAPES.items()) + [("91x91x128", (91, 91, 128))])
TWIN, TWIN_GRID = (6, 7, 70), 16           # the small twin: 42 columns under a grid of 16 wavefronts
TWIN_FULL = (6, 7, 128)
LINE_TWIN_GRID = 8
TOOL = tool.FLAT1
TOOL_OFS = (SOLID, 63)


def kinds(units, grid=GRID_WAVEFRONTS):
    """0 for the units a wavefront walks first or third, 1 for those it walks second."""
    return (numpy.arange(units) // grid) % 2


def walked(units, grid=GRID_WAVEFRONTS):
    """(wavefronts with a second unit, with a third)"""
    return max(0, min(units, 2 * grid) - grid), max(0, min(units, 3 * grid) - 2 * grid)


# ---- columns along z: the reach kernels -----------------------------------------------------------------------------------

Reach = collections.namedtuple("Reach", "ids r flags")


@functools.lru_cache(maxsize=None)
def reach_case(shape, member, grid=GRID_WAVEFRONTS):
    """`member` "empty": R = E, for drainage; "solid": R = S, for islands.  flags: the samples of R whose entry is flagged."""
    nx, ny, nz = shape
    columns = nx * ny
    rng = numpy.random.default_rng(7000 + sum(shape) + (member == "solid"))
    kind = kinds(columns, grid)[:, None]
    x, y = numpy.divmod(numpy.arange(columns), ny)
    r = (numpy.cumsum(rng.random((columns, nz)) < 0.3, axis=1) + rng.integers(0, 2, size=(columns, 1))) % 2 == 0     # runs
    r[:, 0] = r[:, -1] = (kind[:, 0] == 0) | (rng.random(columns) < 0.5)
    r &= ((x + y) % 2 == 0)[:, None]
    parts = numpy.where(kind == 0, rng.integers(0, 32, size=(columns, nz)), rng.integers(32, 63, size=(columns, nz)))
    parts[rng.random((columns, nz)) < 0.25] = 63
    ids = (numpy.where(r, parts, EMPTY) if member == "solid" else numpy.where(r, EMPTY, parts)).astype(numpy.uint8)
    flags = r & (rng.random((columns, nz)) < 0.1)
    flags[:, 0], flags[:, -1] = r[:, 0] & (kind[:, 0] == 0), r[:, -1] & (kind[:, 0] == 0)
    out = Reach(ids.reshape(shape), r.reshape(shape), flags.reshape(shape))
    for a in out:
        a.setflags(write=False)
    return out


def members(ids, member, of=SOLID):
    return ids == EMPTY if member == "empty" else isl.in_set_of(ids, of)


def buffer_indices(shape, pitch):
    """uint32[nx, ny, nz]: the index of every sample in a buffer of pitch `pitch`."""
    nx, ny, nz = shape
    return (numpy.arange(nx * ny, dtype=numpy.int64)[:, None] * pitch + numpy.arange(nz)).reshape(shape).astype(numpy.uint32)


def own_labels(r, pitch, flags=None):
    """uint32[nx][ny][pitch]: the label buffer after a flatten when every layer component of R is ONE sample -- its own index,
    NONE elsewhere and in the padding -- with bit 31 set on `flags`."""
    out = numpy.full(r.shape[:2] + (pitch,), NONE, dtype=numpy.uint32)
    q = buffer_indices(r.shape, pitch)
    if flags is not None:
        q = q | numpy.where(flags, FLAG, 0).astype(numpy.uint32)
    out[:, :, :r.shape[2]] = numpy.where(r, q, NONE)
    return out


def risen(r, seeds, axis, up):
    """The least subset of R that holds `seeds` & R and every p of R whose sample below or a lateral neighbour is in it: the
    definition of instance_reach.hip, grown by shifted arrays as escape_set and grounded_set grow theirs."""
    sign = 1 if up else -1
    x = seeds & r
    while True:
        grown = drain.shifted(x, axis, sign)
        for a in range(3):
            if a != axis:
                grown = grown | drain.shifted(x, a, 1) | drain.shifted(x, a, -1)
        grown = x | (r & grown)
        if numpy.array_equal(grown, x):
            return x
        x = grown


def trapped_of(ids, flagged, axis, up):
    """(trapped ids, 64 counts) of hu_drain_floor under the flags `flagged`: an unflagged sample of E takes its floor."""
    out = numpy.where((ids == EMPTY) & ~flagged, drain.floors(ids, axis, up), EMPTY).astype(numpy.uint8)
    return out, numpy.bincount(out.ravel(), minlength=256)[:64].tolist()


def marks_of(ids, s, grounded, axis, up):
    """[(ids, 64 counts)] of floating, start and join of hu_ground_mark under the flags `grounded`."""
    sign = 1 if up else -1
    f = s & ~grounded
    out = []
    for m in (f, f & ~isl.shifted(s, axis, sign), f & isl.shifted(grounded, axis, -sign)):
        v = numpy.where(m, ids, EMPTY).astype(numpy.uint8)
        out.append((v, numpy.bincount(v.ravel(), minlength=256)[:64].tolist()))
    return out


# ---- the column walks, emulated ---------------------------------------------------------------------------------------------

def _columns(a, up, fill):
    """[columns, 64 * segments] in the order of the walk: the padding of the last word is `fill`, downwards it comes FIRST."""
    nz = a.shape[-1]
    flat = a.reshape(-1, nz)
    out = numpy.full((flat.shape[0], -(-nz // 64) * 64), fill, dtype=flat.dtype)
    out[:, :nz] = flat
    return out if up else out[:, ::-1]


def _back(a, shape, up):
    return (a if up else a[:, ::-1])[:, :shape[2]].reshape(shape)


def _chained(walk, columns, first, stale, grid):
    """walk(slice of columns, state in) -> state out, chunk by chunk of `grid` units; stale: a chunk starts from what the chunk
    before left, unit for unit, else from `first`."""
    left = None
    for lo in range(0, columns, grid):
        n = min(grid, columns - lo)
        left = walk(slice(lo, lo + n), left[:n] if stale and left is not None else numpy.full(n, first))
    return left


def rise(r, flags, up, stale, grid=GRID_WAVEFRONTS):
    """k_reach_rise<true>, one pass over own labels -> the flagged samples.  State: the carry bit."""
    e, f = _columns(r, up, False), _columns(flags, up, False)
    out = numpy.zeros_like(e)

    def walk(at, carry):
        carry = carry.copy()
        for z in range(e.shape[1]):
            carry = e[at, z] & (f[at, z] | carry)
            out[at, z] = carry
        return carry
    _chained(walk, e.shape[0], False, stale, grid)
    return _back(out, r.shape, up)


def floor(ids, flagged, up, stale, grid=GRID_WAVEFRONTS):
    """k_drain_floor<true> -> the trapped ids.  State: the id of the last sample of S."""
    v, f = _columns(ids, up, EMPTY), _columns(flagged, up, False)
    active = _columns(numpy.ones(ids.shape, dtype=bool), up, False)
    out = numpy.full(v.shape, EMPTY, dtype=numpy.uint8)

    def walk(at, carry):
        carry = carry.copy()
        for z in range(v.shape[1]):
            held = active[at, z] & (v[at, z] == EMPTY) & ~f[at, z] & (carry != EMPTY)
            out[at, z] = numpy.where(held, carry, EMPTY)
            carry = numpy.where(v[at, z] != EMPTY, v[at, z], carry)
        return carry
    _chained(walk, v.shape[0], numpy.uint8(EMPTY), stale, grid)
    return _back(out, ids.shape, up)


def mark_starts(ids, s, grounded, up, stale, grid=GRID_WAVEFRONTS):
    """k_ground_mark<true> -> the start ids.  State: the carry bit, "the top sample of the word below is in S"; the kernel's
    word loop ends with a step of empty ballots that clears it, so nothing leaves a unit."""
    m, g, v = _columns(s, up, False), _columns(grounded, up, False), _columns(ids, up, EMPTY)
    out = numpy.full(v.shape, EMPTY, dtype=numpy.uint8)

    def walk(at, below):
        below = below.copy()
        for z in range(m.shape[1]):
            out[at, z] = numpy.where(m[at, z] & ~g[at, z] & ~below, v[at, z], EMPTY)
            below = m[at, z]
        return numpy.zeros_like(below)                                                # (the step beyond the last word: s = 0)
    _chained(walk, m.shape[0], False, stale, grid)
    return _back(out, ids.shape, up)


def geo_sweep(field, s, stale, grid=GRID_WAVEFRONTS):
    """k_geo_sweep_columns -> the field after the sweep.  State: the carry c, NONE before the walk up and again before the walk
    down; stale, the walk up of a unit starts from what the walk down of the unit before left."""
    d, m = _columns(field.astype(numpy.int64), True, NONE), _columns(s, True, False)

    def walk(at, c):
        for order in (range(d.shape[1]), range(d.shape[1] - 1, -1, -1)):
            for z in order:
                v = numpy.minimum(d[at, z], numpy.minimum(c + 1, NONE))
                d[at, z] = numpy.where(m[at, z], v, d[at, z])
                c = numpy.where(m[at, z], v, NONE)
            left, c = c, numpy.full(len(c), NONE, dtype=numpy.int64)
        return left
    _chained(walk, d.shape[0], numpy.int64(NONE), stale, grid)
    return _back(d, field.shape, True).astype(numpy.uint32)


# ---- the geodesic cases -------------------------------------------------------------------------------------------------------

GEO_OFS = (SOLID, 3, flow.EMPTY_SPACE)


@functools.lru_cache(maxsize=None)
def geo_ids(shape, grid=GRID_WAVEFRONTS):
    """flow_length_scenes.some_ids; the columns of kind 0 begin and end with part 3, in S for SOLID and for 3, or, every second
    one, with an empty sample, in S for EMPTY_SPACE."""
    ids = flow.some_ids(numpy.random.default_rng(8100 + sum(shape)), shape)
    first = (kinds(shape[0] * shape[1], grid) == 0).reshape(shape[:2])
    even = (numpy.arange(shape[0] * shape[1]) % 2 == 0).reshape(shape[:2])
    ids[first & even, 0] = ids[first & even, -1] = 3
    ids[first & ~even, 0] = ids[first & ~even, -1] = EMPTY
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def geo_field(shape, of, grid=GRID_WAVEFRONTS):
    """flow_length_scenes.some_field, no distance field; the first sample of a column of kind 0 holds a small value where it is
    in S, that of a column of kind 1 NONE: what the first column's walk down leaves would lower it."""
    s = flow.in_set_of(geo_ids(shape, grid), of)
    field = flow.some_field(numpy.random.default_rng(8200 + sum(shape) + flow.code(of)), shape, s)
    first = (kinds(shape[0] * shape[1], grid) == 0).reshape(shape[:2])
    field[:, :, 0] = numpy.where(s[:, :, 0], numpy.where(first, 5, NONE), field[:, :, 0])
    field.setflags(write=False)
    return field


# ---- lines along x and y --------------------------------------------------------------------------------------------------

def line_kinds(grid=GRID_WAVEFRONTS):
    """The kind of every line: a unit is a line's segment, and the grid holds whole lines."""
    segments = -(-WIDE_NZ // 64)
    assert grid % segments == 0
    return kinds(WIDE_LINES * segments, grid)[::segments]


def _placed(lines_first, axis):
    """[na][lines][z] as the volume of `axis`: along x the lines are the y, along y the x."""
    return numpy.ascontiguousarray(lines_first if axis == 0 else numpy.swapaxes(lines_first, 0, 1))


def _lines_first(volume, axis):
    return volume if axis == 0 else numpy.swapaxes(volume, 0, 1)


@functools.lru_cache(maxsize=None)
def tool_ids(axis, na, grid=GRID_WAVEFRONTS):
    """Lines of kind 0: noise of parts 0..31 and 63; of kind 1: half of them hold NO sample of S at all (the key is 0), the
    others noise of parts 32..63."""
    rng = numpy.random.default_rng(8300 + 10 * axis + na)
    shape = (na, WIDE_LINES, WIDE_NZ)
    kind = line_kinds(grid)[None, :, None]
    parts = numpy.where(kind == 0, rng.integers(0, 32, size=shape), rng.integers(32, 63, size=shape))
    parts[rng.random(shape) < 0.25] = 63
    ids = numpy.where(rng.random(shape) < 0.3, parts, EMPTY)
    bare = (kind == 1) & (rng.random((1, WIDE_LINES, 1)) < 0.5)
    ids = _placed(numpy.where(bare, EMPTY, ids).astype(numpy.uint8), axis)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def tool_reference(axis, na, up, of):
    return tool.reference_tool_access(tool_ids(axis, na), axis, up, TOOL, of, 64, pockets=False)


def keys_of(ref):
    return numpy.where(ref.tops > 0, ref.tops * 256 + (255 - ref.top_ids.astype(numpy.int64)), 0)


def _stale_lines(values, stale, grid):
    """[..., lines, z] -> what the lane of the same z held after the line its wavefront walked before, None for the first."""
    per = grid // (-(-WIDE_NZ // 64))
    out = numpy.zeros_like(values)
    out[..., per:, :] = values[..., :-per, :]
    seen = numpy.zeros(values.shape[-2], dtype=bool)
    seen[per:] = stale
    return out, seen[:, None]


def line_keys(ids, axis, up, of, stale, grid=GRID_WAVEFRONTS):
    """k_tool_tops<false> -> the keys [lines, nz].  State: key and open, a register per lane; stale, a lane that found a sample of
    S in the line before is not open and keeps that key."""
    lines = _lines_first(ids, axis)
    s = tool.in_set_of(lines, of)
    na = lines.shape[0]
    h = (numpy.arange(na) if up else na - 1 - numpy.arange(na))[:, None, None]
    heights = numpy.where(s, h + 1, 0)
    top = heights.max(axis=0)
    owner = numpy.take_along_axis(lines, heights.argmax(axis=0)[None], 0)[0]
    key = numpy.where(top > 0, top * 256 + (255 - owner.astype(numpy.int64)), 0)
    before, seen = _stale_lines(key, stale, grid)
    while stale and (seen & (before != 0) & (key != before)).any():                   # (a third unit: from the second's stale key)
        key = numpy.where(seen & (before != 0), before, key)
        before, seen = _stale_lines(key, stale, grid)
    return key


def line_rest(ids, axis, up, of, keys, cut, stale, grid=GRID_WAVEFRONTS):
    """k_tool_rest<false> -> (the rest ids, the holders the walk leaves [lines, nz]).  State: the holder, and top, cut and crowd where a wavefront loaded them once; stale, a
    unit walks under those of the unit before (a wavefront has at most two units here)."""
    lines = _lines_first(ids, axis)
    s = tool.in_set_of(lines, of)
    na = lines.shape[0]
    top, reach, crowd = keys >> 8, cut >> 8, cut & 255
    holder = numpy.full(lines.shape[1:], EMPTY, dtype=numpy.int64)
    if stale:
        honest = line_rest(ids, axis, up, of, keys, cut, False, grid)[1]
        (top, _), (reach, _), (crowd, _) = (_stale_lines(v, True, grid) for v in (top, reach, crowd))
        last, seen = _stale_lines(honest, True, grid)
        top, reach, crowd = (numpy.where(seen, v, w) for v, w in ((top, keys >> 8), (reach, cut >> 8), (crowd, cut & 255)))
        holder = numpy.where(seen, last, EMPTY)
    out = numpy.full(lines.shape, EMPTY, dtype=numpy.uint8)
    for t in range(na):
        at, h = (na - 1 - t, na - 1 - t) if up else (t, na - 1 - t)
        holder = numpy.where(s[at], lines[at], holder)
        out[at] = numpy.where(~s[at] & (h < top), holder, numpy.where(~s[at] & (h >= top) & (h < reach), crowd, EMPTY))
    return _placed(out, axis), holder


@functools.lru_cache(maxsize=None)
def seed_lines(axis, na, grid=GRID_WAVEFRONTS):
    """(ids, R): R is whole z lines of the lines with an even index, about half of them in every layer; lines of kind 0 hold
    parts 0..31, of kind 1 parts 32..63.  Within a layer of `axis` a component of R is one z line."""
    rng = numpy.random.default_rng(8400 + 10 * axis + na)
    r = (rng.random((na, WIDE_LINES, 1)) < 0.5) & (numpy.arange(WIDE_LINES) % 2 == 0)[None, :, None]
    r = numpy.broadcast_to(r, (na, WIDE_LINES, WIDE_NZ))
    parts = numpy.where(line_kinds(grid)[None, :, None] == 0, rng.integers(0, 32, size=r.shape), rng.integers(32, 64, size=r.shape))
    ids, r = _placed(numpy.where(r, parts, EMPTY).astype(numpy.uint8), axis), _placed(r, axis)
    ids.setflags(write=False), r.setflags(write=False)
    return ids, r


def line_labels(r, pitch, flagged=None):
    """uint32[nx][ny][pitch]: the label buffer after a flatten when every layer component of R is a z line: the index of the
    line's sample at z = 0, with bit 31 on that ROOT's own entry where `flagged` holds the line."""
    out = numpy.full(r.shape[:2] + (pitch,), NONE, dtype=numpy.uint32)
    root = buffer_indices(r.shape, pitch)[:, :, :1]
    out[:, :, :r.shape[2]] = numpy.where(r, root, NONE)
    if flagged is not None:
        out[:, :, 0] |= numpy.where(r[:, :, 0] & flagged[:, :, 0], FLAG, 0).astype(numpy.uint32)
    return out


def seeded_lines(r, axis, layer, reused, grid=GRID_WAVEFRONTS):
    """k_ground_seed along x or y -> the samples of R under a flagged root: those of layer `layer`.  `reused`: a wavefront's second
    unit takes the base of its first, and flags that line again."""
    at = numpy.zeros(r.shape, dtype=bool)
    index = [slice(None)] * 3
    index[axis] = layer
    at[tuple(index)] = True
    if reused:
        lines = _lines_first(at, axis)                                                # (a view)
        lines[:, grid // (-(-WIDE_NZ // 64)):, :] = False
    return r & at
