"""The outlines of an assembly on a STACK of parallel planes -- the layers of a print, the frames of a fly-through of a
section, the cross-section area along an axis --, every layer in one traversal of the device.

`layer_outlines(asm, plane, resolution, heights) -> Layers`.  `heights` are finite offsets along `plane.normal` from
`plane.origin`, strictly increasing, 1 to 2^20 of them (`layer_heights` gives the mid-layer heights of a layer height).
LAYER l is the cut of `section_outlines()` (section_outlines.py; its docstring defines the ring of samples, the shifted
indices, squares, edges, strict insideness, the crossing t, the direction of a segment and the saddles) on

    planes[l] = plane._replace(origin=float32(float64(plane.origin) + float64(plane.normal) * heights[l])),

the frame vectors those of `plane`, untouched.  ONE LATTICE serves all layers: `step`, `dims` = (nu, nv) and `first` are
`section.lattice(instances, plane, resolution)`'s, of the base plane and of no layer; the sample (0, 0) of layer l sits at
`corners[l]` = float32(float64(planes[l].origin) + u * first[0] + v * first[1]) (the expression of `section.lattice`) and
its samples at `section.sample_positions(plane, corners[l], step, i, j)`.  For `Plane.xy(0)` and its like, layer l is bit
for bit `section_outlines(asm, Plane.xy(heights[l]), resolution)`.

CANDIDATES.  The windows of squares along u and v are `square_windows(section.windows(...))` of the base plane's projection
WITHOUT its test along the normal.  Instance k is a candidate of layer l unless its box lies on one side of planes[l] by more
than a step: d = (box corners - float64(planes[l].origin)) . normal, taken as (d_x n_x + d_y n_y) + d_z n_z in float64, and k
is no candidate when min d > step or max d < -step -- the test of `section.windows`.  Heights increase, so an instance's
candidate layers are a contiguous range.

A ROW is the 16-byte row of every traversal over instances with the layer in word 1: {a0 | b0 << 16, layer, mask lo, mask
hi}.  The host seeds, per layer, the tiles of `cells.top_side(squares, first=64, factor=8)` squares (the value of
`section_outlines`, whatever the number of layers) that the window of a candidate of that layer reaches, with those
candidates; rows with an empty mask are dropped; rows are ordered by layer, then as `cell_rows` orders them.  A layer without
a candidate has no row, and when no layer has one nothing is launched (`runs == 0`).  `cull=False` lists every tile of 8 x 8
squares of every layer that has a candidate, with all of that layer's candidates, and runs the finest level alone.

A RECORD is 16 bytes {a | b << 16, k | e_from << 8 | e_to << 10 | layer << 12, t_from, t_to} (LAYER_SEGMENT, `unpack`); the
device's order is unspecified and the host sorts by (layer, k, b, a, e_from).  The kernels are csrc/instance_layers.hip:
the outline kernels with the plane's corner read from a table by the row's layer, driven by `_instance_cells.traverse` as it
is -- one table, one set of lists, one synchronisation.
"""
import collections

import numpy

from . import _instance_cells as cells
from . import hip_util
from .hip_util import manager as hip_manager
from ._instance_cells import Instance
from .section import Plane, lattice, windows, _projected
from .section_outlines import SEGMENT, Outlines, checked_samples, square_windows, radius, stitch

_TILE = 8
MAX_LAYERS = 1 << 20                # a record keeps the layer in the 20 bits above bit 12
MAX_TOP_ROWS = 1 << 22
_CHUNK = 4096                       # layers whose candidates are found at a time

# a segment as the device writes it: 16 bytes {a | b << 16, k | e_from << 8 | e_to << 10 | layer << 12, t_from, t_to}
LAYER_SEGMENT = numpy.dtype([("a", "<u2"), ("b", "<u2"), ("word", "<u4"), ("t_from", "<f4"), ("t_to", "<f4")])
assert LAYER_SEGMENT.itemsize == 16


def pack(k, e_from, e_to, layer):
    """uint32: word 1 of a record, k | e_from << 8 | e_to << 10 | layer << 12."""
    k, e_from, e_to, layer = (numpy.asarray(x, dtype=numpy.uint32) for x in (k, e_from, e_to, layer))
    return k | (e_from << numpy.uint32(8)) | (e_to << numpy.uint32(10)) | (layer << numpy.uint32(12))


def unpack(word):
    """(k, e_from, e_to, layer) of word 1 of a record, int64 each."""
    word = numpy.asarray(word, dtype=numpy.uint32).astype(numpy.int64)
    return word & 0xff, (word >> 8) & 3, (word >> 10) & 3, word >> 12


def sort_records(records):
    """The records (LAYER_SEGMENT) sorted by (layer, k, b, a, e_from)."""
    records = numpy.asarray(records, dtype=LAYER_SEGMENT)
    k, e_from, _, layer = unpack(records["word"])
    return records[numpy.lexsort((e_from, records["a"], records["b"], k, layer))]


def to_segments(records):
    """The records as SEGMENT records of section_outlines (the layer is dropped)."""
    records = numpy.asarray(records, dtype=LAYER_SEGMENT)
    out = numpy.zeros(len(records), dtype=SEGMENT)
    out["k"], out["e_from"], out["e_to"], _ = unpack(records["word"])
    for field in ("a", "b", "t_from", "t_to"):
        out[field] = records[field]
    return out


class Layers(collections.namedtuple("Layers", "instances plane heights planes corners step dims segments layer_counts counts "
                                              "evaluations runs")):
    """`instances`, `plane`, `step`, `dims`: as Outlines', of the base plane; `heights` (float64[L]); `planes[l]` and
    `corners[l]` (float32[L, 3]): the plane of layer l and its sample (0, 0); `segments`: the LAYER_SEGMENT records of all
    layers sorted by (layer, k, b, a, e_from); `layer_counts[l, k]` (int64[L, n]): the segments of instance k on layer l,
    counted on the host; `counts[k]`: the segments of instance k on all layers, counted on the device; `evaluations`,
    `runs`: as Outlines'."""

    __slots__ = ()

    def _first(self):
        return lattice([i.instance for i in self.instances], self.plane, self.step)[3]

    def _layer(self, l, first):
        lo, hi = numpy.searchsorted(unpack(self.segments["word"])[3], [l, l + 1])
        segments = to_segments(self.segments[lo:hi])
        return Outlines(self.instances, self.planes[l], self.corners[l], self.step, self.dims, segments,
                        stitch(segments, len(self.instances), first, float(self.step)), self.layer_counts[l].copy(), 0, 0)

    def layer(self, l):
        """The Outlines of layer l: `planes[l]`, `corners[l]`, the layer's records as SEGMENT records and their loops
        (`evaluations` and `runs` are the stack's and left 0 here)."""
        l = int(l)
        if not 0 <= l < len(self.heights):
            raise IndexError("layer %d of %d" % (l, len(self.heights)))
        return self._layer(l, self._first())

    def areas(self):
        """float64[L, n]: per layer and instance, the sum of the signed areas of its closed loops."""
        out = numpy.zeros(self.layer_counts.shape, dtype=numpy.float64)
        first = self._first()
        for l in numpy.flatnonzero(self.layer_counts.sum(axis=1)):
            for k, loops in enumerate(self._layer(int(l), first).loops):
                out[l, k] = sum(loop.area for loop in loops if loop.closed)
        return out


def checked_heights(heights):
    """float64[L] of `heights`, or ValueError: finite, strictly increasing, 1 <= L <= 2^20."""
    try:
        h = numpy.array(heights, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise ValueError("heights must be a sequence of numbers, not %r" % (heights,))
    if h.ndim != 1 or not 1 <= len(h) <= MAX_LAYERS:
        raise ValueError("layer_outlines takes 1 to 2^20 heights, not an array of shape %s" % (h.shape,))
    if not numpy.isfinite(h).all() or not (numpy.diff(h) > 0).all():
        raise ValueError("heights must be finite and strictly increasing")
    return h


def layer_heights(asm, plane, layer_height):
    """float64[L]: the mid-layer heights lo + (l + 0.5) * layer_height, l < ceil((hi - lo) / layer_height), over the extent
    lo .. hi of the visible instances' boxes along `plane.normal` from `plane.origin` (none for no visible instance).
    ValueError for a layer height that is not positive and finite or gives more than 2^20 layers."""
    if not isinstance(plane, Plane):
        raise ValueError("layer_heights takes a codecad_amd.Plane, not %r" % (plane,))
    if not (isinstance(layer_height, (int, float, numpy.floating, numpy.integer)) and numpy.isfinite(layer_height) and layer_height > 0):
        raise ValueError("layer_height must be a positive finite number, not %r" % (layer_height,))
    instances = cells.visible(asm, 1.0)
    if not instances:
        return numpy.zeros(0, dtype=numpy.float64)
    along = _projected(instances, plane)[:, :, 2]
    lo, hi = float(along.min()), float(along.max())
    count = numpy.ceil((hi - lo) / float(layer_height))
    if count > MAX_LAYERS:
        raise ValueError("layer_height %g gives %d layers: at most 2^20" % (layer_height, count))
    return lo + (numpy.arange(int(count), dtype=numpy.float64) + 0.5) * float(layer_height)


def layer_planes(plane, heights, first):
    """(planes, corners float32[L, 3]) of the layers at `heights` (the module's docstring)."""
    o, u, v, normal = (x.astype(numpy.float64) for x in (plane.origin, plane.u, plane.v, plane.normal))
    origins = (o[None, :] + normal[None, :] * numpy.asarray(heights, dtype=numpy.float64)[:, None]).astype(numpy.float32)
    corners = (origins.astype(numpy.float64) + u * first[0] + v * first[1]).astype(numpy.float32)
    return [plane._replace(origin=origin) for origin in origins], corners


def box_corners(instances):
    """float64 (n, 8, 3): the corners of every instance's bounding box, in the order of section._projected."""
    out = numpy.zeros((len(instances), 8, 3))
    for n, inst in enumerate(instances):
        box = inst.shape().bounding_box()
        ab = (numpy.array(tuple(box.a), dtype=numpy.float64), numpy.array(tuple(box.b), dtype=numpy.float64))
        out[n] = [[ab[(c >> k) & 1][k] for k in range(3)] for c in range(8)]
    return out


def candidates(boxes, origins, normal, step):
    """bool[L, n]: is instance k a candidate of the layer with the (float32) origin origins[l] (the module's docstring)."""
    step, normal = float(step), numpy.asarray(normal).astype(numpy.float64)
    origins = numpy.asarray(origins).astype(numpy.float64).reshape(-1, 3)
    out = numpy.zeros((len(origins), len(boxes)), dtype=bool)
    if not len(boxes):
        return out
    for at in range(0, len(origins), _CHUNK):
        d = boxes[None, :, :, :] - origins[at:at + _CHUNK, None, None, :]
        along = (d[..., 0] * normal[0] + d[..., 1] * normal[1]) + d[..., 2] * normal[2]
        out[at:at + _CHUNK] = ~((along.min(axis=2) > step) | (along.max(axis=2) < -step))
    return out


def top_rows(wins, candidate, squares, side, everywhere=False):
    """uint32[m, 4]: the rows of the top level, {a0 | b0 << 16, layer, mask lo, mask hi}: per layer, the tiles of `side`
    squares that the window (`wins`, int64[n, 2, 3]) of a candidate of the layer (`candidate`, bool[L, n]) reaches, with
    those candidates; ordered by layer, then as cells.cell_rows orders them.  `everywhere`: every tile of the lattice of a
    layer that has a candidate, with all its candidates.  ValueError for more than 2^22 rows."""
    dims3 = numpy.array([squares[0], squares[1], 1], dtype=numpy.int64)
    wins = numpy.array(wins, dtype=numpy.int64)
    if everywhere:
        wins[:, 0], wins[:, 1] = 0, dims3 - 1
    n_layers, n = candidate.shape
    if n == 0:
        return numpy.zeros((0, 4), dtype=numpy.uint32)
    masks = (candidate.astype(numpy.uint64) << numpy.arange(n, dtype=numpy.uint64)).sum(axis=1, dtype=numpy.uint64)
    distinct, which = numpy.unique(masks, return_inverse=True)          # (contiguous ranges of layers: at most 2 n + 1)
    of_mask = []
    for mask in distinct.tolist():
        mine = wins.copy()
        absent = numpy.array([not (mask >> k) & 1 for k in range(n)], dtype=bool)
        mine[absent, 0, :2], mine[absent, 1, :2] = 65536, 0            # (an empty window, as section.windows gives)
        of_mask.append(cells.cell_rows(mine, dims3, side, least=1))
    per_layer = numpy.array([len(r) for r in of_mask], dtype=numpy.int64)[which]
    total = int(per_layer.sum())
    if total > MAX_TOP_ROWS:
        raise ValueError("%d layers give %d top rows: at most 2^22" % (n_layers, total))
    start = numpy.cumsum(per_layer) - per_layer
    rows = numpy.zeros((total, 4), dtype=numpy.uint32)
    for m, tiles in enumerate(of_mask):
        layers = numpy.flatnonzero(which == m)
        if len(tiles) == 0 or len(layers) == 0:
            continue
        at = (start[layers][:, None] + numpy.arange(len(tiles))[None, :]).reshape(-1)
        rows[at] = numpy.tile(tiles, (len(layers), 1))
        rows[at, 1] = numpy.repeat(layers, len(tiles))
    return rows


def _result(named, plane, heights, planes, corners, step, dims, records, counts, evaluations, runs):
    n = len(named)
    k, _, _, layer = unpack(records["word"])
    layer_counts = numpy.bincount(layer * n + k, minlength=len(heights) * n).reshape(len(heights), n).astype(numpy.int64) if n else \
        numpy.zeros((len(heights), 0), dtype=numpy.int64)
    return Layers(named, plane, heights, planes, corners, step, tuple(int(d) for d in dims), records, layer_counts, counts, evaluations, runs)


Seed = collections.namedtuple("Seed", "step dims first planes corners wins squares side top")


def seed(instances, plane, resolution, heights, cull=True):
    """What the host prepares of a stack (the module's docstring) -> Seed: the lattice (`step`, `dims`, `first`), the layers'
    `planes` and `corners`, the windows of squares `wins`, the lattice of `squares`, the `side` of the top tiles and the `top`
    rows."""
    _, step, dims, first, projected = lattice(instances, plane, resolution)
    checked_samples(resolution, dims)
    planes, corners = layer_planes(plane, heights, first)
    flat = projected.copy()
    flat[:, :, 2] = 0.0                                  # the windows along u and v alone: every layer has its own test
    wins = square_windows(windows(flat, first, step, dims))
    squares = numpy.array([dims[0] + 1, dims[1] + 1, 1], dtype=numpy.int64)
    side = cells.top_side(squares, first=_TILE * _TILE, factor=_TILE) if cull else _TILE
    candidate = candidates(box_corners(instances), numpy.stack([p.origin for p in planes]), plane.normal, step)
    return Seed(step, dims, first, planes, corners, wins, squares, side, top_rows(wins, candidate, squares, side, everywhere=not cull))


def layer_outlines(asm, plane, resolution, heights, cull=True, initial_capacity=None, segment_capacity=None):
    """The outlines of the 3D assembly `asm` on the planes parallel to `plane` at `heights` along its normal, at `resolution`
    (the module's docstring) -> Layers.

    `cull`, `initial_capacity` and `segment_capacity` are section_outlines()'s (the first capacity of the segment buffer is
    a guess from the lattice's perimeter per layer that has a row).  Raises the ValueErrors of section_outlines(), and
    ValueError for heights that are not 1 to 2^20 finite, strictly increasing numbers and for more than 2^22 top rows."""
    if not isinstance(plane, Plane):
        raise ValueError("layer_outlines takes a codecad_amd.Plane, not %r" % (plane,))
    instances = cells.visible(asm, resolution)
    heights = checked_heights(heights)
    step, dims, first, planes, corners, wins, squares, side, top = seed(instances, plane, resolution, heights, cull)
    n, n_layers = len(instances), len(heights)
    named = [Instance(i.name, i) for i in instances]
    empty = numpy.zeros(0, dtype=LAYER_SEGMENT)
    if len(top) == 0:
        return _result(named, plane, heights, planes, corners, step, dims, empty, numpy.zeros(n, dtype=numpy.int64), 0, 0)
    if segment_capacity is None:
        capacity = min((8 * int(squares[0] + squares[1]) + 64) * len(numpy.unique(top[:, 1])), 1 << 22)
    else:
        capacity = max(1, int(segment_capacity))
    table = numpy.zeros((n_layers, 4), dtype=numpy.float32)
    table[:, :3] = corners
    table_dev = hip_util.Buffer(numpy.float32, table.shape, queue=hip_manager.queue)
    table_dev.enqueue_write(table)
    try:
        evaluations, totals, runs, rows = cells.traverse_records(
            instances, top, side, corners[0], step, squares, initial_capacity, capacity, 4, thr=lambda child: radius(child, step),
            cells="hu_layer_tiles", leaf="hu_layer_leaf", wins=wins, factor=_TILE, frame=plane.frame() + (table_dev.device_ptr, n_layers),
            too_many="%d segments: more than one buffer of 2^32 records holds")
    finally:
        table_dev.release()
    records = sort_records(rows.view(LAYER_SEGMENT).reshape(-1))
    return _result(named, plane, heights, planes, corners, step, dims, records, totals[1:].astype(numpy.int64), evaluations, runs)
