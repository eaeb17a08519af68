"""The scenarios of the layered outlines (test_layer_outlines_host.py shows on the CPU what each holds;
test_gpu_layer_outlines.py runs them on the device) and their CPU reference.

The REFERENCE STACK is built from the pieces of test_section_outlines_host.py: per layer the oracle at
`sample_positions(plane, corners[l], ...)` over the ringed indices (`ringed_values`), the segments derived from the crossed
edges (`segments_of`), the layer number added, the layers in order.  Planes and corners are restated here from the
definitions in codecad_amd/layer_outlines.py, layer by layer.  The REFERENCE TRAVERSAL is `reference_traversal` of that
file with the corner and the candidates of each row's layer: the candidates from `section._projected` about the layer's own
plane, the windows along u and v from the base plane.
"""
import collections
import functools

import numpy

from codecad_amd import nodes, _instance_cells
from codecad_amd.section import Plane, lattice, windows, sample_positions, _projected
from codecad_amd.section_outlines import square_windows, radius
from codecad_amd.layer_outlines import LAYER_SEGMENT, layer_heights
import oracle

import test_section_host as tsh
import heavy_instances
import test_section_outlines_host as tso

Reference = collections.namedtuple("Reference", "instances plane heights planes corners step dims first w segments counts layer_counts")
Traversal = collections.namedtuple("Traversal", "rows evaluations")


def planes_of(plane, heights, first):
    o, u, v, normal = (x.astype(numpy.float64) for x in (plane.origin, plane.u, plane.v, plane.normal))
    planes, corners = [], []
    for h in heights:
        origin = (o + normal * float(h)).astype(numpy.float32)
        planes.append(plane._replace(origin=origin))
        corners.append((origin.astype(numpy.float64) + u * first[0] + v * first[1]).astype(numpy.float32))
    return planes, numpy.array(corners, dtype=numpy.float32).reshape(-1, 3)


def records_of(segments, layer):
    """SEGMENT records of one layer as LAYER_SEGMENT records (the word written out here, not through the package's pack)."""
    out = numpy.zeros(len(segments), dtype=LAYER_SEGMENT)
    for field in ("a", "b", "t_from", "t_to"):
        out[field] = segments[field]
    out["word"] = [int(s["k"]) + int(s["e_from"]) * 256 + int(s["e_to"]) * 1024 + int(layer) * 4096 for s in segments]
    return out


def reference_layers(asm, plane, resolution, heights):
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    planes, corners = planes_of(plane, heights, first)
    w, records = [], []
    for l in range(len(heights)):
        w.append(tso.ringed_values(instances, plane, corners[l], step, dims))
        records.append(records_of(tso.segments_of(w[-1]), l))
    layer_counts = numpy.array([numpy.bincount(r["word"] & 0xff, minlength=len(instances)) for r in records], dtype=numpy.int64)
    return Reference(instances, plane, numpy.array(heights, dtype=numpy.float64), planes, corners, step, dims, first, w,
                     numpy.concatenate(records), layer_counts.sum(axis=0), layer_counts)


def layer_candidates(instances, planes, step):
    """[the instances that are candidates of layer l]: the test along the normal of section.windows, about the layer's plane."""
    out = []
    for p in planes:
        along = _projected(instances, p)[:, :, 2]
        out.append([k for k in range(len(instances)) if not (along[k].min() > float(step) or along[k].max() < -float(step))])
    return out


def base_windows(instances, plane, resolution):
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    on_plane = projected.copy()
    on_plane[:, :, 2] = 0
    return square_windows(windows(on_plane, first, step, dims))


def reference_top_rows(asm, plane, resolution, heights, cull=True):
    """[(layer, a0, b0, mask)] in the order the host lists them."""
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    planes, corners = planes_of(plane, heights, first)
    wins = base_windows(instances, plane, resolution)
    squares = numpy.array([dims[0] + 1, dims[1] + 1, 1])
    side = _instance_cells.top_side(squares, first=64, factor=8) if cull else 8
    rows = []
    for l, ks in enumerate(layer_candidates(instances, planes, step)):
        mine = wins.copy()
        for k in range(len(instances)):
            if k not in ks:
                mine[k, 0, :2], mine[k, 1, :2] = 65536, 0
            elif not cull:
                mine[k, 0, :2], mine[k, 1, :2] = 0, squares[:2] - 1
        for r in _instance_cells.cell_rows(mine, squares, side, least=1):
            rows.append((l, int(r[0]) & 0xffff, int(r[0]) >> 16, int(r[2]) | (int(r[3]) << 32)))
    return rows, side


def reference_layer_traversal(asm, plane, resolution, heights, cull=True):
    """`reference_traversal` of test_section_outlines_host.py over the rows of all layers: the corner of a row's layer in the
    position formula, the layer handed down to the children -> the rows {(layer, a0, b0, mask)} of every level and the
    evaluations of all levels."""
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    planes, corners = planes_of(plane, heights, first)
    wins = base_windows(instances, plane, resolution)
    squares = numpy.array([dims[0] + 1, dims[1] + 1, 1])
    tapes = [nodes.make_program(i.shape()) for i in instances]
    tiles, side = reference_top_rows(asm, plane, resolution, heights, cull)
    rows, evaluations = [sorted(tiles)], 0
    if not tiles:
        return Traversal(rows, 0)
    while side > 8:
        child = side // 8
        r, children = radius(child, step), []
        for l, a0, b0, mask in tiles:
            xs, ys = a0 + numpy.arange(8) * child, b0 + numpy.arange(8) * child
            ks = [k for k in range(len(instances)) if mask >> k & 1]
            points = sample_positions(plane, corners[l], step, (xs - 1 + child / 2).astype(numpy.float32), (ys - 1 + child / 2).astype(numpy.float32))
            w = numpy.stack([oracle.evaluate_points(tapes[k], points.reshape(-1, 3))[:, 3].reshape(8, 8) for k in ks])
            for j, y in enumerate(ys):
                for i, x in enumerate(xs):
                    if x >= squares[0] or y >= squares[1]:
                        continue
                    evaluations += len(ks)
                    keep = 0
                    for n, k in enumerate(ks):
                        if not (x <= wins[k, 1, 0] and x + child - 1 >= wins[k, 0, 0] and y <= wins[k, 1, 1] and y + child - 1 >= wins[k, 0, 1]):
                            continue
                        if not w[n, j, i] >= r and not w[n, j, i] <= -r:
                            keep |= 1 << k
                    if keep:
                        children.append((l, int(x), int(y), keep))
        tiles, side = children, child
        rows.append(sorted(tiles))
    for l, a0, b0, mask in tiles:      # a finest tile: the samples a0 .. a0 + 8 by b0 .. b0 + 8 that exist
        evaluations += (min(a0 + 8, squares[0]) - a0 + 1) * (min(b0 + 8, squares[1]) - b0 + 1) * bin(mask).count("1")
    return Traversal(rows, int(evaluations))


def records_reached(ref, leaf_rows):
    """The reference's records in the squares and of the candidates of the finest rows: what the traversal emits."""
    masks = {(l, a0, b0): mask for l, a0, b0, mask in leaf_rows}
    s = ref.segments
    keep = [bool(masks.get((int(word) >> 12, int(a) & ~7, int(b) & ~7), 0) >> (int(word) & 0xff) & 1)
            for a, b, word in zip(s["a"], s["b"], s["word"])]
    return s[numpy.array(keep, dtype=bool)] if len(s) else s


# ---- the scenarios ----------------------------------------------------------------------------------------------------

def _boxes_and_ball():
    asm = tsh.boxes_and_ball()
    plane = tso.oblique_of(asm)
    along = _projected(_instance_cells.visible(asm, 0.0625), plane)[:, :, 2]
    return asm, plane, 0.0625, layer_heights(asm, plane, (along.max() - along.min()) / 5)


def _far():
    asm = tsh.far_assembly(tso.FAR_RESOLUTION)
    return asm, Plane(tsh.centre_of(asm), (1, 1, 2)), tso.FAR_RESOLUTION, [-tso.FAR_RESOLUTION, 0.0, tso.FAR_RESOLUTION]


# name -> (assembly, base plane, resolution, heights); the named planes first
SCENARIOS = {
    "two_boxes": lambda: (tsh.two_boxes(), Plane.xy(0), 0.0625, [-2.25, -1.75, -0.5, 0.125, 0.9375, 1.5]),
    "diagonal": lambda: (tso.diagonal(), Plane.xy(0), 0.25, [-0.25, 0.125, 0.375]),
    "bar_64_9": lambda: (tsh.bar(64, 9, 0.125), Plane.xy(0), 0.125, [-0.25, 0.3125]),
    "grid_64": lambda: (tsh.grid_64_with_hidden(), Plane.xz(0), 0.25, [-1.0, -0.6, 0.1]),
    "coincident": lambda: (tsh.coincident(), Plane.xy(0), 0.05, [-0.3, 0.02, 0.3]),
    "boxes_and_ball": _boxes_and_ball,
    "far": _far,
}
SCENARIOS.update(heavy_instances.layer_scenarios())      # parts with wide register files among light ones, three layers
NAMED = ["two_boxes", "diagonal", "bar_64_9", "grid_64"]


def named_plane(plane, height):
    """The named plane that layer `height` of the named base plane is: what the per-plane function is given."""
    axis = int(numpy.argmax(numpy.abs(plane.normal)))
    return {2: Plane.xy, 1: Plane.xz, 0: Plane.yz}[axis](float(plane.origin[axis]) + float(plane.normal[axis]) * float(height))


@functools.lru_cache(maxsize=None)
def scenario(name):
    """(assembly, plane, resolution, heights, its reference stack)"""
    asm, plane, resolution, heights = SCENARIOS[name]()
    return asm, plane, resolution, heights, reference_layers(asm, plane, resolution, heights)


@functools.lru_cache(maxsize=None)
def traversal(name, cull=True):
    asm, plane, resolution, heights, ref = scenario(name)
    return reference_layer_traversal(asm, plane, resolution, heights, cull)


# ---- 70 000 layers of one sample --------------------------------------------------------------------------------------

SPECK_LAYERS = 70000


def speck_heights():
    return (numpy.arange(SPECK_LAYERS, dtype=numpy.float64) - 35000) * 2.0 ** -17


@functools.lru_cache(maxsize=None)
def speck_reference():
    """(assembly, plane, resolution, heights, sorted records, evaluations) of tso.speck() on 70 000 layers, over all layers
    at once: the 3 x 3 ringed samples of every layer from the oracle, one inside sample in the middle, so four squares of
    one inside corner each; the segments of those four squares from `square_segments`, their crossings in NumPy float32."""
    asm, plane, resolution, heights = tso.speck(), Plane.xy(0), 0.125, speck_heights()
    assert (heights.astype(numpy.float32).astype(numpy.float64) == heights).all()          # exact in float32
    instances = _instance_cells.visible(asm, resolution)
    corner, step, dims, first, projected = lattice(instances, plane, resolution)
    assert dims.tolist() == [1, 1]
    o, u, v, normal = (x.astype(numpy.float64) for x in (plane.origin, plane.u, plane.v, plane.normal))
    origins = (o[None] + normal[None] * heights[:, None]).astype(numpy.float32)
    corners = (origins.astype(numpy.float64) + u * first[0] + v * first[1]).astype(numpy.float32)
    index = numpy.arange(-1, 2, dtype=numpy.float32)
    a, b = (step * index)[None, None, :, None], (step * index)[None, :, None, None]
    points = ((corners[:, None, None, :] + plane.u * a) + plane.v * b).astype(numpy.float32)           # [layer, t, s, 3]
    assert points.dtype == numpy.float32 and numpy.array_equal(points[7], sample_positions(plane, corners[7], step, index, index))
    w = oracle.evaluate_points(nodes.make_program(instances[0].shape()), points.reshape(-1, 3))[:, 3].reshape(SPECK_LAYERS, 3, 3)
    inside = w < 0
    assert inside[:, 1, 1].all() and inside.sum() == SPECK_LAYERS
    records = numpy.zeros((SPECK_LAYERS, 4), dtype=LAYER_SEGMENT)
    layer = numpy.arange(SPECK_LAYERS)
    for n, (sb, sa) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):          # the squares in the order (b, a)
        corner_w = [w[:, sb + (c >> 1), sa + (c & 1)] for c in range(4)]
        (e, f), = tso.square_segments([bool(v[0] < 0) for v in corner_w])
        with numpy.errstate(all="ignore"):
            t = {g: (corner_w[p] / (corner_w[p] - corner_w[q])).astype(numpy.float32) for g, (p, q) in tso.EDGE_ENDS.items()}
        assert all(x.dtype == numpy.float32 for x in corner_w) and not numpy.isnan(t[e]).any() and not numpy.isnan(t[f]).any()
        records[:, n]["a"], records[:, n]["b"] = sa, sb
        records[:, n]["word"] = e * 256 + f * 1024 + layer * 4096
        records[:, n]["t_from"], records[:, n]["t_to"] = t[e], t[f]
    # per layer: the top tile evaluates its one child that exists, the finest tile its 3 x 3 samples
    return asm, plane, resolution, heights, records.reshape(-1), SPECK_LAYERS * (1 + 9)
