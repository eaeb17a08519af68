"""The scenarios of the assembly mesh tests (test_assembly_meshes_host.py shows on the CPU that each holds what it is there
for; test_gpu_assembly_meshes.py runs them on the device) and their CPU reference.

The REFERENCE MESH is written from the definitions in codecad_amd/assembly_meshes.py: every instance's tape evaluated by the
oracle (`oracle.evaluate_points`) at the float32 positions of the ringed samples, inside = w < 0, the case of a cube from
its eight corners, crossings t = w_p / (w_p - w_q) in NumPy float32 from the end with the lower lattice index (0.5 for a
NaN).  The case table is DERIVED here by importing tools/gen_mc_table.py and calling its construction, not parsed from the
header the kernel includes.  The REFERENCE TRAVERSAL applies the windows of cubes, the top cells and the keep rule level by
level, the centres of the children in float32 operation for operation as the kernels compute them.
"""
import collections
import concurrent.futures
import functools
import importlib.util
import os

import numpy

import codecad_amd as cc
from codecad_amd import shapes, nodes, _instance_cells
from codecad_amd.assembly_meshes import (TRIANGLE, CORNERS, EDGES, Meshes, sort_triangles, cube_windows, radius, top_cells,
                                          first_capacity)
import oracle

import assembly_mass_scenes as mass_scenes
import heavy_instances
import test_section_host as tsh
from test_gpu_interference import _gear_train
from test_section_outlines_host import diagonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def case_table():
    """[case] -> [(e0, e1, e2)], from the derivation of tools/gen_mc_table.py."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert tuple(gen.CORNERS) == CORNERS and tuple(gen.EDGES) == EDGES
    return [[tuple(int(e) for e in tri) for tri in tris] for tris in gen.build()]


# ---- the reference mesh -----------------------------------------------------------------------------------------------

Reference = collections.namedtuple("Reference", "instances corner step dims w cases triangles counts")


def evaluate(tape, points):
    """The distance of the oracle at float32 points (m, 3), in a few threads (the oracle's library releases the GIL)."""
    points = numpy.ascontiguousarray(points, dtype=numpy.float32).reshape(-1, 3)
    if len(points) < 1 << 15:
        return oracle.evaluate_points(tape, points)[:, 3].copy()
    parts = numpy.array_split(points, 8)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        return numpy.concatenate(list(pool.map(lambda p: oracle.evaluate_points(tape, p)[:, 3], parts)))


def ringed_axes(corner, step, dims):
    """Per axis the float32 coordinates of the samples with the shifted indices 0 .. dims + 1."""
    corner, step = numpy.asarray(corner, dtype=numpy.float32), numpy.float32(step)
    axes = [corner[a] + step * (numpy.arange(int(dims[a]) + 2).astype(numpy.float32) - numpy.float32(1)) for a in range(3)]
    assert all(x.dtype == numpy.float32 for x in axes)
    return axes


def ringed_values(instances, corner, step, dims):
    """float32 w[k, sx, sy, sz] at the ringed samples."""
    xs, ys, zs = ringed_axes(corner, step, dims)
    points = numpy.stack(numpy.meshgrid(xs, ys, zs, indexing="ij"), axis=-1)
    assert points.dtype == numpy.float32
    w = numpy.zeros((len(instances),) + points.shape[:3], dtype=numpy.float32)
    for k, inst in enumerate(instances):
        w[k] = evaluate(nodes.make_program(inst.shape()), points.reshape(-1, 3)).reshape(points.shape[:3])
    return w


def cube_cases(inside):
    """uint8 case of every cube of a lattice of inside bits [sx, sy, sz]: bit m from the corner at CORNERS[m]."""
    nx, ny, nz = (d - 1 for d in inside.shape)
    case = numpy.zeros((nx, ny, nz), dtype=numpy.uint8)
    for m, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:dx + nx, dy:dy + ny, dz:dz + nz].astype(numpy.uint8) << numpy.uint8(m)
    return case


def crossing(wp, wq):
    wp, wq = numpy.asarray(wp, dtype=numpy.float32), numpy.asarray(wq, dtype=numpy.float32)
    with numpy.errstate(all="ignore"):
        t = wp / (wp - wq)
    assert t.dtype == numpy.float32
    return numpy.where(numpy.isnan(t), numpy.float32(0.5), t)


def triangles_of(w):
    """(the sorted TRIANGLE records of the distances w[k, sx, sy, sz] at the ringed samples, the cases [k, a, b, c])."""
    table = case_table()
    corners = numpy.array(CORNERS)
    found, cases = [], []
    for k in range(len(w)):
        case = cube_cases(w[k] < 0)                               # (a NaN is not inside)
        cases.append(case)
        for value in numpy.unique(case):
            tris = table[int(value)]
            if not tris:
                continue
            at = numpy.argwhere(case == value)                    # [m, 3]: the cubes of this case
            t = {}
            for e in {e for tri in tris for e in tri}:
                p, q = (corners[c] for c in EDGES[e])
                if (q < p).any():
                    p, q = q, p                                   # from the end with the lower lattice index
                wp, wq = (w[k][tuple((at + c).T)] for c in (p, q))
                assert ((wp < 0) != (wq < 0)).all()               # the table lists crossed edges only
                t[e] = crossing(wp, wq)
            for which, tri in enumerate(tris):
                rec = numpy.zeros(len(at), dtype=TRIANGLE)
                rec["a"], rec["b"], rec["c"] = at.T
                rec["k"], rec["which"], rec["case"] = k, which, value
                for v, e in enumerate(tri):
                    rec["e"][:, v] = e
                    rec["t"][:, v] = t[e]
                found.append(rec)
    records = numpy.concatenate(found) if found else numpy.zeros(0, dtype=TRIANGLE)
    return sort_triangles(records), (numpy.stack(cases) if cases else numpy.zeros((0, 1, 1, 1), numpy.uint8))


def reference_meshes(instances, corner, step, dims):
    w = ringed_values(instances, corner, step, dims)
    triangles, cases = triangles_of(w)
    counts = numpy.bincount(triangles["k"], minlength=len(instances)).astype(numpy.int64)
    return Reference(instances, corner, step, dims, w, cases, triangles, counts)


def meshes_of(ref):
    """The Meshes a device run must give, from the reference (evaluations and runs left 0)."""
    named = [_instance_cells.Instance(i.name, i) for i in ref.instances]
    return Meshes(named, ref.corner, ref.step, ref.dims, ref.triangles, ref.counts, 0, 0)


# ---- the reference traversal ------------------------------------------------------------------------------------------

Traversal = collections.namedtuple("Traversal", "rows evaluations dropped_outside dropped_inside")


def reference_traversal(instances, corner, step, dims, cull=True, side=None):
    """What assembly_meshes.py and csrc/instance_mesh.hip do, in NumPy over the oracle -> the rows {(a0, b0, c0, mask)} of every
    level from the top one to the finest, the evaluations of all levels, and how many candidates a level dropped for
    w >= r and for w <= -r."""
    corner, step = numpy.asarray(corner, dtype=numpy.float32), numpy.float32(step)
    n = len(instances)
    if n == 0:
        return Traversal([[]], 0, 0, 0)
    wins = cube_windows(_instance_cells.windows(instances, corner, float(step), dims))
    cubes = numpy.asarray(dims, dtype=numpy.int64) + 1
    if side is None:
        side = _instance_cells.top_side(cubes) if cull else 4
    tapes = [nodes.make_program(i.shape()) for i in instances]
    top = top_cells(wins, cubes, side, everywhere=not cull)
    origin = numpy.stack([top[:, 0] & 0xffff, top[:, 0] >> 16, top[:, 1]], axis=-1).astype(numpy.int64).reshape(-1, 3)
    cand = top[:, 2].astype(numpy.uint64) | (top[:, 3].astype(numpy.uint64) << numpy.uint64(32))

    def listed():
        return sorted((int(x), int(y), int(z), int(m)) for (x, y, z), m in zip(origin.tolist(), cand.tolist()))

    rows, evaluations, outside, inside = [listed()], 0, 0, 0
    if len(top) == 0:
        return Traversal(rows, 0, 0, 0)                           # nothing is launched
    lanes = numpy.arange(64)
    offsets = numpy.stack([lanes >> 4, (lanes >> 2) & 3, lanes & 3], axis=-1)     # lane = 16 x + 4 y + z
    one = numpy.uint64(1)
    while side > 4:
        child = side // 4
        r = radius(child, step)
        first = origin[:, None, :] + offsets[None, :, :] * child                 # [m, 64, 3]
        live = (first < cubes).all(axis=-1)
        h = numpy.float32(0.5) * numpy.float32(child)
        centre = corner + step * ((first.astype(numpy.float32) + h) - numpy.float32(1))      # float32, one rounding per operation
        assert centre.dtype == numpy.float32
        keep = numpy.zeros(live.shape, dtype=numpy.uint64)
        for k in range(n):
            bit = one << numpy.uint64(k)
            at = ((cand & bit) != 0)[:, None] & live
            if not at.any():
                continue
            values = evaluate(tapes[k], centre[at])
            evaluations += len(values)
            lo = first[at]
            reach = ((lo <= wins[k, 1]) & (lo + child - 1 >= wins[k, 0])).all(axis=-1)
            out = reach & (values >= r)
            inn = reach & ~out & (values <= -r)
            outside, inside = outside + int(out.sum()), inside + int(inn.sum())
            keep[at] |= numpy.where(reach & ~out & ~inn, bit, numpy.uint64(0))    # (a NaN keeps its candidate)
        going = live & (keep != 0)
        origin, cand, side = first[going], keep[going], child
        rows.append(listed())
    for x0, y0, z0, mask in rows[-1]:        # a finest cell: those of its 5^3 samples that exist
        evaluations += int(numpy.prod([min(v + 4, int(c)) - v + 1 for v, c in zip((x0, y0, z0), cubes)])) * bin(mask).count("1")
    return Traversal(rows, int(evaluations), outside, inside)


def dense_evaluations(dims, n):
    """The evaluations of cull=False in closed form: every axis has its cubes + 1 samples, and the samples between two cells
    are evaluated by both."""
    cubes = [int(d) + 1 for d in dims]
    return n * int(numpy.prod([c + -(-c // 4) for c in cubes]))


def triangles_reached(ref, leaf_rows):
    """The reference's triangles in the cubes and of the candidates of the finest rows: what the traversal emits."""
    masks = {(a0, b0, c0): mask for a0, b0, c0, mask in leaf_rows}
    s = ref.triangles
    keep = [bool(masks.get((int(a) & ~3, int(b) & ~3, int(c) & ~3), 0) >> int(k) & 1) for a, b, c, k in zip(s["a"], s["b"], s["c"], s["k"])]
    return s[numpy.array(keep, dtype=bool)] if len(s) else s


# ---- the properties of a welded mesh that depend on no table ----------------------------------------------------------

def directed_edges(triangles):
    t = numpy.asarray(triangles, dtype=numpy.int64).reshape(-1, 3)
    return numpy.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_and_oriented(triangles):
    """Every directed edge of the mesh occurs once, and so does its reverse."""
    e = directed_edges(triangles)
    if len(e) == 0:
        return True
    stride = int(e.max()) + 1
    forward, backward = e[:, 0] * stride + e[:, 1], e[:, 1] * stride + e[:, 0]
    return len(numpy.unique(forward)) == len(forward) and numpy.array_equal(numpy.sort(forward), numpy.sort(backward))


def signed_volume(vertices, triangles):
    """The divergence theorem in float64: the sum of det(p0, p1, p2) / 6 about the mesh's first vertex."""
    if len(triangles) == 0:
        return 0.0
    p = numpy.asarray(vertices, dtype=numpy.float64)[numpy.asarray(triangles, dtype=numpy.int64)] - numpy.asarray(vertices[0], dtype=numpy.float64)
    return float(numpy.einsum("ij,ij->i", p[:, 0], numpy.cross(p[:, 1], p[:, 2])).sum() / 6)


def euler_characteristic(vertices, triangles):
    e = directed_edges(triangles)
    return len(vertices) - len(numpy.unique(numpy.sort(e, axis=1), axis=0)) + len(triangles)


def components(vertices, triangles):
    """The number of connected components of the welded mesh."""
    parent = list(range(len(vertices)))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in directed_edges(triangles).tolist():
        parent[find(a)] = find(b)
    return len({find(v) for v in range(len(vertices))})


def check_mesh_properties(meshes, ref):
    """The table-free properties of every instance's welded mesh against the reference's own values -> [(vertices,
    triangles)]: closed and consistently oriented; the signed volume positive where the part has an inside sample; and
    |volume - step^3 N| <= step^3 M, N the inside samples and M the cubes with a mixed case (the two solids differ inside
    mixed cubes only)."""
    cell = float(ref.step) ** 3
    out = []
    for k in range(len(ref.instances)):
        vertices, triangles = meshes.mesh(k)
        assert vertices.dtype == numpy.float64 and triangles.dtype == numpy.uint32 and len(triangles) == ref.counts[k]
        assert is_closed_and_oriented(triangles), k
        volume = signed_volume(vertices, triangles)
        inside, mixed = int((ref.w[k] < 0).sum()), int(((ref.cases[k] != 0) & (ref.cases[k] != 255)).sum())
        if inside:
            assert volume > 0, k
        assert abs(volume - cell * inside) <= cell * mixed, (k, volume, cell * inside, cell * mixed)
        out.append((vertices, triangles))
    return out


# ---- the scenarios ----------------------------------------------------------------------------------------------------

Scene = collections.namedtuple("Scene", "build resolution side", defaults=(None,))
Scene.__doc__ = """`build()` -> the assembly meshed at `resolution`; `side`: the top side forced on it (None: what top_side() gives)."""

FAR_RESOLUTION = 0.0625


def _ball():
    return cc.assembly("ball", [shapes.sphere(r=1).make_part("ball"), shapes.box(1.5, 1.0, 0.75).make_part("box").translated(2.5, 0.1, 0.2)])


def _torus():
    return cc.assembly("torus", [shapes.circle(r=0.4).translated_x(1).revolved().make_part("torus")])


def _box_with_hole():
    return cc.assembly("holed", [(shapes.box(2, 2, 1) - shapes.cylinder(h=2, d=0.9)).make_part("holed")])


def _rims_4k1():
    """12 x 8 x 4 samples: 13 x 9 x 5 cubes, the last cell of every axis one cube wide."""
    return cc.assembly("rims", [shapes.box(1.5, 1.0, 0.5).make_part("block")])


def _speck():
    return cc.assembly("speck", [shapes.box(0.1, 0.1, 0.1).make_part("speck")])


def _dust():
    """Thinner than a step and between the samples: nothing is inside."""
    return cc.assembly("dust", [shapes.box(0.5, 0.5, 0.02).make_part("dust").translated_z(0.05)])


def _coincident():
    peg = (shapes.cylinder(h=1.1, d=0.8) - shapes.sphere(r=0.3).translated_x(0.4)).make_part("peg")
    return cc.assembly("twice", [peg.translated_x(0.3), peg.translated_x(0.3), shapes.box(1, 1, 1).make_part("block").translated_x(1.2)])


def _strict_notch():
    """The dyadic construction with a concave edge: a lattice of step 2^-3 with corner = -0.5 exactly, and a block whose
    faces AND whose notch's faces lie on samples.  A sample on the concave edge is outside and has two inside neighbours in
    one cube: both crossings land on it, and the triangles between them have no area."""
    outer = shapes.box(1.125).make_part("outer")
    notched = (shapes.box(1) - shapes.box(0.5, 0.5, 2).translated(0.25, 0.25, 0)).make_part("notched")
    return cc.assembly("notch", [outer, notched])


SCENES = {
    "ball": Scene(_ball, 0.2),
    "torus": Scene(_torus, 0.125),
    "box_with_hole": Scene(_box_with_hole, 0.125),
    "rims": Scene(mass_scenes._rims, 0.125),
    "rims_4k1": Scene(_rims_4k1, 0.125),
    "zigzag": Scene(diagonal, 0.25),
    "speck": Scene(_speck, 0.125),
    "dust": Scene(_dust, 0.125),
    "coincident": Scene(_coincident, 0.125),
    "solids64": Scene(functools.partial(mass_scenes._solids, 64), 0.07),
    "far": Scene(functools.partial(tsh.far_assembly, FAR_RESOLUTION), FAR_RESOLUTION),
    "strict": Scene(mass_scenes._strict, 0.0625),
    "strict_notch": Scene(_strict_notch, 0.125),
    "coarse_64": Scene(mass_scenes._coarse, 0.0625, 64),
    "coarse_256": Scene(mass_scenes._coarse, 0.0625, 256),
    "gears": Scene(_gear_train, 0.3),
}
SCENES.update(heavy_instances.mass_scenes(Scene))        # parts with wide register files among light ones
forced_top_cells = mass_scenes.forced_top_cells


@functools.lru_cache(maxsize=None)
def scene(name):
    """(assembly, resolution, visible instances, corner, step, dims) of a scenario."""
    sc = SCENES[name]
    asm = sc.build()
    instances = _instance_cells.visible(asm, sc.resolution)
    corner, step, dims = _instance_cells.checked_lattice(instances, sc.resolution)
    return asm, sc.resolution, instances, corner, step, dims


@functools.lru_cache(maxsize=None)
def reference(name):
    """The Reference of a scenario, computed once and shared; nobody changes it."""
    if name == "coarse_256":
        return reference("coarse_64")                             # the same assembly on the same lattice
    asm, resolution, instances, corner, step, dims = scene(name)
    return reference_meshes(instances, corner, step, dims)


@functools.lru_cache(maxsize=None)
def traversal(name, cull=True):
    asm, resolution, instances, corner, step, dims = scene(name)
    return reference_traversal(instances, corner, step, dims, cull, SCENES[name].side if cull else None)


def default_capacity(name):
    """The first capacity assembly_meshes() gives the triangle buffer of a scenario."""
    asm, resolution, instances, corner, step, dims = scene(name)
    return first_capacity(cube_windows(_instance_cells.windows(instances, corner, float(step), dims)))
