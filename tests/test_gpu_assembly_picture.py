"""The picture of an assembly on the device (codecad_amd/rendering/assembly_picture.py, csrc/instance_rays.hip): one
instance is the existing ray caster byte for byte; ids and depth against the oracle, point by point; skipping changes
nothing; the picture is the union's; colours; 64 instances."""
import math
import random

import numpy
import pytest

import codecad_amd as cc
from codecad_amd import shapes, nodes, examples
from codecad_amd.rendering import assembly_picture as ap, ray_caster, pictures
from codecad_amd.rendering.ray_caster import RenderOptions
import oracle
import random_trees
import shapes_zoo

pytestmark = pytest.mark.gpu

SIZE = (160, 120)


# ---- scenes (the gear train and the random assemblies of test_gpu_interference.py) -----------------------------------
def _gear_train():
    m, h = 1.0, 4.0
    sun = shapes.gears.InvoluteGear(12, m).extruded(h).make_part("sun")
    planet = shapes.gears.InvoluteGear(9, m).extruded(h).make_part("planet")
    pin = shapes.cylinder(h=h + 4, d=2.0).make_part("pin")
    carrier = (shapes.cylinder(h=2, d=30) - shapes.cylinder(h=3, d=6)).make_part("carrier")
    orbit = (12 + 9) * m / 2
    instances = [sun]
    for k in range(3):
        instances.append(planet.rotated_z(7 + 40 * k).translated_x(orbit).rotated_z(120 * k))
    for k in range(3):
        instances.append(pin.translated(orbit, 0, 1).rotated_z(120 * k))
    instances.append(carrier.translated_z(h / 2 + 1.5))
    return cc.assembly("planetary", instances).rotated_x(-55)     # (the gears' side tilted towards the camera, not edge on)


def _safe_random_shape(rng):
    """A random tree whose distance is a lower bound (no repetition, no twist) and whose box is finite and not huge."""
    while True:
        s = random_trees.random_3d(rng, 2)
        names = {ins.name for ins in nodes.make_schedule(s)[1]}
        box = s.bounding_box()
        if names & {"repetition", "circular_repetition_to", "twist_revolution_to"}:
            continue
        if not all(math.isfinite(v) for v in tuple(box.a) + tuple(box.b)) or max(box.size()) > 8:
            continue
        return s


def _random_assembly(seed, k, blended):
    rng = random.Random(seed)
    parts = [_safe_random_shape(rng).make_part("p%d" % i) for i in range(max(2, k // 3))]
    if blended:
        parts.append(shapes.union([shapes.box(2, 1, 1), shapes.sphere(1.5).translated_x(1)], r=0.3).make_part("blend"))

    def place(inst):
        axis = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.1, 1))
        return inst.rotated(axis, rng.uniform(-180, 180)).translated(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3))

    inner = cc.assembly("inner", [place(rng.choice(parts)) for _ in range(3)])
    instances = [place(inner)] + [place(rng.choice(parts)) for _ in range(k - 3)]
    instances.append(place(rng.choice(parts)).hidden())
    return cc.assembly("random", instances)


def _grid(n):
    """n small distinct solids on a grid in the x-z plane (the camera looks along +y), none touching."""
    parts = []
    for i in range(n):
        kind, s = i % 4, 0.5 + 0.4 * ((i * 7) % 11) / 11
        solid = (shapes.sphere(s) if kind == 0 else shapes.box(1.6 * s, 1.2 * s, 1.4 * s) if kind == 1 else
                 shapes.cylinder(h=1.5 * s, d=1.5 * s) if kind == 2 else shapes.sphere(s) - shapes.box(s, 3 * s, s))
        parts.append(solid.make_part("solid%d" % i).rotated((1, i % 3, 2), 13 * i).translated(2.5 * (i % 8), 0.3 * (i % 5), 2.5 * (i // 8)))
    return cc.assembly("grid", parts)


SCENES = {
    "gear_train": _gear_train,
    "random_4": lambda: _random_assembly(1, 4, False),
    "random_9": lambda: _random_assembly(2, 9, False),
    "random_12_blended": lambda: _random_assembly(5, 12, True),
    "grid_64": lambda: _grid(64),
}
_cache = {}


def scene(name):
    """(assembly, its picture with skipping, its picture without), rendered once per session"""
    if name not in _cache:
        asm = SCENES[name]()
        _cache[name] = (asm, ap.render_assembly_pixels(asm, SIZE, colors="parts", count=True),
                        ap.render_assembly_pixels(asm, SIZE, colors="parts", skip=False, count=True))
    return _cache[name]


# ---- (a) one instance = the existing ray caster ----------------------------------------------------------------------
def _single(name):
    if name == "sponge":
        return cc.assembly("one", [examples.sponge(2).make_part("sponge")])
    if name == "placed":
        part = shapes_zoo.shapes_3d["csg_thing"].make_part("thing")
        return cc.assembly("one", [part.rotated((1, 2, 3), 35).translated(3, -1, 2)]).translated(8, -4, 2)
    return cc.assembly("one", [shapes_zoo.shapes_3d[name].make_part(name)])


@pytest.mark.parametrize("name", ["csg_thing", "torus", "mirror_3d", "nested_transformations", "revolved_pentagon", "sponge", "placed"])
def test_one_instance_is_the_ray_caster_byte_for_byte(hip, name):
    asm = _single(name)
    united = asm.shape()
    camera = ray_caster.get_camera_params(united.bounding_box(), SIZE, None)
    for options in (RenderOptions.no_flags, RenderOptions.false_color, RenderOptions.zebra):
        got = ap.render_assembly_pixels(asm, SIZE, colors=None, options=options)
        want = ray_caster.render(united, *camera, size=SIZE, options=options)        # the interpreter: nothing was specialised
        differing = numpy.count_nonzero(numpy.any(got.pixels != want, axis=-1))
        assert differing == 0, "%s, options %d: %d of %d pixels differ" % (name, int(options), differing, SIZE[0] * SIZE[1])
        assert got.pixels.shape == (SIZE[1], SIZE[0], 3) and got.part_ids.shape == got.depth.shape == (SIZE[1], SIZE[0])
        assert set(numpy.unique(got.part_ids)) <= {-1, 0} and (got.part_ids == 0).any()
    assert numpy.array_equal(ap.render_assembly_pixels(asm, SIZE).pixels, pictures.render_pixels(united, SIZE))


# ---- (b) ids and depth against the oracle ------------------------------------------------------------------------------
def _points(picture):
    """The end of every primary ray, origin + depth * direction, in the kernel's float32 arithmetic -> (h, w, 3)."""
    f = numpy.float32
    a = picture.arguments
    origin, forward, up, right = (numpy.array(list(a[k])[:3], dtype=f) for k in ("origin", "forward", "up", "right"))
    h, w = picture.part_ids.shape
    filmx = (numpy.arange(w, dtype=f) - f(w - 1) / f(2))[None, :, None]
    filmy = (numpy.arange(h, dtype=f) - f(h - 1) / f(2))[:, None, None]
    d = (forward + right * filmx) - up * filmy
    d = d * (f(1) / numpy.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None]
    with numpy.errstate(invalid="ignore"):
        return origin + d * picture.depth[..., None]


def check_ids_and_depth(picture):
    a = picture.arguments
    tol = float(numpy.float32(a["pixel_tolerance"]))
    ids, depth = picture.part_ids, picture.depth
    n = len(picture.instances)
    assert ids.min() >= -1 and ids.max() < n
    assert numpy.isinf(depth[ids < 0]).all() and (depth[ids < 0] > 0).all()
    hit = ids >= 0
    assert hit.any() and numpy.isfinite(depth[hit]).all() and (depth[hit] > 0).all()
    points = _points(picture)[hit]
    w = numpy.stack([oracle.evaluate_points(nodes.make_program(i.instance.shape()), points)[:, 3] for i in picture.instances]).astype(numpy.float64)
    own = w[ids[hit], numpy.arange(points.shape[0])]
    d = depth[hit].astype(numpy.float64)
    # the float32 rounding of origin + depth * direction: a few ulp of its magnitude, on top of the bounds
    rounding = 4 * 2.0 ** -23 * (numpy.abs(numpy.array(list(a["origin"])[:3], dtype=numpy.float64)).max() + d)
    surface = numpy.abs(own) - (3 * tol * d + rounding)
    nearest = own - (w.min(axis=0) + 4 * tol * d + rounding)
    print("pixels hit %d of %d; worst |w_k| - bound %.3g, worst w_k - min_j w_j - bound %.3g" % (hit.sum(), hit.size, surface.max(), nearest.max()))
    assert (surface <= 0).all(), "%d pixels off the surface of their part" % (surface > 0).sum()
    assert (nearest <= 0).all(), "%d pixels whose part is not the nearest" % (nearest > 0).sum()
    return hit


@pytest.mark.parametrize("name", ["gear_train", "random_4", "random_9", "random_12_blended"])
def test_ids_and_depth_against_the_oracle(hip, name):
    asm, picture, _ = scene(name)
    assert [i.name for i in picture.instances] == [i.name for i in asm.all_instances() if i.visible]
    hit = check_ids_and_depth(picture)
    assert len(numpy.unique(picture.part_ids[hit])) >= 3                 # several parts are in the picture
    y, x = numpy.argwhere(hit)[0]
    assert picture.part_at(x, y) is picture.instances[picture.part_ids[y, x]]
    y, x = numpy.argwhere(~hit)[0]
    assert picture.part_at(x, y) is None


# ---- (c) skipping changes nothing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gear_train", "random_4", "random_9", "random_12_blended"])
def test_skipping_changes_nothing(hip, name):
    _, skipped, full = scene(name)
    assert numpy.array_equal(skipped.pixels, full.pixels)
    assert numpy.array_equal(skipped.part_ids, full.part_ids)
    assert numpy.array_equal(skipped.depth.view(numpy.uint32), full.depth.view(numpy.uint32))
    run, asked = skipped.evaluations
    print("%s: %d of %d instance programs run with skipping (%.1f %%); %d without" % (name, run, asked, 100.0 * run / asked, full.evaluations[0]))
    assert full.evaluations[0] == full.evaluations[1] and 0 < run <= asked
    for options in (RenderOptions.false_color, RenderOptions.zebra):
        asm = scene(name)[0]
        a, b = (ap.render_assembly_pixels(asm, SIZE, options=options, skip=s) for s in (True, False))
        assert numpy.array_equal(a.pixels, b.pixels) and numpy.array_equal(a.part_ids, b.part_ids)
        assert numpy.array_equal(a.depth.view(numpy.uint32), b.depth.view(numpy.uint32))


# ---- (d) the assembly's picture is the union's -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gear_train", "random_4", "random_9", "random_12_blended"])
def test_the_picture_is_the_unions(hip, name):
    asm = scene(name)[0]
    got = ap.render_assembly_pixels(asm, SIZE, colors=None).pixels
    want = pictures.render_pixels(asm.shape(), SIZE)
    mse = float(numpy.mean((got.astype(numpy.float32) - want.astype(numpy.float32)) ** 2)) / 255 ** 2
    differing = numpy.count_nonzero(numpy.any(got != want, axis=-1))
    print("%s: %d of %d pixels differ from the union's picture, mean squared error %.3g" % (name, differing, SIZE[0] * SIZE[1], mse))
    assert mse <= 1e-3


# ---- (e) colours -----------------------------------------------------------------------------------------------------------
def test_colours(hip):
    asm, parts_picture, _ = scene("gear_train")
    n = len(parts_picture.instances)
    k = 1                                                                  # a planet
    red = [(0.2, 0.4, 0.9)] * n
    red[k] = (1, 0, 0)
    picture = ap.render_assembly_pixels(asm, SIZE, colors=red)
    assert numpy.array_equal(picture.part_ids, parts_picture.part_ids)
    mine = picture.part_ids == k
    assert mine.any()
    r, g, b = (picture.pixels[..., c][mine].astype(int) for c in range(3))
    assert (g == b).all() and (r >= g).all() and (r > g).any()
    nothing = picture.part_ids == -1
    assert nothing.any() and numpy.array_equal(picture.pixels[nothing], parts_picture.pixels[nothing])
    # two palettes that differ in one part's colour differ on that part's pixels only ("parts": the three planets are one part)
    base = [tuple(c) for c in parts_picture.colors]
    assert base[1] == base[2] == base[3] and base[0] != base[1]
    changed = list(base)
    changed[k] = (0.0, 0.2, 1.0)
    other = ap.render_assembly_pixels(asm, SIZE, colors=changed)
    differs = numpy.any(other.pixels != parts_picture.pixels, axis=-1)
    assert differs.any() and not differs[~mine].any()
    named = ap.render_assembly_pixels(asm, SIZE, colors={"planet": (0.0, 0.2, 1.0)})
    planets = numpy.isin(named.part_ids, [1, 2, 3])
    plain = ap.render_assembly_pixels(asm, SIZE)
    assert numpy.array_equal(named.pixels[~planets], plain.pixels[~planets]) and numpy.any(named.pixels[planets] != plain.pixels[planets])


# ---- (f) many instances --------------------------------------------------------------------------------------------------
def test_sixty_four_instances(hip):
    asm, skipped, full = scene("grid_64")
    assert len(skipped.instances) == 64
    hit = check_ids_and_depth(skipped)
    assert len(numpy.unique(skipped.part_ids[hit])) == 64                 # every solid is seen
    assert numpy.array_equal(skipped.pixels, full.pixels) and numpy.array_equal(skipped.part_ids, full.part_ids)
    assert numpy.array_equal(skipped.depth.view(numpy.uint32), full.depth.view(numpy.uint32))
    run, asked = skipped.evaluations
    print("grid of 64: %d of %d instance programs run with skipping (%.1f %%)" % (run, asked, 100.0 * run / asked))
    with pytest.raises(ValueError, match="64"):
        ap.render_assembly_pixels(_grid(65), SIZE)


def test_the_reference_size_once(hip):
    asm = scene("gear_train")[0]
    picture = ap.render_assembly_pixels(asm, colors="parts")
    assert picture.pixels.shape == (768, 1024, 3) and picture.part_ids.shape == (768, 1024)
    assert len(numpy.unique(picture.part_ids)) >= 5 and picture.part_ids.min() == -1 and picture.part_ids.max() <= 7
