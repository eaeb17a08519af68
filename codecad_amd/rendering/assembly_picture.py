"""Sphere-traced picture of an ASSEMBLY with a colour per part, a part-id map and a depth map.

`pictures.render_image` takes one shape, so an assembly rendered through it is `asm.shape()`: one union, one colour.
Here every visible instance keeps its own tape (as in `interference()`), and the ray caster walks the instance table
(csrc/instance_rays.hip).  With `e_k(p)` the float4 the interpreter gives for instance k at p, the field is

    F(p).w = min_k e_k(p).w,    F(p).xyz = e_m(p).xyz,    id(p) = m, the LOWEST index with e_m(p).w == F(p).w:

what the union of the instances computes, with the one freedom a union chain has -- which of two exactly equal
operands gives the direction -- fixed by index.  The kernel is the ray caster of `ray_caster.render` around that field,
so with one hue for every part the picture is the union's (up to such ties).  An instance that provably cannot be the
nearest at a sample is not evaluated there (`skip`); that assumes what `subdivision()` and `interference()` assume, a
distance with Lipschitz constant at most 1 -- shapes from `shapes.unsafe` may break it here as they do there --, and then
changes no byte of the result.

Camera and scene scalars are those of `asm.shape()`: a picture of the assembly and a picture of its union share a camera.
The instances are the visible ones in `all_instances()` order, placed by the assembly's own transform, at most 64, 3D.
"""
import collections

import numpy

from .. import _instance_cells as cells
from .. import hip_util
from ..hip_util import manager as hip_manager
from . import ray_caster
from .ray_caster import RenderOptions
from .pictures import DEFAULT_SIZE

DEFAULT_HUE = (0.7, 1.0, 0.0)           # the flat colour of ray_caster.render (kernels.hpp default_hue)
# colors="parts": one hue per BOM item in order of first appearance, cycling
PALETTE = (
    (0.7, 1.0, 0.0), (1.0, 0.35, 0.1), (0.1, 0.55, 1.0), (1.0, 0.8, 0.0), (0.7, 0.2, 1.0), (0.0, 0.85, 0.6),
    (1.0, 0.2, 0.5), (0.45, 0.45, 0.5), (0.55, 0.3, 0.1), (0.3, 0.9, 1.0), (0.9, 0.6, 0.9), (0.2, 0.6, 0.2),
)


class AssemblyPicture(collections.namedtuple("AssemblyPicture", "pixels part_ids depth instances colors camera arguments evaluations")):
    """`pixels`: uint8 (height, width, 3); `part_ids`: int32 (height, width), the index into `instances` of the part the
    primary ray hit, -1 where it hit none (background, floor); `depth`: float32 (height, width), the distance along the
    primary ray where it hit, +inf where not; `instances`: the visible instances, as Instance(name, instance) like
    interference()'s report; `colors`: float32 (n, 3), the hue of each; `camera`: (origin, direction, up, focal_length);
    `arguments`: the kernel's camera frame and scene scalars (ray_caster.kernel_arguments); `evaluations`: None, or
    (instance programs run, instance programs asked for = samples x n) per wavefront, when counted."""

    __slots__ = ()

    def part_at(self, x, y):
        """The Instance under pixel (x, y) -- column, row --, or None."""
        k = int(self.part_ids[y, x])
        return None if k < 0 else self.instances[k]


def part_colors(instances, colors):
    """float32 (n, 3) hues in [0, 1] for the placed `instances`: None -> DEFAULT_HUE for all; "parts" -> PALETTE per BOM
    item (instances of one Part share it); a sequence of n RGB triples; or {part name: rgb} (parts it does not name
    keep DEFAULT_HUE).  ValueError for a wrong length, an unknown name or a component outside [0, 1]."""
    n = len(instances)
    out = numpy.empty((n, 3), dtype=numpy.float64)
    out[:] = DEFAULT_HUE
    if colors is None:
        pass
    elif isinstance(colors, str):
        if colors != "parts":
            raise ValueError('colors must be None, "parts", a sequence of RGB triples or a {part name: rgb} dict, not %r' % (colors,))
        parts = []
        for k, instance in enumerate(instances):
            for item, part in enumerate(parts):
                if part is instance.part:
                    break
            else:
                item = len(parts)
                parts.append(instance.part)
            out[k] = PALETTE[item % len(PALETTE)]
    elif isinstance(colors, dict):
        names = {instance.name for instance in instances}
        unknown = sorted(str(name) for name in colors if name not in names)
        if unknown:
            raise ValueError("colors names parts the assembly does not show: %s" % ", ".join(unknown))
        for k, instance in enumerate(instances):
            if instance.name in colors:
                out[k] = _rgb(colors[instance.name])
    else:
        colors = list(colors)
        if len(colors) != n:
            raise ValueError("colors has %d entries, the assembly shows %d instances" % (len(colors), n))
        for k, c in enumerate(colors):
            out[k] = _rgb(c)
    if not (numpy.isfinite(out).all() and (out >= 0).all() and (out <= 1).all()):
        raise ValueError("colour components must lie in [0, 1]")
    return out.astype(numpy.float32)


def _rgb(c):
    try:
        c = tuple(float(v) for v in c)
    except (TypeError, ValueError):
        raise ValueError("a colour is an (r, g, b) triple, not %r" % (c,))
    if len(c) != 3:
        raise ValueError("a colour is an (r, g, b) triple, not %r" % (c,))
    return c


def scene(asm, size=DEFAULT_SIZE, view_angle=None, colors=None):
    """Everything the launch needs, on the host: (instances placed, hues float32 (n, 3), camera, kernel arguments).
    Raises the ValueErrors of render_assembly_pixels; touches no device."""
    instances = cells.visible(asm, 1.0)      # (the checks' resolution argument plays no part here)
    if not instances:
        raise ValueError("the assembly has no visible instance: nothing to aim a camera at")
    hues = part_colors(instances, colors)
    united = asm.shape()
    camera = ray_caster.get_camera_params(united.bounding_box(), size, view_angle)
    return instances, hues, camera, ray_caster.kernel_arguments(united, *camera)


def render_assembly_pixels(asm, size=DEFAULT_SIZE, view_angle=None, colors=None, options=RenderOptions.no_flags, skip=True,
                           count=False):
    """-> AssemblyPicture of the 3D assembly `asm` seen along +y (`view_angle` in degrees; None = a normal lens), see
    the module's docstring.  `colors`: part_colors(); `options`: ray_caster.RenderOptions (false colour and zebra keep
    their meaning); `skip=False` evaluates every instance at every sample (the same arrays, slower); `count=True` fills
    `evaluations`.

    Raises ValueError for a 2D assembly, more than 64 visible instances, none at all, or bad colours -- before any launch."""
    size = (int(size[0]), int(size[1]))
    instances, hues, camera, a = scene(asm, size, view_angle, colors)
    n = len(instances)
    queue = hip_manager.queue
    table, distance_only, lane_bytes = cells.device_table(instances, queue, full_programs=True)
    hues4 = numpy.zeros((n, 4), dtype=numpy.float32)
    hues4[:, :3] = hues
    colors_dev = hip_util.Buffer(numpy.float32, hues4.shape, queue=queue)
    colors_dev.enqueue_write(hues4)
    pixels = hip_util.Buffer(numpy.uint8, size + (3,), queue=queue)
    part_ids = hip_util.Buffer(numpy.int32, size, queue=queue)
    depth = hip_util.Buffer(numpy.float32, size, queue=queue)
    counters = None
    if count:
        counters = hip_util.Buffer(numpy.uint64, (2,), queue=queue)
        counters.enqueue_fill(0)
    ev = hip_manager.k.ray_caster_instances(
        size, None, table, n, distance_only, lane_bytes, a["origin"].as_float4(), a["forward"].as_float4(), a["up"].as_float4(),
        a["right"].as_float4(), numpy.float32(a["pixel_tolerance"]), numpy.float32(a["box_radius"]), numpy.float32(a["min_distance"]),
        numpy.float32(a["max_distance"]), numpy.float32(a["floor_z"]), numpy.uint32(int(options)), colors_dev, pixels, part_ids, depth,
        flags=0 if skip else 1, counters=counters, queue=queue)
    ev.wait()
    got = AssemblyPicture(pixels.read().copy().transpose((1, 0, 2)), part_ids.read().copy().T, depth.read().copy().T,
                          [cells.Instance(i.name, i) for i in instances], hues, camera, a,
                          tuple(int(v) for v in counters.read()) if counters is not None else None)
    for b in (table, colors_dev, pixels, part_ids, depth) + ((counters,) if counters is not None else ()):
        b.release()
    return got


def render_assembly_pil_image(asm, size=DEFAULT_SIZE, view_angle=None, colors="parts", options=RenderOptions.no_flags):
    import PIL.Image
    return PIL.Image.fromarray(render_assembly_pixels(asm, size, view_angle, colors, options).pixels)


def render_assembly_image(asm, filename, size=DEFAULT_SIZE, view_angle=None, colors="parts", options=RenderOptions.no_flags):
    render_assembly_pil_image(asm, size, view_angle, colors, options).save(filename)
