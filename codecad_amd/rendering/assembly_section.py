"""The picture of a section of an assembly (codecad_amd/section.py): every sample of the cut in the colour of the part
that owns it, samples inside two parts or more in a colour of their own, part boundaries outlined.  The maps come from
the device (`section()`); the colouring is NumPy over them.  The image has v pointing up and u to the right, like the
other renderers: row 0 is the greatest v."""
import numpy

from .. import _instance_cells as cells
from ..section import section
from .assembly_picture import part_colors


def section_colors(part_ids, inside_count, hues, overlap_color=(1, 0, 0), background=(1, 1, 1), outline=True):
    """uint8 (h, w, 3) from the maps of a Section (shape (dims v, dims u)): `hues[k]` (float (n, 3) in [0, 1]) where part k
    owns the sample, `background` where none does, `overlap_color` where inside_count >= 2; with `outline`, samples whose
    part id differs from that of a 4-neighbour at half the brightness.  Row 0 of the image is the last row of the maps."""
    part_ids = numpy.asarray(part_ids)
    table = numpy.concatenate([numpy.asarray(hues, dtype=numpy.float32).reshape(-1, 3),
                               numpy.asarray([background], dtype=numpy.float32)])
    rgb = table[part_ids]                       # (-1, no part, takes the last row)
    rgb[numpy.asarray(inside_count) >= 2] = numpy.asarray(overlap_color, dtype=numpy.float32)
    if outline:
        edge = numpy.zeros(part_ids.shape, dtype=bool)
        differs = part_ids[1:, :] != part_ids[:-1, :]
        edge[1:, :] |= differs
        edge[:-1, :] |= differs
        differs = part_ids[:, 1:] != part_ids[:, :-1]
        edge[:, 1:] |= differs
        edge[:, :-1] |= differs
        rgb[edge] *= numpy.float32(0.5)
    return numpy.rint(numpy.clip(rgb, 0, 1) * 255).astype(numpy.uint8)[::-1]


def _triple(c, what):
    try:
        c = tuple(float(v) for v in c)
    except (TypeError, ValueError):
        raise ValueError("%s is an (r, g, b) triple, not %r" % (what, c))
    if len(c) != 3 or not all(0 <= v <= 1 for v in c):
        raise ValueError("%s is an (r, g, b) triple with components in [0, 1], not %r" % (what, c))
    return c


def render_assembly_section_pixels(asm, plane, resolution, colors="parts", overlap_color=(1, 0, 0), background=(1, 1, 1), outline=True):
    """-> (uint8 (h, w, 3), Section) of the 3D assembly `asm` cut by `plane` at `resolution`: section() and
    section_colors().  `colors`: assembly_picture.part_colors().  Raises the ValueErrors of section() and of bad colours."""
    overlap_color, background = _triple(overlap_color, "overlap_color"), _triple(background, "background")
    hues = part_colors(cells.visible(asm, resolution), colors)      # (bad colours are refused before any launch)
    cut = section(asm, plane, resolution)
    return section_colors(cut.part_ids, cut.inside_count, hues, overlap_color, background, outline), cut


def render_assembly_section_pil_image(asm, plane, resolution, colors="parts", overlap_color=(1, 0, 0), background=(1, 1, 1), outline=True):
    import PIL.Image
    return PIL.Image.fromarray(render_assembly_section_pixels(asm, plane, resolution, colors, overlap_color, background, outline)[0])


def render_assembly_section_image(asm, filename, plane, resolution, colors="parts", overlap_color=(1, 0, 0), background=(1, 1, 1),
                                  outline=True):
    render_assembly_section_pil_image(asm, plane, resolution, colors, overlap_color, background, outline).save(filename)
