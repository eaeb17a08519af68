"""The drawing of a section of an assembly (codecad_amd/section_outlines.py) as an SVG: per part one path of its closed
outlines, filled with the even-odd rule in the part's colour -- a hole is a sub-path of its own --, in millimetres with
v pointing up (y is negated, as polygon2d.svg_document does).  Outlines that the lattice's rim cut open are stroked and
not filled.  The view box is the rectangle of the section's lattice with its ring of samples."""
import numpy

from .. import _instance_cells as cells
from ..section_outlines import section_outlines
from .assembly_picture import part_colors

_SVG_STYLE = ('<style type="text/css">path{stroke:#000;stroke-width:1px;vector-effect:non-scaling-stroke;}'
              'path.open{fill:none;}</style>')


def _hex(hue):
    return "#%02x%02x%02x" % tuple(int(v) for v in numpy.rint(numpy.clip(numpy.asarray(hue, dtype=numpy.float64), 0, 1) * 255))


def _sub_path(loop):
    points = loop.points
    text = ["M%r,%r" % (float(points[0][0]), -float(points[0][1]))]
    text.extend("L%r,%r" % (float(x), -float(y)) for x, y in points[1:])
    return "".join(text) + ("Z" if loop.closed else "")


def assembly_section_svg_document(outlines, colors="parts"):
    """The SVG text of an Outlines: for every instance with closed loops one <path fill-rule="evenodd"> in its colour
    (`colors`: assembly_picture.part_colors()), a closed sub-path per loop; for every instance with open loops one
    <path class="open">, stroked only.  Raises ValueError for bad colours."""
    hues = part_colors([i.instance for i in outlines.instances], colors)
    o, u, v = (x.astype(numpy.float64) for x in (outlines.plane.origin, outlines.plane.u, outlines.plane.v))
    step = float(outlines.step)
    first = numpy.array([(outlines.corner.astype(numpy.float64) - o) @ u, (outlines.corner.astype(numpy.float64) - o) @ v])
    lo = first - step                                   # the ring: sample indices -1 .. dims
    width, height = step * (outlines.dims[0] + 1), step * (outlines.dims[1] + 1)
    parts = ['<svg xmlns="http://www.w3.org/2000/svg" width="%rmm" height="%rmm" viewBox="%r %r %r %r">'
             % (width, height, float(lo[0]), -float(lo[1] + height), width, height), _SVG_STYLE]
    for k, loops in enumerate(outlines.loops):
        closed, cut = [l for l in loops if l.closed], [l for l in loops if not l.closed]
        if closed:
            parts.append('<path fill-rule="evenodd" fill="%s" d="%s"/>' % (_hex(hues[k]), "".join(_sub_path(l) for l in closed)))
        if cut:
            parts.append('<path class="open" d="%s"/>' % "".join(_sub_path(l) for l in cut))
    parts.append("</svg>")
    return "".join(parts)


def render_assembly_section_svg(asm, filename, plane, resolution, colors="parts"):
    """Writes the section of the 3D assembly `asm` on `plane` at `resolution` as an SVG drawing -> the Outlines.  Raises the
    ValueErrors of section_outlines() and of bad colours."""
    part_colors(cells.visible(asm, resolution), colors)         # (bad colours are refused before any launch)
    outlines = section_outlines(asm, plane, resolution)
    with open(filename, "w") as fp:
        fp.write(assembly_section_svg_document(outlines, colors))
    return outlines
