"""The layers of an assembly (codecad_amd/layer_outlines.py) as SVG drawings, one per layer: `layer_%05d.svg` in a
directory, each the drawing assembly_section_svg.py makes of that layer's outlines."""
import os

from .. import _instance_cells as cells
from ..layer_outlines import layer_outlines
from .assembly_picture import part_colors
from .assembly_section_svg import assembly_section_svg_document

LAYER_FILE = "layer_%05d.svg"


def render_assembly_layers_svg(asm, directory, plane, resolution, heights, colors="parts"):
    """Writes the cuts of the 3D assembly `asm` on the planes parallel to `plane` at `heights`, at `resolution`, as one SVG
    drawing per layer, `directory`/layer_00000.svg and so on (the directory is made when it is not there) -> the Layers.
    Raises the ValueErrors of layer_outlines() and of bad colours."""
    part_colors(cells.visible(asm, resolution), colors)         # (bad colours are refused before any launch)
    layers = layer_outlines(asm, plane, resolution, heights)
    os.makedirs(directory, exist_ok=True)
    for l in range(len(layers.heights)):
        with open(os.path.join(directory, LAYER_FILE % l), "w") as fp:
            fp.write(assembly_section_svg_document(layers.layer(l), colors))
    return layers
