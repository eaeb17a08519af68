"""The part-id volume of an assembly (codecad_amd/assembly_voxels.py) as a stack of bitmaps, one per lattice plane:
`layer_%05d.png` in a directory, every sample in the colour of the part that owns it -- the input of a multi-material
print.  The volume comes from the device (`assembly_voxels()`); the colouring is NumPy over it.  An image has y pointing
up and x to the right, like the section's picture: row 0 is the greatest y."""
import os

import numpy

from .. import _instance_cells as cells
from ..assembly_voxels import assembly_voxels, EMPTY
from .assembly_picture import part_colors
from .assembly_section import section_colors, _triple

LAYER_FILE = "layer_%05d.png"


def render_assembly_voxel_pixels(voxels, z, colors="parts", background=(1, 1, 1)):
    """uint8 (ny, nx, 3): lattice plane `z` of the AssemblyVoxels `voxels`, `part_colors()` of `colors` where a part owns
    the sample and `background` where none does (section_colors() without overlaps and outlines).  Raises ValueError for
    bad colours and IndexError for a plane the lattice does not have."""
    background = _triple(background, "background")
    hues = part_colors([i.instance for i in voxels.instances], colors)
    if not 0 <= int(z) < int(voxels.dims[2]):
        raise IndexError("the lattice has the planes 0..%d, not %r" % (int(voxels.dims[2]) - 1, z))
    ids = voxels.layer(int(z)).T.astype(numpy.int32)
    ids[ids == EMPTY] = -1
    return section_colors(ids, numpy.zeros(ids.shape, numpy.uint8), hues, background=background, outline=False)


def render_assembly_voxel_layers(asm, resolution, directory, colors="parts", background=(1, 1, 1)):
    """Writes the part-id volume of the 3D assembly `asm` at `resolution` as one PNG per z plane, `directory`/layer_00000.png
    and so on (the directory is made when it is not there) -> the AssemblyVoxels.  Raises the ValueErrors of
    assembly_voxels() and of bad colours."""
    import PIL.Image
    _triple(background, "background")
    part_colors(cells.visible(asm, resolution), colors)         # (bad colours are refused before any launch)
    voxels = assembly_voxels(asm, resolution)
    os.makedirs(directory, exist_ok=True)
    for z in range(int(voxels.dims[2])):
        PIL.Image.fromarray(render_assembly_voxel_pixels(voxels, z, colors, background)).save(os.path.join(directory, LAYER_FILE % z))
    return voxels
