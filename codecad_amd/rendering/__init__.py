"""Renderers built on the same evaluate() (reference codecad/rendering/): the sphere-tracing ray
caster for 3D shapes and the inside/outside bitmap for 2D shapes, as one `render_image` (SURVEY.md section
8(f) rank 3), the 2D contouring `polygon2d.polygon` with its SVG writer (rank 4), and the leaf-block
consumer `mesh.triangular_mesh` (marching cubes on the device) with its STL writer (rank 2); an assembly's
bill of materials as CSV (`render_bom`) and its picture with a colour per part, a part-id map and a depth map
(`render_assembly_image`, assembly_picture.py) and the picture of its section on a plane
(`render_assembly_section_image`, assembly_section.py) or its outlines as an SVG drawing
(`render_assembly_section_svg`, assembly_section_svg.py), a stack of parallel cuts as one drawing per layer
(`render_assembly_layers_svg`, assembly_layers_svg.py), its parts as one binary STL each
(`render_assembly_stl`, assembly_stl.py), and its part-id volume as one PNG per lattice plane
(`render_assembly_voxel_layers`, assembly_voxel_layers.py).  The rest of the reference's rendering package (matplotlib viewers, animations, the CLI dispatch) is out of scope."""
from . import ray_caster, pictures, polygon2d, mesh, stl_renderer, bom, assembly_picture, assembly_section, assembly_section_svg, assembly_stl  # noqa: F401
from . import assembly_layers_svg, assembly_voxel_layers  # noqa: F401
from .bom import render_bom  # noqa: F401
from .stl_renderer import render_stl  # noqa: F401
from .pictures import render_image, render_pil_image, render_pixels  # noqa: F401
from .polygon2d import render_svg  # noqa: F401
from .assembly_picture import render_assembly_image, render_assembly_pil_image, render_assembly_pixels  # noqa: F401
from .assembly_section import render_assembly_section_image, render_assembly_section_pil_image, render_assembly_section_pixels  # noqa: F401
from .assembly_section_svg import render_assembly_section_svg, assembly_section_svg_document  # noqa: F401
from .assembly_layers_svg import render_assembly_layers_svg  # noqa: F401
from .assembly_stl import render_assembly_stl, write_assembly_stl  # noqa: F401
from .assembly_voxel_layers import render_assembly_voxel_layers, render_assembly_voxel_pixels  # noqa: F401
