"""codecad_amd: MI355X-native SDF evaluation behind the bluecube/codecad modelling surface.

    import codecad_amd as codecad
    s = codecad.shapes.sphere(130) & codecad.shapes.box(100)
    codecad.mass_properties(s, 1.0)

Public layout mirrors the reference package (reference codecad/__init__.py:1-11): `shapes`,
`util`, `nodes`, `hip_util` (in place of `cl_util`), `grid_eval`, `subdivision`,
`mass_properties`, `assembly` (assemblies.py) and the renderers the package has (`rendering`);
`interference(asm, resolution)` finds the overlapping instances of an assembly on the device, and
`clearance(asm, resolution, min_gap)` the pairs closer than a gap, with how close and where (clearance.py);
`separation(asm, resolution)` how far apart every pair of parts is and where they come closest, by branch and bound on the
device (separation.py);
`section(asm, plane, resolution)` cuts an assembly with a `Plane`: which part owns each sample of the cut, where parts
overlap on it, and the cut area of every part and pair (section.py); `section_outlines(asm, plane, resolution)` gives the
same cut as vectors: closed outlines per part on the plane (section_outlines.py), and
`layer_outlines(asm, plane, resolution, heights)` those outlines on a stack of parallel planes -- the layers of a print -- in
one traversal of the device, `layer_heights(asm, plane, layer_height)` the heights of such a stack (layer_outlines.py);
`assembly_mass_properties(asm, resolution, densities)` weighs an assembly: volume, mass, centre of gravity and inertia of
every part and of the whole, overlaps counted once (assembly_mass.py); `assembly_meshes(asm, resolution)` gives the surface of
every part as placed, one triangle mesh each on one lattice (assembly_meshes.py); `assembly_voxels(asm, resolution)` gives the
lattice itself: a uint8 volume with the index of the part that owns each sample, filled on the device (assembly_voxels.py);
`cavities(asm, resolution)` finds the voids of that volume that no path joins to the outside, and
`assembly_components(asm, resolution, of)` its connected components of empty space or of solid, labelled on the device
(assembly_components.py); `thin_walls(asm, resolution, min_thickness)` flags the walls of that volume that are thinner than a
ball, by an exact distance transform on the device, with the thin regions as components (thin_walls.py);
`overhangs(asm, resolution, axis, up)` says what a print along a lattice axis lays into air, how much support holds it up and
whether those supports stand on the plate or on a part, by a scan along the lattice lines on the device (overhangs.py);
`disassembly(asm, resolution)` says which part blocks which along the lattice axes, how far a part travels before it meets
another and in what order the parts come apart by straight moves, by one scan per axis on the device (disassembly.py);
`contacts(asm, resolution)` says which parts touch, over what area, where, facing which way and in what patches, which parts
form connected groups and which hang loose, by one pass across the faces of that volume on the device (contacts.py);
`drainage(asm, resolution, axis, up)` says what the assembly holds when it is drained with a lattice axis pointing up -- cups,
blind holes, U-bends, pockets between parts --, on which parts each pool stands and how high it fills, by a labelling of the
layers and a scan with a carry along the lattice lines on the device (drainage.py);
`islands(asm, resolution, axis, up, of)` says what a print along a lattice axis starts in mid-air -- a peg hanging from a
ceiling, the short leg of an arch, a captive ball --, where each island starts, where it is finally joined from above and
which islands stay loose, by grounding the solid from the plate with the same layer labelling and scans (islands.py);
`tool_access(asm, resolution, axis, up, tool, of)` says what a 3-axis cutter with its spindle along a lattice axis cannot
remove -- undercuts, and what is in view but too narrow for the tool: inside corners, slots, the fillet of a ball nose --,
which part holds or crowds each pocket of it, and the drop-cutter surface of the tool (`flat_tool`, `ball_tool`, `Tool`), by a
grey-scale closing of the height field of that volume between two scans of it on the device (tool_access.py);
`wall_thickness(asm, resolution, max_thickness, of)` says how thick the solid is at every sample -- the greatest ball inside it
that contains the sample, up to a cap -- and per part the thinnest spot and where it is, by the distance transform of
`thin_walls` and one dense gather over tiles on the device (wall_thickness.py);
`flow_length(asm, resolution, source, of)` says how far it is through the material from gates, from the plate or from the
lattice's rim (`Gates`, `Samples`, `Plate`, `BORDER`) -- the flow length of a moulding, the way out of a channel -- and per
part the sample that is reached last, by a min-plus relaxation along the lattice lines that is repeated on the device until it
changes nothing (flow_length.py).
The CLI is out of scope.  Importing the package does not touch the GPU; the first kernel launch does,
and raises if the HIP library or a device is missing -- there is no CPU fallback.
"""
from . import util  # noqa: F401
from . import nodes  # noqa: F401
from . import shapes  # noqa: F401
from . import hip_util  # noqa: F401
from . import grid_eval  # noqa: F401
from . import subdivision  # noqa: F401
from .mass_properties import mass_properties, MassProperties  # noqa: F401
from . import examples  # noqa: F401
from . import rendering  # noqa: F401
from . import assemblies  # noqa: F401
from .assemblies import assembly  # noqa: F401
from .interference import interference, InterferenceReport  # noqa: F401
from .clearance import clearance, ClearanceReport, NearMiss  # noqa: F401
from .separation import separation, SeparationReport, PairSeparation  # noqa: F401
from .section import section, Section, Plane  # noqa: F401
from .section_outlines import section_outlines, Outlines, Loop  # noqa: F401
from .layer_outlines import layer_outlines, layer_heights, Layers, LAYER_SEGMENT  # noqa: F401
from .assembly_mass import assembly_mass_properties, AssemblyMassReport, PartMass  # noqa: F401
from .assembly_meshes import assembly_meshes, Meshes, TRIANGLE  # noqa: F401
from .assembly_voxels import assembly_voxels, AssemblyVoxels  # noqa: F401
from .assembly_components import (assembly_components, cavities, ComponentsReport, CavityReport, Component, Cavity,  # noqa: F401
                                  EMPTY_SPACE, SOLID)
from .thin_walls import thin_walls, ThinWallReport  # noqa: F401
from .overhangs import overhangs, OverhangReport  # noqa: F401
from .disassembly import disassembly, DisassemblyReport  # noqa: F401
from .contacts import contacts, ContactReport  # noqa: F401
from .drainage import drainage, DrainageReport, Pool  # noqa: F401
from .islands import islands, IslandReport, Island  # noqa: F401
from .tool_access import tool_access, ToolAccessReport, Tool, flat_tool, ball_tool  # noqa: F401
from .wall_thickness import wall_thickness, WallThicknessReport  # noqa: F401
from .flow_length import flow_length, FlowLengthReport, Gates, Samples, Plate, BORDER  # noqa: F401

__all__ = ["util", "nodes", "shapes", "hip_util", "grid_eval", "subdivision", "mass_properties",
           "MassProperties", "examples", "assembly", "interference", "InterferenceReport", "clearance",
           "ClearanceReport", "NearMiss", "separation", "SeparationReport", "PairSeparation", "section", "Section", "Plane", "section_outlines", "Outlines", "Loop", "layer_outlines",
           "layer_heights", "Layers", "LAYER_SEGMENT", "assembly_mass_properties",
           "AssemblyMassReport", "PartMass", "assembly_meshes", "Meshes", "TRIANGLE", "assembly_voxels", "AssemblyVoxels",
           "assembly_components", "cavities", "ComponentsReport", "CavityReport", "Component", "Cavity", "EMPTY_SPACE", "SOLID",
           "thin_walls", "ThinWallReport", "overhangs", "OverhangReport", "disassembly", "DisassemblyReport",
           "contacts", "ContactReport", "drainage", "DrainageReport", "Pool", "islands",
           "IslandReport", "Island", "tool_access", "ToolAccessReport", "Tool", "flat_tool", "ball_tool",
           "wall_thickness", "WallThicknessReport", "flow_length", "FlowLengthReport", "Gates", "Samples", "Plate", "BORDER"]
