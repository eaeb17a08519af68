// codecad_amd/csrc/launchers.hpp -- the two launches that cross a unit boundary, and what both ray casters fill alike.
//
// Translation units (hip_util/builder.py lists the flags of each).  A unit holds its kernels AND their extern "C" entry
// points; what the host code of all of them shares is in host.hpp.
//   hip_util.hip  the tape handle and the launches of the dense / leaf-block / classification kernels over the tape
//                 interpreter, built with -mllvm -structurizecfg-skip-uniform-regions (the interpreter's dispatch loop
//                 needs it);
//   tape_build.hip  host only: a tape's own kernels, generated, compiled with hipRTC, cached on disk and loaded;
//   render.hip    every other kernel over one tape or none -- ray caster, bitmap, 2D contouring, the mass-integral
//                 reduction, the arithmetic self-test -- built WITHOUT that option: it once let a scalar branch choose a
//                 per-lane value in a divergent loop (csrc/exchange.hip), so it stays confined to the kernels that are
//                 nothing but the interpreter's wave-uniform loop around branch-free ops.  The tape's ray caster and
//                 bitmap are validated and shaped in hip_util.hip, which knows the tape, and launched through the two
//                 functions below;
//   instance_pairs.hip  the interference and clearance checks between the instances of an assembly, built without
//                 it as well;
//   instance_rays.hip   the ray caster over the instances of an assembly (codecad_amd/rendering/assembly_picture.py), likewise;
//   instance_section.hip  the planar section of an assembly (codecad_amd/section.py), likewise;
//   instance_outline.hip  the vector outlines of that section (codecad_amd/section_outlines.py), likewise;
//   instance_layers.hip   those outlines on a stack of parallel planes in one traversal (codecad_amd/layer_outlines.py), likewise;
//                 both wrap the one kernel body of outline_kernels.hpp, each with its own Args type;
//   instance_mass.hip   the mass properties of an assembly (codecad_amd/assembly_mass.py), likewise;
//   instance_mesh.hip   the surface meshes of an assembly's parts (codecad_amd/assembly_meshes.py), likewise;
//   instance_voxels.hip the part-id volume of an assembly (codecad_amd/assembly_voxels.py), likewise;
//   instance_gap.hip    the least gap of every pair of parts (codecad_amd/separation.py), likewise; these eight share
//                 instance_cells.hpp;
//   instance_components.hip, instance_thickness.hip, instance_overhang.hip, instance_blocking.hip, instance_contacts.hip,
//   instance_reach.hip, instance_tool.hip, instance_local.hip, instance_geodesic.hip
//                 the kernels that walk the part-id volume (id_volume.hpp): connected components, distance transforms,
//                 overhangs, which part blocks which, which parts touch, the layer reachability of drainage and islands,
//                 what a cutter along an axis cannot reach (with a 2D morphology stage between its two scans), the local
//                 thickness (the greatest inscribed ball over every sample, a 3D gather over tiles), and the shortest paths
//                 inside a set (a min-plus relaxation along the lines of the axes, repeated until it changes nothing);
//   sort.hip, exchange.hip, mesh.hip  the sort of a block list, the exchange step of the multi-GPU levels, marching cubes.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace hu_render {

// each enqueues one launch and returns hipGetLastError()
hipError_t ray_caster(const sdfk::InterpEval<false>& ev, const sdfk::RayCasterArgs& a, uint32_t blocks, uint32_t block, size_t lds,
                      hipStream_t stream);
hipError_t bitmap(bool distance_only, const sdf::Rec* prog, const float* extra, uint32_t n4, float ox, float oy, float oz,
                  float step_size, uint32_t width, uint32_t height, uint8_t* out, uint32_t blocks, uint32_t block, size_t lds,
                  hipStream_t stream);

// the camera and the picture of hu_ray_caster and hu_ray_caster_instances
inline sdfk::RayCasterArgs ray_caster_args(const float origin[4], const float forward[4], const float up[4], const float right[4],
                                           float pixel_tolerance, float box_radius, float min_distance, float max_distance,
                                           float floor_z, uint32_t render_options, uint32_t width, uint32_t height, void* out_dev)
{
    sdfk::RayCasterArgs a;
    a.origin = sdfk::mk3(origin[0], origin[1], origin[2]);
    a.forward = sdfk::mk3(forward[0], forward[1], forward[2]);
    a.up = sdfk::mk3(up[0], up[1], up[2]);
    a.right = sdfk::mk3(right[0], right[1], right[2]);
    a.pixel_tolerance = pixel_tolerance;
    a.box_radius = box_radius;
    a.min_distance = min_distance;
    a.max_distance = max_distance;
    a.floor_z = floor_z;
    a.options = render_options;
    a.w = width;
    a.h = height;
    a.out = static_cast<uint8_t*>(out_dev);
    return a;
}

}  // namespace hu_render
