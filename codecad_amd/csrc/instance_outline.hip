// codecad_amd/csrc/instance_outline.hip
//
// The OUTLINES of an assembly's section (codecad_amd/section_outlines.py): the kernels and the entry points.  The kernels'
// body is outline_kernels.hpp's, which defines the outlines, with OutlineArgs: the plane's corner is the kernel argument
// c.corner, word 1 of a row is unused and written as 0, and a segment is a 16-byte record
// {a | b << 16, k | e_from << 8 | e_to << 16, t_from, t_to}.  instance_layers.hip wraps the same body for a stack of planes.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).
#include "outline_kernels.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

template <bool DO> __global__ void __launch_bounds__(256) k_outline_tiles(const OutlineArgs t) { outline_tiles<DO>(t); }
template <bool DO> __global__ void __launch_bounds__(256) k_outline_leaf(const OutlineArgs t) { outline_leaf<DO>(t); }

// [leaf][distance_only]
void (*const kOutlineTable[2][2])(OutlineArgs) = {
    {k_outline_tiles<false>, k_outline_tiles<true>},
    {k_outline_leaf<false>, k_outline_leaf<true>},
};
HU_BIG_LDS(kOutlineTable);

}  // namespace

extern "C" {

int hu_outline_tiles(const hu_cells_launch* launch, const hu_cells_children* children, const float u[3], const float v[3])
{
    OutlineArgs t;
    int rc;
    if ((rc = outline_frame_args(launch, u, v, t))) return rc;
    if ((rc = outline_children(t.c, children))) return rc;
    return cells_launch(kOutlineTable[0][launch->distance_only != 0], t, t.c, *launch, 0u);
}

int hu_outline_leaf(const hu_cells_launch* launch, const float u[3], const float v[3], void* segments_dev, uint32_t segment_capacity,
                    uint64_t* totals_dev)
{
    OutlineArgs t;
    int rc;
    if ((rc = outline_frame_args(launch, u, v, t))) return rc;
    if ((rc = outline_segments(t, segments_dev, segment_capacity, totals_dev))) return rc;
    // the 81 values of a tile: 128 floats per wavefront, 8 bytes per lane, after the register file
    return cells_launch(kOutlineTable[1][launch->distance_only != 0], t, t.c, *launch, 8u);
}

}  // extern "C"
