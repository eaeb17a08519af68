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

}  // namespace

hipError_t hu_cells::allow_big_lds_outline(size_t bytes)
{
    return allow_big_lds_table(kOutlineTable, bytes);
}

extern "C" {

int hu_outline_tiles(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const uint32_t* windows_dev,
                     const void* parents_dev, const uint32_t* n_parents_dev, uint32_t max_parents, uint32_t child_side,
                     const uint32_t dims[2], const float corner[3], const float u[3], const float v[3], float step, float radius,
                     uint32_t* counter_dev, void* children_dev, uint32_t capacity, uint64_t* evaluations_dev, void* stream)
{
    OutlineArgs t;
    int rc;
    if ((rc = outline_frame_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, step, evaluations_dev, t)))
        return rc;
    if ((rc = cells_children(t.c, child_side, radius, counter_dev, children_dev, capacity))) return rc;
    if (child_side < 8u || child_side > 8192u || (child_side & (child_side - 1u)))
        return hu_fail(HU_ERR_BAD_ARG, "child_side must be a power of two in 8..8192");
    if (std::isnan(radius) || radius < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "radius must not be negative");
    return cells_launch(kOutlineTable[0][distance_only_kernel != 0], t, t.c, lane_bytes, 0u, stream);
}

int hu_outline_leaf(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const uint32_t* windows_dev,
                    const void* parents_dev, const uint32_t* n_parents_dev, uint32_t max_parents, const uint32_t dims[2],
                    const float corner[3], const float u[3], const float v[3], float step, void* segments_dev,
                    uint32_t segment_capacity, uint64_t* totals_dev, uint64_t* evaluations_dev, void* stream)
{
    OutlineArgs t;
    int rc;
    if ((rc = outline_frame_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, step, evaluations_dev, t)))
        return rc;
    if (!totals_dev || (!segments_dev && segment_capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    t.c.child_side = 1u;
    t.c.pairs = totals_dev;
    t.segments = static_cast<uint4*>(segments_dev);
    t.segment_capacity = segment_capacity;
    // the 81 values of a tile: 128 floats per wavefront, 8 bytes per lane, after the register file
    return cells_launch(kOutlineTable[1][distance_only_kernel != 0], t, t.c, lane_bytes, 8u, stream);
}

}  // extern "C"
