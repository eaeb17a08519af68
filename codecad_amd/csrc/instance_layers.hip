// codecad_amd/csrc/instance_layers.hip
//
// The LAYERED OUTLINES of an assembly (codecad_amd/layer_outlines.py): the outlines of instance_outline.hip on a stack of
// parallel planes, every layer in ONE traversal.  The layers share the instance table, the frame (u, v), the step, the
// lattice of squares and the windows; they differ in the 3D position of the section's sample (0, 0) alone, and a tile's row
// says which layer it belongs to in its second word: {a0 | b0 << 16, layer, mask lo, mask hi}.  The corners are a table of
// n_layers float4 {x, y, z, unused} in global memory; one wavefront takes one tile, so the layer is wave-uniform and the
// corner arrives through constant_uniform by one scalar load, like the windows and the programs.  A row whose layer is not
// below n_layers is treated as absent: nothing is read past the table.  Children inherit their parent's layer word, and a
// segment is a 16-byte record {a | b << 16, k | e_from << 8 | e_to << 10 | layer << 12, t_from, t_to}.
//
// Those are the LayerArgs hooks of outline_kernels.hpp.  Everything else -- the squares and their segments, the keep rule of
// the tiles, the two passes and the placement of the leaf -- is that header's one body, which instance_outline.hip wraps too.
// Built WITHOUT -structurizecfg-skip-uniform-regions (hip_util/builder.py FLAGGED_SOURCES).
#include "outline_kernels.hpp"

using namespace sdfk;
using namespace hu_cells;

namespace {

template <bool DO> __global__ void __launch_bounds__(256) k_layer_tiles(const LayerArgs t) { outline_tiles<DO>(t); }
template <bool DO> __global__ void __launch_bounds__(256) k_layer_leaf(const LayerArgs t) { outline_leaf<DO>(t); }

// [leaf][distance_only]
void (*const kLayerTable[2][2])(LayerArgs) = {
    {k_layer_tiles<false>, k_layer_tiles<true>},
    {k_layer_leaf<false>, k_layer_leaf<true>},
};

constexpr uint32_t kMaxLayers = 1u << 20;     // (a record keeps the layer in the 20 bits from bit 12)

// What both entry points of the layered outlines check and fill: outline_frame_args() and the table of the layers' corners.
// `corner` is checked and otherwise unused.
int layer_args(const void* table_dev, uint32_t n, const uint32_t* windows_dev, const void* parents_dev, const uint32_t* n_parents_dev,
               uint32_t max_parents, const uint32_t dims[2], const float corner[3], const float u[3], const float v[3],
               const float* layer_corners_dev, uint32_t n_layers, float step, uint64_t* evaluations_dev, LayerArgs& t)
{
    if (!dims || !u || !v || !layer_corners_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (n_layers == 0u || n_layers > kMaxLayers) return hu_fail(HU_ERR_BAD_ARG, "1..2^20 layers");
    int rc;
    if ((rc = outline_frame_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, step, evaluations_dev, t)))
        return rc;
    t.layer_corners = reinterpret_cast<const float4*>(layer_corners_dev);
    t.n_layers = n_layers;
    return HU_OK;
}

}  // namespace

hipError_t hu_cells::allow_big_lds_layers(size_t bytes)
{
    return allow_big_lds_table(kLayerTable, bytes);
}

extern "C" {

int hu_layer_tiles(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const uint32_t* windows_dev,
                   const void* parents_dev, const uint32_t* n_parents_dev, uint32_t max_parents, uint32_t child_side,
                   const uint32_t dims[2], const float corner[3], const float u[3], const float v[3], const float* layer_corners_dev,
                   uint32_t n_layers, float step, float radius, uint32_t* counter_dev, void* children_dev, uint32_t capacity,
                   uint64_t* evaluations_dev, void* stream)
{
    LayerArgs t;
    int rc;
    if ((rc = layer_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, layer_corners_dev, n_layers,
                         step, evaluations_dev, t)))
        return rc;
    if ((rc = cells_children(t.c, child_side, radius, counter_dev, children_dev, capacity))) return rc;
    if (child_side < 8u || child_side > 8192u || (child_side & (child_side - 1u)))
        return hu_fail(HU_ERR_BAD_ARG, "child_side must be a power of two in 8..8192");
    if (std::isnan(radius) || radius < 0.0f) return hu_fail(HU_ERR_BAD_ARG, "radius must not be negative");
    return cells_launch(kLayerTable[0][distance_only_kernel != 0], t, t.c, lane_bytes, 0u, stream);
}

int hu_layer_leaf(const void* table_dev, uint32_t n, int distance_only_kernel, uint32_t lane_bytes, const uint32_t* windows_dev,
                  const void* parents_dev, const uint32_t* n_parents_dev, uint32_t max_parents, const uint32_t dims[2],
                  const float corner[3], const float u[3], const float v[3], const float* layer_corners_dev, uint32_t n_layers,
                  float step, void* segments_dev, uint32_t segment_capacity, uint64_t* totals_dev, uint64_t* evaluations_dev,
                  void* stream)
{
    LayerArgs t;
    int rc;
    if ((rc = layer_args(table_dev, n, windows_dev, parents_dev, n_parents_dev, max_parents, dims, corner, u, v, layer_corners_dev, n_layers,
                         step, evaluations_dev, t)))
        return rc;
    if (!totals_dev || (!segments_dev && segment_capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    t.c.child_side = 1u;
    t.c.pairs = totals_dev;
    t.segments = static_cast<uint4*>(segments_dev);
    t.segment_capacity = segment_capacity;
    // the 81 values of a tile: 128 floats per wavefront, 8 bytes per lane, after the register file
    return cells_launch(kLayerTable[1][distance_only_kernel != 0], t, t.c, lane_bytes, 8u, stream);
}

}  // extern "C"
