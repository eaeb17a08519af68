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
HU_BIG_LDS(kLayerTable);

constexpr uint32_t kMaxLayers = 1u << 20;     // (a record keeps the layer in the 20 bits from bit 12)

// What both entry points of the layered outlines check and fill: outline_frame_args() and the table of the layers' corners.
// `corner` is checked and otherwise unused.
int layer_args(const hu_cells_launch* l, const float u[3], const float v[3], const float* layer_corners_dev, uint32_t n_layers, LayerArgs& t)
{
    if (!l || !u || !v || !layer_corners_dev) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (n_layers == 0u || n_layers > kMaxLayers) return hu_fail(HU_ERR_BAD_ARG, "1..2^20 layers");
    int rc;
    if ((rc = outline_frame_args(l, u, v, t))) return rc;
    t.layer_corners = reinterpret_cast<const float4*>(layer_corners_dev);
    t.n_layers = n_layers;
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_layer_tiles(const hu_cells_launch* launch, const hu_cells_children* children, const float u[3], const float v[3],
                   const float* layer_corners_dev, uint32_t n_layers)
{
    LayerArgs t;
    int rc;
    if ((rc = layer_args(launch, u, v, layer_corners_dev, n_layers, t))) return rc;
    if ((rc = outline_children(t.c, children))) return rc;
    return cells_launch(kLayerTable[0][launch->distance_only != 0], t, t.c, *launch, 0u);
}

int hu_layer_leaf(const hu_cells_launch* launch, const float u[3], const float v[3], const float* layer_corners_dev, uint32_t n_layers,
                  void* segments_dev, uint32_t segment_capacity, uint64_t* totals_dev)
{
    LayerArgs t;
    int rc;
    if ((rc = layer_args(launch, u, v, layer_corners_dev, n_layers, t))) return rc;
    if ((rc = outline_segments(t, segments_dev, segment_capacity, totals_dev))) return rc;
    // the 81 values of a tile: 128 floats per wavefront, 8 bytes per lane, after the register file
    return cells_launch(kLayerTable[1][launch->distance_only != 0], t, t.c, *launch, 8u);
}

}  // extern "C"
