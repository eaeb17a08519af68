/* include/hip_util.h -- C ABI of libhip_util.so, the MI355X (gfx950) replacement for the
 * device half of bluecube/codecad's hot path.
 *
 * What it replaces (paths relative to /root/reference/codecad/):
 *   - cl_util/opencl_manager.py:73-85   `opencl_manager.k.<kernel>(global, local, *args)`
 *   - cl_util/cl_buffer.py:9-131        `Buffer` (device allocation + host transfers)
 *   - nodes/program.py:79-84            `make_program_buffer` (tape upload)
 *   - grid_eval.cl, subdivision.cl, mass_properties.cl and the generated evaluate()
 *   - rendering/ray_caster.cl, bitmap.cl, polygon2d.cl, and the PyMCubes call of rendering/mesh.py
 *
 * Conventions: every function returns 0 on success or a negative hu_status code; the
 * message for the last failure on the calling thread is hu_last_error().  All pointers
 * named *_dev are device pointers (from hu_malloc or any hipMalloc-compatible allocator,
 * e.g. a torch tensor's data_ptr()).  `stream` is a hipStream_t passed as void*
 * (NULL = the legacy default stream).  Launch functions are asynchronous and perform no
 * allocation or synchronisation, so they can be captured into a hipGraph (exceptions, each
 * documented at its declaration: hu_tape_create/specialize, hu_sort_blocks and hu_selftest_math
 * synchronise).  The caller owns every handle; there are no hidden global allocations.
 */
#ifndef HIP_UTIL_H
#define HIP_UTIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HU_ABI_VERSION 3

enum hu_status {
    HU_OK = 0,
    HU_ERR_HIP = -1,        /* a HIP runtime call failed (message has hipGetErrorString) */
    HU_ERR_BAD_TAPE = -2,   /* malformed instruction tape */
    HU_ERR_BAD_ARG = -3,    /* NULL pointer, zero/oversized dims, ... */
    HU_ERR_NO_DEVICE = -4,  /* no gfx950 device / no HIP runtime */
    HU_ERR_UNSUPPORTED = -5 /* e.g. tape needs more value registers than fit in LDS */
};

typedef struct hu_tape_s* hu_tape; /* opaque: decoded program resident in HBM */

/* ---- runtime (replaces OpenCLManager.__init__, opencl_manager.py:88-98) ---------------- */
int hu_abi_version(void);
const char* hu_last_error(void);
int hu_device_count(int* count);
int hu_set_device(int ordinal);
int hu_device_name(int ordinal, char* buf, size_t buflen);
int hu_synchronize(void);

/* ---- memory (replaces cl_util.Buffer / pyopencl.enqueue_copy, cl_buffer.py:31-94) ------ */
int hu_malloc(void** out_dev, size_t bytes);
int hu_free(void* dev); /* NULL is a no-op */
int hu_host_alloc(void** out_host, size_t bytes); /* pinned host memory */
int hu_host_free(void* host);
int hu_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int hu_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int hu_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
int hu_memset(void* dst_dev, int value, size_t bytes, void* stream);

/* ---- streams and events (replaces the OOO queue + pyopencl.Event, wait_for=) ----------- */
int hu_stream_create(void** out_stream);
int hu_stream_destroy(void* stream);
int hu_stream_synchronize(void* stream);
int hu_stream_wait_event(void* stream, void* event);
int hu_event_create(void** out_event);
int hu_event_destroy(void* event);
int hu_event_record(void* event, void* stream);
int hu_event_synchronize(void* event);
int hu_event_elapsed_ms(void* start, void* stop, float* out_ms);

/* ---- tape (replaces nodes.make_program_buffer, nodes/program.py:79-84) ------------------ */
/* `tape`: the reference float32 instruction tape (opcode*512+register words + params,
 * nodes/program.py:55-71).  Validated, pre-decoded and uploaded; synchronous. */
int hu_tape_create(const float* tape, size_t n_floats, hu_tape* out);
int hu_tape_destroy(hu_tape t);
/* n_instructions, value registers used, flags bit0 = a rounded union/intersection is present */
int hu_tape_info(hu_tape t, int* n_instructions, int* n_registers, int* flags);

/* ---- reference-shaped kernels: same arguments as the OpenCL kernels --------------------- */
/* grid_eval.cl:23-25  out_dev: float4[dims[0]*dims[1]*dims[2]], index z + sz*(y + sy*x) */
int hu_grid_eval(hu_tape t, const float corner[4], float step, const uint32_t dims[3],
                 void* out_dev, void* stream);
/* grid_eval.cl:2-4    out_dev: float[...], index z + (x + (sy-1-y)*sx)*sz */
int hu_grid_eval_pymcubes(hu_tape t, const float corner[4], float step, const uint32_t dims[3],
                          void* out_dev, void* stream);
/* subdivision.cl:12-16  counter_dev: uint32 (caller zeroes it); list_dev: uchar4[cells] */
int hu_subdivision_step(hu_tape t, const float corner[4], float step, float threshold,
                        const uint32_t dims[3], uint32_t* counter_dev, void* list_dev,
                        void* stream);
/* mass_properties.cl:7-12  sum_dev: uint32[10] xx,xy,xz,x,yy,yz,y,zz,z,n (caller zeroes) */
int hu_mass_properties(hu_tape t, const float corner[4], float step, float threshold,
                       const uint32_t dims[3], uint32_t* sum_dev, uint32_t* counter_dev,
                       void* list_dev, void* stream);

/* ---- level-batched kernels (one launch per subdivision LEVEL instead of one per block) -- */
/* Dense grid sharded along x: evaluates x in [x0, x0+x_count) of the logical grid `dims`
 * and writes them at out_dev (which points at the FIRST voxel of the slab).  layout 0 =
 * float4 grid_eval, 1 = float grid_eval_pymcubes (then out_dev is the whole-grid base). */
int hu_grid_eval_slab(hu_tape t, const float corner[4], float step, const uint32_t dims[3],
                      uint32_t x0, uint32_t x_count, int layout, void* out_dev, void* stream);

/* Leaf blocks of subdivision() (subdivision.py:96-111): blocks_dev = int32[4]*n_blocks
 * integer corners; float corner = int*resolution + origin in fp64, cast once
 * (util/geometry.py:98-99).  out_dev: n_blocks consecutive grids of `dims`. */
int hu_grid_eval_blocks(hu_tape t, const int32_t* blocks_dev, uint32_t n_blocks,
                        double resolution, const double origin[3], float step,
                        const uint32_t dims[3], int layout, void* out_dev, void* stream);

/* ---- the launch record of a level of a tape's hierarchy ----------------------------------------------
 * hu_subdivision_level and hu_mass_properties_level classify one level for ALL its parents in one launch and take what such
 * a launch needs as ONE record; then come the entry point's own arguments.  The record is read during the call and not
 * kept: a caller may fill one and change its list fields from level to level.  A NULL record is HU_ERR_BAD_ARG.
 * The list lengths.  n_parents_dev == NULL: exactly max_parents parents.  Else the length is ON THE DEVICE, so that a whole
 * traversal can be enqueued without a host round trip between its levels: the launch covers max_parents (the list's
 * capacity) and workgroups past *n_parents_dev leave at once.  Typical chaining: counter_dev = word 0 of a [header row |
 * rows...] buffer and children_dev = its row 1, which makes the buffer the next level's (parents_dev = row 1, n_parents_dev
 * = word 0) and, on several GPUs, the fixed-size piece of the all-gather (hu_slice_rows).  counter_dev (the caller zeroes
 * it) ends up as the number of ambiguous cells even when it exceeds `capacity` (extra cells are dropped); the caller checks
 * counter <= capacity -- once, at the end of a traversal -- and re-runs with a larger list.
 * Ownership.  world = 1, rank = 0: every cell is kept.  world >= 2: a level that SEVERAL ranks classify in full (multi-GPU,
 * codecad_amd/dist.py "replicated levels"; the reference has one device, cl_util/opencl_manager.py:89-98): of every parent's
 * cells a rank lists -- and sums -- only those it OWNS: owner = mix(hash of the parent's row, the cell's linear index z + sz *
 * (y + sy * x)) mod world.  The ranks' lists then partition the level's survivors (their moment sums add up to the level's)
 * without any exchange, whatever order each rank's parents were in.  rank must be below world. */
typedef struct hu_level_launch {        /* what every level launch of a tape takes */
    hu_tape tape;
    const void* parents_dev;            /* rows after the list's header: int32[4] (subdivision) or double[4] (mass properties) */
    const uint32_t* n_parents_dev;      /* word 0 of the list's header; NULL: exactly max_parents parents */
    uint32_t* counter_dev;              /* word 0 of the children's header */
    void* children_dev;                 /* rows after it, of the parents' type; may be NULL for a capacity of 0 */
    void* stream;
    uint32_t max_parents, capacity;
    uint32_t world, rank;
    uint32_t dims[3];                   /* cells of a parent per axis, at most 256 each */
    float step, thr;                    /* the cells' spacing and the threshold that makes a cell ambiguous */
} hu_level_launch;
#define HU_LEVEL_LAUNCH_BYTES 88

/* One level of subdivision() (subdivision.py:48-113).  parents_dev: int32[4] integer box corners; per parent the sample
 * corner is (int_corner + int_step/2)*resolution + origin in fp64 (z unshifted when dimension==2), thr =
 * step*sqrt(dimension)/2 is computed by the caller.  Ambiguous cells are appended (wavefront ballot scan, one atomic per
 * workgroup) to children_dev as int32[4] = parent + (x,y,z)*int_step, ready to be the next level's parents; the 4th
 * component is a caller tag (e.g. an object id) copied from parent to child untouched. */
int hu_subdivision_level(const hu_level_launch* launch, int32_t int_step, int dimension, double resolution,
                         const double origin[3]);

/* hu_grid_eval_blocks with the number of blocks on the device, like a level's parents: the launch covers max_blocks and
 * workgroups past *n_blocks_dev leave at once. */
int hu_grid_eval_blocks_indirect(hu_tape t, const int32_t* blocks_dev, const uint32_t* n_blocks_dev,
                                 uint32_t max_blocks, double resolution, const double origin[3], float step,
                                 const uint32_t dims[3], int layout, void* out_dev, void* stream);
/* Multi-GPU level exchange (the reference has one device and no counterpart).  After
 * an all-gather of fixed-size pieces gathered_dev holds world x piece_rows rows of row_bytes (16 or 32) each;
 * row 0 of a piece is its header (word 0 = number of rows that follow).  Writes this rank's balanced share of
 * the concatenated rows -- begin = rank*base + min(rank, extra), base/extra = divmod(total, world) -- to
 * out_dev as [header | rows] (out_capacity rows after the header).  stats_dev: uint32[2] <- {rows over all
 * ranks, 1 if a piece or the share was truncated}.  Asynchronous, no host involvement. */
int hu_slice_rows(const void* gathered_dev, uint32_t world, uint32_t piece_rows, uint32_t row_bytes,
                  uint32_t rank, void* out_dev, uint32_t out_capacity, uint32_t* stats_dev, void* stream);
/* The same for ONE piece that every rank holds identically -- a level small enough that each rank classified ALL of it
 * itself, in one workgroup per parent, whose compaction order is the lane order and hence the same everywhere (the top
 * level of a hierarchy: one parent, a few cells) -- shared out among `world` ranks without any collective. */
int hu_slice_rows_of(const void* piece_dev, uint32_t piece_rows, uint32_t row_bytes, uint32_t rank, uint32_t world,
                     void* out_dev, uint32_t out_capacity, uint32_t* stats_dev, void* stream);

/* One level of mass_properties() (mass_properties.py:69-157).  parents_dev: double[4] box corners; sample corner = corner
 * + s/2 (fp64), cast once.  sums_dev: uint32[10] per parent (the caller zeroes them for max_parents parents), same order
 * as hu_mass_properties.  children_dev: double[4] = (i,j,k)*s + corner (fp64), 4th component = the parent's tag, appended
 * like above (32-byte rows, and a header row of 32 bytes in the chained form). */
int hu_mass_properties_level(const hu_level_launch* launch, double s, uint32_t* sums_dev);

/* The ten integrals (1, x, y, z, xx, yy, zz, xy, xz, yz over the inside cells) of one level from
 * the per-parent index sums, with the per-block formulas of mass_properties.py:119-148 in fp64,
 * summed deterministically on the device: out_dev: double[rows][10], row g = the integrals of the g-th
 * of `rows` contiguous slices of the parents (Kahan per thread, fixed tree per workgroup); the caller adds
 * the rows in order.  rows = 1 gives the level's integrals directly; more rows spread a long level over
 * the chip (1 row per ~2048 parents is plenty).  n_parents_dev as in the record: NULL for exactly max_parents parents,
 * else the rows are cut from the count on the device (at most max_parents): the same slices as with that many parents. */
int hu_mass_integrals(const double* parents_dev, const uint32_t* sums_dev, const uint32_t* n_parents_dev,
                      uint32_t max_parents, double s, double* out_dev, uint32_t rows, void* stream);

/* ---- the launch records of the entry points over instance cells ------------------------------------
 * Every entry point from here to hu_mesh_leaf_instances (hu_instance_table apart) launches one kernel over a list of cells
 * and takes what such a launch needs as ONE record, hu_cells_launch; those of a level above the finest one also take the
 * children's list as hu_cells_children.  Then come the check's own arguments.  The records are read during the call and
 * not kept: a caller may fill one, and change its parent fields from level to level.  A NULL record is HU_ERR_BAD_ARG. */
typedef struct hu_cells_launch {        /* what every launch over instance cells takes */
    const void* table_dev;              /* hu_instance_table's records */
    const uint32_t* windows_dev;        /* n x 6; NULL for entry points that take none, which never read it */
    const void* parents_dev;            /* rows after the list's header */
    const uint32_t* n_parents_dev;      /* word 0 of the list's header */
    uint64_t* evaluations_dev;
    void* stream;
    uint32_t n, lane_bytes, max_parents;   /* n and lane_bytes as hu_instance_table gave them */
    int32_t distance_only;              /* as hu_instance_table gave it */
    uint32_t dims[3];                   /* section, outline and layer entry points read [0] and [1] only */
    float corner[3];
    float step;
} hu_cells_launch;
typedef struct hu_cells_children {      /* ... and what a level above the finest adds */
    uint32_t* counter_dev;              /* word 0 of the children's header */
    void* children_dev;                 /* rows after it */
    uint32_t capacity, child_side;
    float thr;                          /* the "radius" or "r" of the section, outline, layer, mesh and separation levels */
} hu_cells_children;
#define HU_CELLS_LAUNCH_BYTES 96
#define HU_CELLS_CHILDREN_BYTES 32

/* ---- interference between the instances of an assembly (codecad_amd/interference.py) --------------
 * The instances' tapes are evaluated one at a time by the interpreter; the kernels reach them through a device
 * table of 24-byte records, n <= 64 (one bit each in a cell's candidate mask).  A cell list is a [header row |
 * rows...] buffer of 16-byte rows {x0 | y0 << 16, z0, mask lo, mask hi}, header word 0 its length; a cell is a cube
 * of lattice samples (corner + step * index, per axis) whose first sample is (x0, y0, z0).
 * hu_instance_table: no device work.  Writes the table of `tapes` into table_host (host memory of at least
 *   n * 24 bytes; the caller uploads it): every instance's distance-only program when all have one (*distance_only
 *   = 1), else every instance's full program, and *lane_bytes, the LDS bytes per lane of a register file that holds
 *   every instance's (one layout for all: the wavefronts of a workgroup run different instances at once).
 * hu_interference_cells_indirect: a cell of side 4 * child_side per parent row; each of its 4^3 children keeps the
 *   candidates whose distance at the child's centre is below thr, and is appended to children_dev (counted into
 *   *counter_dev; rows past `capacity` are dropped and counted) when two or more remain.
 * hu_interference_leaf_indirect: a cell of 4^3 samples per parent row; every pair (i < j) of candidates with
 *   samples inside both (w < 0) adds to pairs_dev[i * n + j] (64 bytes: uint64 count, x, y, z index sums; uint32
 *   min x, y, z; uint32 max x, y, z; 8 bytes unused).
 * Both read the number of parents from *n_parents_dev (at most max_parents are there) and add the sample
 * evaluations they perform to *evaluations_dev. */
/* full_programs != 0 writes every instance's FULL program (*distance_only = 0) whether or not all have a distance-only
 * one -- the ray caster over instances needs the directions --, and reports a register file of one float4 slot at least
 * (*lane_bytes >= 16) even when no program stores a value. */
int hu_instance_table(const hu_tape* tapes, uint32_t n, int full_programs, void* table_host, size_t bytes,
                      int* distance_only, uint32_t* lane_bytes);
int hu_interference_cells_indirect(const hu_cells_launch* launch, const hu_cells_children* children);
int hu_interference_leaf_indirect(const hu_cells_launch* launch, void* pairs_dev);

/* ---- clearance (near misses) between the instances of an assembly (codecad_amd/clearance.py) ----
 * The interference traversal with a threshold: the same table (hu_instance_table), cell lists and lattice.  Each
 * also takes windows_dev, n x 6 uint32 {lo x, y, z, hi x, y, z}: the lattice indices at which instance k may be near,
 * inclusive.  A sample is near the pair (i, j) when it lies in both windows and w_i < t, w_j < t (strictly); there
 * v = max(w_i, w_j).  dims at most 65536 per axis; step, t and thr finite and not negative.
 * hu_clearance_cells_indirect: as hu_interference_cells_indirect; a candidate also leaves a child whose index range
 *   misses its window.
 * hu_clearance_leaf_indirect: a cell of 4^3 samples per parent row; every pair (i < j) of candidates with near samples
 *   adds to pairs_dev[i * n + j] (72 bytes: uint64 count, x, y, z index sums; uint64 witness; uint32 min x, y, z; uint32
 *   max x, y, z; uint32 key of the least v; 4 bytes unused).  The caller starts min and key at 0xffffffff and the
 *   witness at ~0.  The key of v is its float32 bits b (of +0 for either zero) mapped to ~b when the sign is set, else
 *   b | 0x80000000, so that keys order as the values do.
 * hu_clearance_witness_indirect: after the leaf launch, over the same list and accumulators: each pair's witness
 *   becomes the least x << 32 | y << 16 | z of its near samples whose v has the pair's key.
 * All read the number of parents from *n_parents_dev and add the sample evaluations they perform to *evaluations_dev. */
int hu_clearance_cells_indirect(const hu_cells_launch* launch, const hu_cells_children* children);
int hu_clearance_leaf_indirect(const hu_cells_launch* launch, float t, void* pairs_dev);
int hu_clearance_witness_indirect(const hu_cells_launch* launch, float t, void* pairs_dev);

/* ---- the planar section of an assembly (codecad_amd/section.py) --------------------------------
 * A 2D lattice of dims[0] x dims[1] samples on a plane, sample (i, j) at (corner + u * (step * i)) + v * (step * j) per
 * coordinate in float32 (u, v: the plane's unit vectors), over the same instance table.  A list is the cell list above
 * with rows {x0 | y0 << 16, unused, mask lo, mask hi}: square tiles of samples.  windows_dev: n x 6 uint32 {lo i, lo j,
 * 0, hi i, hi j, 0}, the samples an instance may be inside at, inclusive.  At most 65536 samples per axis, 2^28 in all.
 * hu_section_tiles: a tile of side 8 * child_side per parent row; each of its 8 x 8 children keeps a candidate k whose
 *   distance at the child's centre is below `radius` (and, without with_distance, whose window reaches the child) or,
 *   with_distance, is at most the least candidate's plus 2 * radius, and is appended to children_dev when any remain.
 * hu_section_leaf: a tile of 8 x 8 samples per parent row.  Writes, at [j * dims[0] + i], part_ids_dev (int32: the lowest
 *   instance with w < 0, -1 for none), inside_count_dev (uint8: how many) and, with_distance, distance_dev (float: the
 *   least w) and nearest_dev (int32: the lowest instance that attains it; both may be NULL otherwise); samples of tiles
 *   that are in no row are left as they are.  acc_dev: n * n accumulators of hu_interference_leaf_indirect's layout (third
 *   index 0), [k * n + k] over the samples inside k, [i * n + j] (i < j) over those inside both.
 * Both read the number of parents from *n_parents_dev and add the sample evaluations they perform to *evaluations_dev. */
int hu_section_tiles(const hu_cells_launch* launch, const hu_cells_children* children, const float u[3], const float v[3],
                     int with_distance);
int hu_section_leaf(const hu_cells_launch* launch, const float u[3], const float v[3], int with_distance,
                    int32_t* part_ids_dev, uint8_t* inside_count_dev, float* distance_dev, int32_t* nearest_dev,
                    void* acc_dev);

/* ---- the outlines of an assembly's section (codecad_amd/section_outlines.py) -------------------
 * The section's lattice with a ring of samples around it: samples carry the shifted index s = (i + 1, j + 1), 0 .. dims[0]
 * by 0 .. dims[1], and sit at the section's formula for (i, j) = s - 1 (corner: the position of the section's sample
 * (0, 0)).  dims counts the SQUARES between them, per axis one more than the section's samples and at most 65536; square
 * (a, b) has the corner samples (a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1) and the edges 0 bottom, 1 right, 2 top,
 * 3 left.  A list is the section's, rows {a0 | b0 << 16, unused, mask lo, mask hi}: square tiles of squares.  windows_dev:
 * n x 6 uint32 {lo a, lo b, 0, hi a, hi b, 0}, the squares an instance may cross, inclusive.  step finite and not
 * negative, the frame finite.
 * hu_outline_tiles: a tile of side 8 * child_side per parent row; each of its 8 x 8 children keeps a candidate k whose
 *   window reaches it and whose distance w at the child's centre (shifted index a + child_side / 2 per axis) is neither
 *   >= radius nor <= -radius, and is appended to children_dev when any remain.  child_side a power of two in 8..8192,
 *   radius not negative.
 * hu_outline_leaf: a tile of 8 x 8 squares per parent row.  Every candidate k is evaluated at the tile's 9 x 9 samples;
 *   inside is w < 0.  An edge from sample p to q (lower index first) with exactly one of them inside is crossed at
 *   t = w_p / (w_p - w_q) in correctly rounded float32, 0.5 where that is no number.  Each square appends 0-2 records of
 *   16 bytes {a | b << 16, k | e_from << 8 | e_to << 16, float t_from, float t_to} to segments_dev, in no particular order:
 *   a segment from edge to edge with the inside on its left (u to the right, v up); diagonal inside corners give two, each
 *   round one inside corner.  totals_dev: n + 1 uint64, the number of records and the number per instance, added to;
 *   records at or past segment_capacity are counted and not stored (segments_dev may be NULL for a capacity of 0).
 * Both read the number of parents from *n_parents_dev and add the sample evaluations they perform (samples and children
 * past the lattice's rim not counted) to *evaluations_dev. */
int hu_outline_tiles(const hu_cells_launch* launch, const hu_cells_children* children, const float u[3], const float v[3]);
int hu_outline_leaf(const hu_cells_launch* launch, const float u[3], const float v[3], void* segments_dev,
                    uint32_t segment_capacity, uint64_t* totals_dev);

/* ---- the layered outlines of an assembly (codecad_amd/layer_outlines.py) -----------------------
 * The outlines above on a stack of n_layers parallel planes, every layer in one traversal.  The layers share the table, the
 * frame (u, v), step, dims and windows_dev; word 1 of a row is the row's layer, {a0 | b0 << 16, layer, mask lo, mask hi}, and
 * layer_corners_dev holds n_layers records of four floats {x, y, z, unused}: the position of the section's sample (0, 0) on
 * that layer, which takes the place of `corner` in the position formula.  `corner` is checked to be finite and otherwise
 * unused.  A row whose layer is not below n_layers is treated as absent.  1 <= n_layers <= 2^20.
 * hu_layer_tiles: hu_outline_tiles on the row's layer; a child carries its parent's layer.
 * hu_layer_leaf: hu_outline_leaf on the row's layer, with records {a | b << 16, k | e_from << 8 | e_to << 10 | layer << 12,
 *   float t_from, float t_to}; totals_dev counts over all layers.
 * Every other argument, check and count is that of the outline entry points. */
int hu_layer_tiles(const hu_cells_launch* launch, const hu_cells_children* children, const float u[3], const float v[3],
                   const float* layer_corners_dev, uint32_t n_layers);
int hu_layer_leaf(const hu_cells_launch* launch, const float u[3], const float v[3], const float* layer_corners_dev,
                  uint32_t n_layers, void* segments_dev, uint32_t segment_capacity, uint64_t* totals_dev);

/* ---- the mass properties of an assembly (codecad_amd/assembly_mass.py) -------------------------
 * The lattice, the instance table and the [header row | rows...] lists of the interference entry points, with rows (and a
 * header) of 32 bytes: {x0 | y0 << 16, z0, cand lo, cand hi, full lo, full hi, 0, 0} -- the candidates of the cell and, a
 * subset of them, the instances every sample of the cell is inside of.  acc_dev: n accumulators of 192 bytes: ten uint64
 * sums n, x, y, z, xx, yy, zz, xy, xz, yz of the indices of the samples inside instance k (w < 0), the same ten over the
 * samples inside k and no instance of lower index, uint32 min x, y, z and max x, y, z of the first set (the caller starts
 * the minima at 0xffffffff), 8 bytes unused.  dims at most 65536 per axis and dims[0] * dims[1] * dims[2] * (largest - 1)^2
 * below 2^64; step and thr finite and not negative; child_side a power of two.
 * hu_assembly_mass_cells: a cell of side 4 * child_side per parent row.  The parent's full instances are full in each of
 *   its 4^3 children; every other candidate is evaluated at the child's centre: dropped for w >= thr, full for w < -thr
 *   (only with retire != 0), a boundary candidate else.  A child whose candidates are all full adds the closed-form sums
 *   over its samples (clipped to dims) to each of them, and to the lowest as the owner; a child with a boundary candidate
 *   is appended to children_dev (counted into *counter_dev; rows past `capacity` are dropped and counted).
 * hu_assembly_mass_leaf: a cell of 4^3 samples per parent row; full instances are inside at every sample, the other
 *   candidates are evaluated at every sample.
 * Both read the number of parents from *n_parents_dev and add the sample evaluations they perform to *evaluations_dev. */
int hu_assembly_mass_cells(const hu_cells_launch* launch, const hu_cells_children* children, int retire, void* acc_dev);
int hu_assembly_mass_leaf(const hu_cells_launch* launch, void* acc_dev);

/* ---- the least gap of every pair of instances (codecad_amd/separation.py) -----------------------
 * The lattice, the instance table and the 16-byte rows of the interference entry points, every index within 16 bits; step
 * finite and not negative.  Per pair i < j the least v = max(w_i, w_j) over the samples where both are numbers, as the key
 * of hu_clearance_leaf_indirect, by branch and bound from cells of top_side = 16 * 4^k samples down; L = k + 1 levels lie
 * above the finest one.  acc_dev, filled with ones by the caller: n * n uint64 witnesses; L + 2 arrays of n * n uint32 keys
 * (U_0 .. U_L and the final one); L uint32, the rows each level listed.
 * hu_separation_cells: the level whose children have child_side = top_side / 4^(l + 1) >= 4.  Copies U_l to U_(l+1) on
 *   the stream, then every child of every parent row evaluates the row's candidates at its lattice sample
 *   min(first + child_side / 2, dims - 1) per axis, drops the pair (i, j) iff (v - U_l[i][j]) > r in float32 (a NaN keeps it),
 *   keeps the bits of its kept pairs and is appended to children_dev when it has any (counted into *counter_dev; rows past
 *   `capacity` are dropped and counted); U_(l+1)[i][j] takes the least key of v met.  r finite and not negative.
 * hu_separation_leaf: a cell of 4^3 samples per parent row; copies U_L to the final array, which takes the least key of
 *   every pair of candidates over the samples inside dims.
 * hu_separation_witness: after the leaf launch, over the same list: each pair's witness becomes the least
 *   x << 32 | y << 16 | z of the samples whose v has the pair's final key.
 * All read the number of parents from *n_parents_dev and add the sample evaluations they perform to *evaluations_dev. */
int hu_separation_cells(const hu_cells_launch* launch, const hu_cells_children* children, uint32_t top_side, void* acc_dev);
int hu_separation_leaf(const hu_cells_launch* launch, uint32_t top_side, void* acc_dev);
int hu_separation_witness(const hu_cells_launch* launch, uint32_t top_side, void* acc_dev);

/* ---- the part-id volume of an assembly (codecad_amd/assembly_voxels.py) -------------------------
 * The lattice, the instance table and the [header row | rows...] lists of the interference entry points, 16-byte rows
 * {x0 | y0 << 16, z0 | capped << 31, cand lo, cand hi}: capped says that the HIGHEST candidate of the cell has every sample
 * of the cell inside it; nothing above a full candidate is listed.  volume_dev: uint8[dims[0]][dims[1]][pitch], aligned to 16
 * bytes, pitch a multiple of 16 from dims[2] to 65536, filled with 255 (no part) by the caller before the first level; a
 * sample's byte becomes the lowest instance index it is inside of.  The bytes of a z run past dims[2] are unspecified.
 * acc_dev: n + 1 uint64, the caller's zeros: the samples each instance owns, then the bytes written for retired cells.
 * dims at most 65536 per axis; step and thr finite and not negative; child_side a power of two.
 * hu_assembly_voxels_cells: a cell of side 4 * child_side per parent row.  In each of its 4^3 children the candidates are
 *   evaluated at the centre in ascending index (a capped one is inherited): dropped for w >= thr, full for w < -thr (only
 *   with retire != 0), a boundary candidate else; candidates above a child's lowest full one are cleared.  A child whose
 *   lowest candidate is full has its samples (clipped to dims in x and y, to pitch in z) set to that index and counted; a
 *   child with any other candidate is appended to children_dev (counted into *counter_dev; rows past `capacity` are
 *   dropped and counted).
 * hu_assembly_voxels_leaf: a cell of 4^3 samples per parent row; every candidate but a capped one is evaluated at every
 *   sample; each z run of four samples is written as one dword (255 past dims[2]).
 * Both read the number of parents from *n_parents_dev and add the sample evaluations they perform to *evaluations_dev. */
int hu_assembly_voxels_cells(const hu_cells_launch* launch, const hu_cells_children* children, int retire, void* volume_dev,
                             uint32_t pitch, void* acc_dev);
int hu_assembly_voxels_leaf(const hu_cells_launch* launch, void* volume_dev, uint32_t pitch, void* acc_dev);

/* ---- connected components of the part-id volume (codecad_amd/assembly_components.py) -----------
 * volume_dev: the uint8[dims[0]][dims[1]][pitch] volume of the entry points above, still on the device.  S is its samples
 * z < dims[2] with id != 255 (solid != 0) or id == 255 (solid == 0); two samples of S are connected when they differ by one
 * step along one axis.  labels_dev: uint32[dims[0]][dims[1]][pitch], aligned to 4 bytes; dims[0] * dims[1] * pitch at most
 * 2^31.  Between hu_components_local and hu_components_finish an entry of a sample of S is the index INTO THE BUFFER,
 * (x * dims[1] + y) * pitch + z, of a sample of its component that is not above its own, and no call raises an entry;
 * 0xffffffff outside S and in the padding.  The calls are made in this order on one stream:
 * hu_components_local: local != 0: every workgroup labels a tile of HU_COMPONENTS_TILE_X x _Y x _Z samples in LDS and writes
 *   the index of the tile-local root; local == 0: every sample of S gets its own index.
 * hu_components_merge: unites the two sides of every connected pair across a tile face (local != 0) or of every pair at
 *   all (local == 0), union-find with atomicMin.
 * hu_components_flatten: every entry becomes the index of its root, the least of its component.
 * hu_components_stats: assign_slots != 0 (the first call): every root adds one to *counter_dev (the caller's zero) and
 *   keeps 0x80000000 | slot in its own entry.  Then every sample adds to row `slot` of table_dev, `capacity` zeroed rows of
 *   HU_COMPONENTS_ROW_BYTES, aligned to 8:
 *     uint64 count, sum x, sum y, sum z, parts; uint32 ~lo[3], hi[3], label, flags
 *   -- the lowest index per axis complemented (a zeroed row is empty), label the LINEAR index (x * dims[1] + y) * dims[2] + z
 *   of the root, flags bit 0: a sample has an index 0 or dims - 1; parts the mask of the ids of the component's samples
 *   (solid != 0) or of the in-lattice 6-neighbours of its samples (solid == 0).  Rows of slots >= capacity are not touched:
 *   with *counter_dev > capacity the caller calls again with a larger zeroed table and assign_slots == 0.
 * hu_components_finish: every entry becomes the LINEAR index of its root. */
#define HU_COMPONENTS_TILE_X 8
#define HU_COMPONENTS_TILE_Y 8
#define HU_COMPONENTS_TILE_Z 16
#define HU_COMPONENTS_ROW_BYTES 72
int hu_components_local(const void* volume_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int solid, int local,
                        void* stream);
int hu_components_merge(void* labels_dev, const uint32_t dims[3], uint32_t pitch, int local, void* stream);
int hu_components_flatten(void* labels_dev, const uint32_t dims[3], uint32_t pitch, void* stream);
int hu_components_stats(const void* volume_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int solid,
                        int assign_slots, uint32_t* counter_dev, void* table_dev, uint32_t capacity, void* stream);
int hu_components_finish(void* labels_dev, const uint32_t dims[3], uint32_t pitch, void* stream);

/* ---- capped squared distance transforms of the part-id volume (codecad_amd/thin_walls.py) ------
 * A pass of the separable transform over uint16[dims[0]][dims[1]][pitch] volumes of the pitch of the id volume ids_dev (still
 * on the device), a capped min-plus stencil along one axis:
 *     out(i) = min(cap, min over |k| <= K of in(i + k) + k * k),
 * a tap outside the lattice counting as `outside`.  S is the samples with id != 255 (of == HU_THICKNESS_SOLID) or id == of
 * (of <= 63).  The padding z in [dims[2], pitch) of any volume is neither read nor written.  lds != 0 stages the inputs of a
 * workgroup in LDS, lds == 0 reads every tap from global memory: the same bytes.  Asynchronous; in and out must not overlap.
 * hu_thickness_pass_z: along z.  depth_dev == NULL (transform 1): in = S ? cap : 0 from ids_dev, outside = 0.  Else
 *   (transform 2): in = depth_dev[...] > radius_sq ? 0 : cap, outside = cap; ids_dev is not read.
 * hu_thickness_pass_axis: along y (axis 1) or x (axis 0), in_dev -> out_dev.  A workgroup takes 64 consecutive z (along x: 64
 *   consecutive entries of a (y, z) plane) times `tile` positions along the axis; with lds != 0, tile + 2 K must not exceed
 *   HU_THICKNESS_LDS_ROWS rows of 128 bytes.  finish == 1: also adds to counts_dev[p] (64 uint64, the caller's zeros) the
 *   samples of id p whose result reaches the cap -- the core, after the x pass of transform 1 (cap = R2 + 1).  finish == 2:
 *   out_dev is not written; thin_dev (uint8, the layout of ids_dev) <- the id of a sample of S whose result reaches the cap
 *   (cap = C2 + 1: no core within C2), 255 elsewhere, counted into counts_dev[p] likewise.  One atomic per accumulator and
 *   wavefront.
 * Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL pointers, a pitch that is no multiple of 16 or
 * below dims[2], dims of 0 or above 65536, cap above 65535, K above HU_THICKNESS_MAX_K, an `of` above 63 that is not
 * HU_THICKNESS_SOLID. */
#define HU_THICKNESS_SOLID 255
#define HU_THICKNESS_MAX_K 255
#define HU_THICKNESS_LDS_ROWS 256
int hu_thickness_pass_z(const void* ids_dev, const void* depth_dev, void* out_dev, const uint32_t dims[3], uint32_t pitch,
                        uint32_t of, uint32_t radius_sq, uint32_t K, uint32_t cap, int lds, void* stream);
int hu_thickness_pass_axis(const void* in_dev, void* out_dev, const void* ids_dev, void* thin_dev, uint64_t* counts_dev,
                           const uint32_t dims[3], uint32_t pitch, int axis, uint32_t of, uint32_t K, uint32_t cap,
                           uint32_t outside, int finish, uint32_t tile, int lds, void* stream);

/* ---- the local thickness of a field on the part-id volume (codecad_amd/wall_thickness.py) --------
 * hu_thickness_local: over depth_dev and out_dev, uint16[dims[0]][dims[1]][pitch], and the id volume ids_dev of that shape, all
 *   still on the device; S as above.  in(q) = depth_dev[q] for q in S inside the lattice, 0 for every other point, whatever is
 *   stored there, and at most radius_sq + 1 (the caller's to ensure).  For a sample p of S with in(p) > 0
 *       out(p) = the greatest in(q) over the q with |p - q|^2 < in(q)          (q = p qualifies: out >= in),
 *   and out(p) = 0 on every other sample of the lattice; the padding z in [dims[2], pitch) is neither read nor written.  On
 *   the capped squared distance to the background (the x pass of transform 1, finish == 1) this is the greatest capped
 *   inscribed ball over every sample.  keys_dev (64 uint64, the caller's all ones): [p] is lowered to the least
 *   out << 48 | x << 32 | y << 16 | z over the samples of id p with out > 0.  counts_dev (64 uint64, the caller's zeros): [p] +=
 *   the samples of id p with out == radius_sq + 1.  One atomic per accumulator, wavefront and part.  A workgroup takes a tile
 *   of HU_COMPONENTS_TILE_X x _Y x _Z samples; lds != 0 stages the tile and a halo of K = isqrt(radius_sq), or of the reach of
 *   the greatest value around the tile where that is less, in LDS while that halo is at most HU_LOCAL_LDS_K (at most
 *   HU_LOCAL_LDS_BYTES a workgroup); beyond that, and with lds == 0, every tap comes from global memory: the same bytes.
 *   Asynchronous; allocates nothing.  Checked before a device is touched (HU_ERR_BAD_ARG): NULL pointers, the pitch, the dims
 *   and `of` as above, radius_sq above HU_LOCAL_MAX_RADIUS_SQ, volumes not aligned to 2 bytes, keys or counts not to 8,
 *   depth_dev == out_dev. */
#define HU_LOCAL_MAX_RADIUS_SQ 1024
#define HU_LOCAL_LDS_K 16
#define HU_LOCAL_LDS_BYTES 153664
int hu_thickness_local(const void* depth_dev, const void* ids_dev, void* out_dev, uint64_t* keys_dev, uint64_t* counts_dev,
                       const uint32_t dims[3], uint32_t pitch, uint32_t of, uint32_t radius_sq, int lds, void* stream);

/* ---- what a print direction leaves in the air (codecad_amd/overhangs.py) -----------------------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device.  S is the samples with id != 255
 * (of == HU_OVERHANG_SOLID) or id == of (of <= 63); nothing outside the lattice is in S, and the padding z in [dims[2], pitch)
 * of any volume is neither read nor written.  The build direction runs along `axis`, upwards (up != 0: the layer of a sample
 * is its index on that axis) or downwards (dims[axis] - 1 - index); "below" is one layer less.  word_dev is the DEPTH WORD, a
 * uint32 the caller zeroes: dims[axis] - h0, h0 the least layer that holds a sample of S, 0 while there is none.
 * hu_overhang_first_layer: raises the word to that value, at most one atomic per wavefront that holds a sample of S.
 * hu_overhang_mark: overhang_dev <- the id of a sample of S above layer h0 that has no sample of S below it at any lateral
 *   offset (u, v) with u * u + v * v <= reach_sq, 255 elsewhere; counts_dev[p] (64 uint64, the caller's zeros) += those of id p.
 * hu_overhang_columns: along every line of the axis from the top layer down to h0, support_dev <- for a sample not in S whose
 *   nearest sample of S above is an overhang, that overhang's id, 255 elsewhere; landing_dev <- the id of a sample of S with
 *   such a sample right above it, 255 elsewhere; counts_dev (129 uint64, the caller's zeros): [p] += the supported samples held
 *   by id p, [64 + p] += the landings id p owns, [128] += the supported samples in layer h0.  One atomic per accumulator and
 *   wavefront.
 * The three run in this order on one stream and read the word on the device: the host need not wait in between.  All allocate
 * nothing and synchronise nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL pointers, a
 * pitch that is no multiple of 16 or below dims[2], dims of 0 or above 65536, an axis above 2, reach_sq above
 * HU_OVERHANG_MAX_REACH_SQ, an `of` above 63 that is not HU_OVERHANG_SOLID, a word not aligned to 4 or counts not to 8 bytes. */
#define HU_OVERHANG_SOLID 255
#define HU_OVERHANG_MAX_REACH_SQ 8
int hu_overhang_first_layer(const void* ids_dev, uint32_t* word_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up,
                            uint32_t of, void* stream);
int hu_overhang_mark(const void* ids_dev, void* overhang_dev, uint32_t* word_dev, uint64_t* counts_dev, const uint32_t dims[3],
                     uint32_t pitch, int axis, int up, uint32_t reach_sq, uint32_t of, void* stream);
int hu_overhang_columns(const void* ids_dev, const void* overhang_dev, void* support_dev, void* landing_dev, uint32_t* word_dev,
                        uint64_t* counts_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, uint32_t of, void* stream);

/* ---- which part blocks which along a lattice axis (codecad_amd/disassembly.py) -----------------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device, with ids 0 .. n - 1 and 255 for a sample
 * inside no part (an id from n up counts as 255); the padding z in [dims[2], pitch) is not read.  A line of `axis` is the samples that agree on the other two
 * indices.  keys_dev is the KEY TABLE, uint64[3][HU_BLOCKING_MAX_PARTS][HU_BLOCKING_MAX_PARTS], which the caller sets to all
 * ones; a call lowers the entries [axis][i][j], i != j < n, to the least
 *   (q[axis] - p[axis]) << 48 | p.x << 32 | p.y << 16 | p.z
 * over the samples p of id i and q of id j on one line of the axis with q[axis] > p[axis]: the least distance from i up to j
 * and, among the p that attain it, the lexicographically first.  An entry no such p and q exist for stays all ones.  Keys are
 * lowered in a table in LDS per workgroup (n * n * 8 bytes, and n * 512 bytes of last indices for axis 0 and 1) and reach the
 * key table by at most one 64-bit atomic minimum per entry and workgroup, so calls for several axes may follow one another
 * on one stream without the host waiting in between.
 * Allocates nothing and synchronises nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL
 * pointers, a key table not aligned to 8 bytes, a pitch that is no multiple of 16 or below dims[2], dims of 0 or above 65536,
 * an axis outside 0..2, n outside 1..HU_BLOCKING_MAX_PARTS. */
#define HU_BLOCKING_MAX_PARTS 64
int hu_blocking_lines(const void* ids_dev, uint64_t* keys_dev, const uint32_t dims[3], uint32_t pitch, int axis, uint32_t n,
                      void* stream);

/* ---- which parts touch, over how many faces and where (codecad_amd/contacts.py) -----------------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device, with ids 0 .. n - 1 and 255 for a sample
 * inside no part (an id from n up counts as 255); the padding z in [dims[2], pitch) of either volume is neither read nor
 * written, and nothing outside the lattice is inside any part.  The FACE of axis a at sample p lies between p and p + e_a, both
 * in the lattice.  rows_dev is the ROW TABLE, hu_contact_row[3][HU_CONTACT_MAX_PARTS][HU_CONTACT_MAX_PARTS], which the caller
 * sets to zero: row [a][i][j], i != j < n, takes the samples p with id i whose neighbour p + e_a has id j,
 *   count += their number, sums[k] += their indices on axis k, hi[k] = the highest, not_lo[k] = ~(the lowest) of them,
 *   not_key = ~(the least p.x << 32 | p.y << 16 | p.z): the lexicographically first p,
 * so a row of zeros is an empty one and every update is an atomic add or an atomic maximum.  counts_dev is uint64[7][64], the
 * caller's zeros: [2 a][i] += the samples of id i whose neighbour p + e_a is empty or outside the lattice, [2 a + 1][i] += the
 * same with p - e_a, [6][i] += the INTERFACE SAMPLES of id i, those with an in-lattice 6-neighbour of another id that is not
 * 255.  contact_ids_dev, where not NULL, is a volume of the shape of ids_dev: the id on the interface samples, 255 elsewhere.
 * A wavefront writes a row only when the pair it meets changes or its walk ends, and adds its counts once at the end.
 * Allocates nothing and synchronises nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL
 * ids, rows, counts or dims, rows or counts not aligned to 8 bytes, a pitch that is no multiple of 16 or below dims[2], dims
 * of 0 or above 65536, n outside 1..HU_CONTACT_MAX_PARTS. */
#define HU_CONTACT_MAX_PARTS 64
typedef struct hu_contact_row {         /* 64 bytes */
    uint64_t count;
    uint64_t sums[3];
    uint64_t not_key;
    uint32_t not_lo[3];
    uint32_t hi[3];
} hu_contact_row;
int hu_contact_faces(const void* ids_dev, void* contact_ids_dev /* may be NULL */, void* rows_dev, uint64_t* counts_dev,
                     const uint32_t dims[3], uint32_t pitch, uint32_t n, void* stream);

/* ---- what an assembly holds when drained along a lattice axis (codecad_amd/drainage.py) ----------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device, aligned to 16 bytes for hu_drain_layers: E is
 * its samples z < dims[2] with id == 255, S those with another id; nothing outside the lattice is in S, and the padding z in [dims[2], pitch)
 * of any volume is neither read nor written as data.  Up runs along `axis` (up != 0: the layer of a sample is its index on that
 * axis; else dims[axis] - 1 - index), "below" is one layer less, the other two axes are the lateral ones.  labels_dev is
 * uint32[dims[0]][dims[1]][pitch], aligned to 4 bytes, dims[0] * dims[1] * pitch at most 2^31, under the invariant of the
 * component labelling above: an entry of a sample of E is the index into the buffer of a sample of its LAYER'S component (E
 * under the edges of the two lateral axes alone) that is not above its own, 0xffffffff outside E, and no call raises an entry.
 * Bit 31 of a root's entry is its ESCAPE FLAG.  The calls are made in this order on one stream:
 * hu_drain_layers: labels every layer at once: local != 0 in tiles of HU_COMPONENTS_TILE_X x _Y x _Z samples in LDS, then a
 *   merge across the tile faces of the two lateral axes; local == 0 from label = own index, a merge of every lateral pair.
 * hu_components_flatten (above): every entry becomes the index of its root.
 * hu_drain_seed: a sample of E in layer 0, or with a lateral index of 0 or dims - 1, sets the flag of its root.
 * hu_drain_rise: one PASS: walks every line of the axis from layer 0 up and sets the flag of the root of every sample of E
 *   whose sample below is in E under a flagged root, the flags it has set itself on the way included; stores 1 to *changed_dev
 *   (aligned to 4 bytes; the caller zeroes it before the call) when a flag was newly set.  The caller repeats the call until a
 *   pass leaves the word zero: at most dims[axis] + 1 passes.  The flagged roots are then those of the samples that ESCAPE.
 * hu_drain_floor: trapped_dev, a volume of the shape of ids_dev: on a sample of E whose root is not flagged the id of the
 *   nearest sample of S below it on its line (its FLOOR), 255 on every other sample of the lattice: every in-lattice byte is
 *   written.  counts_dev[p] (64 uint64, aligned to 8, the caller's zeros) += the samples written with id p (ids are 0..63 or
 *   255).  One atomic per accumulator and wavefront.
 * All allocate nothing and synchronise nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL
 * pointers, a pitch that is no multiple of 16 or below dims[2], dims of 0 or above 65536, an axis outside 0..2, more than 2^31
 * entries, ids not aligned to 16 (hu_drain_layers alone: hu_drain_floor reads bytes and takes ids_dev at any address), labels or
 * the word not to 4 or counts not to 8 bytes. */
int hu_drain_layers(const void* ids_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, int local,
                    void* stream);
int hu_drain_seed(void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, void* stream);
int hu_drain_rise(void* labels_dev, uint32_t* changed_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, void* stream);
int hu_drain_floor(const void* ids_dev, const void* labels_dev, void* trapped_dev, uint64_t* counts_dev, const uint32_t dims[3],
                   uint32_t pitch, int axis, int up, void* stream);

/* ---- what a print starts in mid-air: grounding from the plate (codecad_amd/islands.py) -----------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device, aligned to 16 bytes: S is its samples
 * z < dims[2] with id != 255 (of == HU_OVERHANG_SOLID) or id == of (of <= 63); nothing outside the lattice is in S, and the
 * padding z in [dims[2], pitch) of any volume is neither read nor written as data.  `axis`, `up`, the layers, "below" and the
 * lateral axes are those of the drain entry points above; h0 is the least layer that holds a sample of S, and word_dev the depth
 * word that hu_overhang_first_layer raised to dims[axis] - h0 (0: S is empty).  G, the GROUNDED samples, is the least subset
 * of S that holds every sample of S in layer h0 and every sample of S whose sample below or one of whose in-lattice lateral
 * neighbours is in G; F = S \ G FLOATS.  labels_dev is as for the drain entry points, over S in place of E, and bit 31 of a
 * root's entry says that its layer component is grounded.  The calls are made in this order on one stream:
 * hu_overhang_first_layer (above), with the caller's zeroed word and the same `of`.
 * hu_ground_layers: labels every layer of S at once: local != 0 in tiles of HU_COMPONENTS_TILE_X x _Y x _Z samples in LDS, then
 *   a merge across the tile faces of the two lateral axes; local == 0 from label = own index, a merge of every lateral pair.
 * hu_components_flatten (above): every entry becomes the index of its root.
 * hu_ground_seed: reads the word on the device; every sample of S in layer h0 sets the flag of its root, nothing else does.
 * hu_drain_rise (above), unchanged, repeated until a pass leaves its word zero: the flagged roots are then those of G.
 * hu_ground_mark: three volumes of the shape of ids_dev, every in-lattice byte of each written exactly once: floating_dev <- the
 *   id on F, start_dev <- the id on the samples of F whose sample below is not in S, join_dev <- the id on the samples of F
 *   whose sample above is in G, 255 elsewhere.  counts_dev (3 x 64 uint64, aligned to 8, the caller's zeros): [p] += the
 *   samples of F with id p, [64 + p] += the starts, [128 + p] += the joins.  One atomic per accumulator and wavefront.
 * All allocate nothing and synchronise nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL
 * pointers, a pitch that is no multiple of 16 or below dims[2], dims of 0 or above 65536, an axis outside 0..2, more than 2^31
 * entries (hu_ground_seed: exactly 2^31 with up == 0, where the flag of the last entry would read as 0xffffffff), an `of` above
 * 63 that is not HU_OVERHANG_SOLID, ids not aligned to 16, labels or the word not to 4 or counts not to 8 bytes. */
int hu_ground_layers(const void* ids_dev, void* labels_dev, const uint32_t dims[3], uint32_t pitch, int axis, uint32_t of,
                     int local, void* stream);
int hu_ground_seed(void* labels_dev, const uint32_t* word_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up,
                   void* stream);
int hu_ground_mark(const void* ids_dev, const void* labels_dev, void* floating_dev, void* start_dev, void* join_dev,
                   uint64_t* counts_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, uint32_t of, void* stream);

/* ---- what a 3-axis cutter along a lattice axis cannot reach (codecad_amd/tool_access.py) ---------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device, aligned to 16 bytes: S is its samples
 * z < dims[2] with id != 255 (of == HU_TOOL_SOLID) or id == of (of <= 63); nothing outside the lattice is in S, and the padding
 * z in [dims[2], pitch) of any volume is neither read as data nor written.  The spindle lies beyond the last layer of `axis`
 * and points at the table under layer 0 (up != 0: the layer of a sample is its index on that axis; else dims[axis] - 1 -
 * index).  A COLUMN (u, v) is a line of the axis, u < v the other two axes, nu and nv their dims; a 2D field is [nu][nv], v
 * fastest, aligned to 4 bytes.  The TOOL is the offsets D = {(du, dv) : du * du + dv * dv <= radius_sq}, K = isqrt(radius_sq),
 * and profile_dev, uint16[radius_sq + 1], non-decreasing from profile[0] = 0 (the caller's to ensure): g(du, dv) =
 * profile[du * du + dv * dv], how far above the tip the tool's underside lies.  The calls are made in this order on one stream:
 * hu_tool_tops: tops_dev[u][v] <- the KEY T * 256 + (255 - top id): T = 1 + the greatest layer of a sample of S on the column,
 *   top id that sample's id; 0 for a column without one.
 * hu_tool_dilate: tips_dev, uint32[nu + 2 K][nv + 2 K] with its origin at the column (-K, -K), <- Z(c) = the greatest
 *   T(c + n) - g(n) over n in D, T = 0 outside the lattice: the drop-cutter surface.  Workgroups of HU_TOOL_TILE x HU_TOOL_TILE
 *   columns with a halo of K in LDS.
 * hu_tool_erode: cut_dev[u][v] <- C * 256 + crowd: C(c) = the least Z(c - n) + g(n) over n in D, the closing of T by the tool;
 *   crowd = the top id of the greatest key among the columns c + n, n in D, inside the lattice, 255 when all those keys are 0.
 * hu_tool_rest: rest_dev, a volume of the shape of ids_dev, every in-lattice byte written once: on a sample not in S in a layer
 *   h < C(column), the id of the nearest sample of S above it on its line where h < T(column) (UNDERCUT), crowd(column)
 *   elsewhere (TIGHT); 255 on every other sample.  counts_dev (2 x 64 uint64, aligned to 8, the caller's zeros): [p] += the
 *   undercut samples with id p, [64 + p] += the tight ones.  One atomic per accumulator and wavefront.
 * All allocate nothing and synchronise nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL
 * pointers, a pitch that is no multiple of 16 or below dims[2], dims, nu or nv of 0 or above 65536, an axis outside 0..2, an
 * `of` above 63 that is not HU_TOOL_SOLID, radius_sq above HU_TOOL_MAX_RADIUS_SQ, ids or rest ids not aligned to 16, fields
 * not to 4, the profile not to 2 or counts not to 8 bytes. */
#define HU_TOOL_SOLID 255
#define HU_TOOL_MAX_RADIUS_SQ 1024
#define HU_TOOL_TILE 32
int hu_tool_tops(const void* ids_dev, uint32_t* tops_dev, const uint32_t dims[3], uint32_t pitch, int axis, int up, uint32_t of,
                 void* stream);
int hu_tool_dilate(const uint32_t* tops_dev, const uint16_t* profile_dev, uint32_t* tips_dev, uint32_t nu, uint32_t nv,
                   uint32_t radius_sq, void* stream);
int hu_tool_erode(const uint32_t* tips_dev, const uint32_t* tops_dev, const uint16_t* profile_dev, uint32_t* cut_dev, uint32_t nu,
                  uint32_t nv, uint32_t radius_sq, void* stream);
int hu_tool_rest(const void* ids_dev, const uint32_t* tops_dev, const uint32_t* cut_dev, void* rest_dev, uint64_t* counts_dev,
                 const uint32_t dims[3], uint32_t pitch, int axis, int up, uint32_t of, void* stream);

/* ---- shortest paths inside a set of the part-id volume (codecad_amd/flow_length.py) --------------
 * Over the id volume ids_dev, uint8[dims[0]][dims[1]][pitch], still on the device, at any address: S is its samples z < dims[2]
 * with id != 255 (of == HU_GEODESIC_SOLID), id == of (of <= 63) or id == 255 (of == HU_GEODESIC_EMPTY, this section's own code);
 * nothing outside the lattice is in S, and the padding z in [dims[2], pitch) of any volume is neither read nor written.  A STEP
 * joins two 6-neighbours that are both in S.  dist_dev is uint32[dims[0]][dims[1]][pitch], aligned to 4 bytes, dims[0] * dims[1]
 * * pitch at most 2^31: d of a sample, HU_GEODESIC_NONE where no seed reaches it and outside S.  The calls are made in this order
 * on one stream:
 * hu_geodesic_seed: writes EVERY in-lattice entry of dist_dev: 0 on a seed that is in S, HU_GEODESIC_NONE elsewhere.  The seeds
 *   are, by `mode`: HU_GEODESIC_BORDER the samples with an index of 0 or dims - 1 on some axis; HU_GEODESIC_LAYER those whose
 *   index on `axis` is `layer`; HU_GEODESIC_LIST the n_samples samples {x, y, z} of samples_dev, uint32[n_samples][3] on the
 *   device, aligned to 4 bytes (one outside the lattice or not in S seeds nothing: the caller's to refuse).  `axis` and `layer`
 *   are read under HU_GEODESIC_LAYER only, samples_dev and n_samples under HU_GEODESIC_LIST only.
 * hu_geodesic_sweep: one SWEEP: along every line of `axis` a forward walk and then a backward walk of the whole line.  The carry
 *   c is HU_GEODESIC_NONE at the start of a walk and after a sample outside S; on a sample of S v = min(dist, c + 1), the sum
 *   saturating at HU_GEODESIC_NONE, is stored where it is lower than dist, and c = v.  Entries outside S are neither read as data
 *   nor written.  The lines of an axis share no entry: the bytes after a call are those of the plain walks, whatever ran when.
 *   *word_dev (aligned to 4 bytes; the caller zeroes it) becomes nonzero when any entry was lowered, by at most one store per
 *   wavefront.  The caller repeats ROUNDS of three sweeps (axis 2, 1, 0 on one word) until a round leaves its word zero: dist is
 *   then the least number of steps from a seed, on every sample of S that a seed reaches.
 * hu_geodesic_stats: counts_dev, uint64[3][HU_GEODESIC_SLOTS], the caller's zeros: [0][p] += the samples of S with id p and
 *   d != HU_GEODESIC_NONE, [1][p] += those with d == HU_GEODESIC_NONE, [2][p] += the sum of d over the former; keys_dev,
 *   uint64[HU_GEODESIC_SLOTS], the caller's zeros: [p] is raised by a 64-bit atomic maximum to the greatest
 *   (d + 1) << 32 | (0xffffffff - q) over the former, q = (x * dims[1] + y) * pitch + z: the greatest d and the
 *   lexicographically first sample that has it; 0 while there is none.  Under HU_GEODESIC_EMPTY p is 64 for every sample.  One
 *   atomic per accumulator, wavefront and part.
 * All allocate nothing and synchronise nothing.  Every argument is checked before a device is touched (HU_ERR_BAD_ARG): NULL
 * pointers, a pitch that is no multiple of 16 or below dims[2], dims of 0 or above 65536, more than 2^31 entries, an `of` above
 * 63 that is neither HU_GEODESIC_SOLID nor HU_GEODESIC_EMPTY, an unknown mode, an axis outside 0..2, a layer from dims[axis] up,
 * n_samples outside 1..HU_GEODESIC_MAX_SAMPLES, distances, samples or the word not aligned to 4, keys or counts not to 8 bytes. */
#define HU_GEODESIC_SOLID 255
#define HU_GEODESIC_EMPTY 254
#define HU_GEODESIC_NONE 0xffffffffu
#define HU_GEODESIC_BORDER 0
#define HU_GEODESIC_LAYER 1
#define HU_GEODESIC_LIST 2
#define HU_GEODESIC_MAX_SAMPLES 65536
#define HU_GEODESIC_SLOTS 65
int hu_geodesic_seed(const void* ids_dev, void* dist_dev, const uint32_t dims[3], uint32_t pitch, uint32_t of, int mode, int axis,
                     uint32_t layer, const uint32_t* samples_dev, uint32_t n_samples, void* stream);
int hu_geodesic_sweep(const void* ids_dev, void* dist_dev, uint32_t* word_dev, const uint32_t dims[3], uint32_t pitch, int axis,
                      uint32_t of, void* stream);
int hu_geodesic_stats(const void* ids_dev, const void* dist_dev, uint64_t* keys_dev, uint64_t* counts_dev, const uint32_t dims[3],
                      uint32_t pitch, uint32_t of, void* stream);

/* ---- the surface meshes of an assembly's parts (codecad_amd/assembly_meshes.py) ----------------
 * The lattice of interference() with a ring of samples around it: samples carry the shifted index s = index + 1, 0 .. dims
 * per axis, and sit at corner + step * ((float)s - 1.0f) per axis in float32 (corner: the position of the sample (0, 0, 0) of
 * interference()).  dims counts the CUBES between them, per axis one more than the samples and at most 65536; cube (a, b, c)
 * has its corner m at the shifted index (a, b, c) + CORNERS[m] and the edges EDGES[e] of tools/gen_mc_table.py.  A list is
 * the cell list of the interference entry points, rows {a0 | b0 << 16, c0, mask lo, mask hi}: cubic cells of cubes.
 * windows_dev: n x 6 uint32 {lo a, b, c, hi a, b, c}, the cubes an instance may cross, inclusive.  step finite and not negative.
 * hu_mesh_cells: a cell of side 4 * child_side per parent row; each of its 4^3 children keeps a candidate k whose window
 *   reaches it and whose distance w at the child's centre (shifted index a + child_side / 2 per axis) is neither >= radius
 *   nor <= -radius, and is appended to children_dev when any remain.  child_side a power of two in 4..16384, radius not
 *   negative.
 * hu_mesh_leaf_instances: a cell of 4^3 cubes per parent row.  Every candidate k is evaluated at the cell's 5^3 samples;
 *   inside is w < 0; bit m of a cube's case is set when its corner m is inside.  An edge with exactly one end inside is
 *   crossed at t = w_p / (w_p - w_q) in correctly rounded float32, p the end with the lower lattice index, 0.5 where that is
 *   no number.  Each cube appends the triangles of its case (csrc/mc_table.hpp, in the table's order and winding) to
 *   triangles_dev as records of 32 bytes {a | b << 16, c | k << 16 | which << 24, case | e0 << 8 | e1 << 16 | e2 << 24, 0,
 *   float t0, t1, t2, 0}, in no particular order; `which` is the triangle's number within its case.  totals_dev: n + 1
 *   uint64, the number of records and the number per instance, added to; records at or past triangle_capacity are counted
 *   and not stored (triangles_dev may be NULL for a capacity of 0).
 * Both read the number of parents from *n_parents_dev and add the sample evaluations they perform (samples and children
 * past the lattice's rim not counted) to *evaluations_dev. */
int hu_mesh_cells(const hu_cells_launch* launch, const hu_cells_children* children);
int hu_mesh_leaf_instances(const hu_cells_launch* launch, void* triangles_dev, uint32_t triangle_capacity,
                           uint64_t* totals_dev);

/* ---- renderers on the same evaluate() -------------------- */
/* rendering/ray_caster.cl:146-159, launched by rendering/ray_caster.py:93-110 with global size
 * (width, height).  origin/forward/up/right: float4 as the reference passes them (forward already
 * scaled by the focal length; 4th component ignored).  render_options: bit0 false colour, bit1
 * zebra (ray_caster.cl:9-10).  out_dev: uchar[width*height*3], pixel (x, y) at (y + height*x)*3. */
int hu_ray_caster(hu_tape t, const float origin[4], const float forward[4], const float up[4],
                  const float right[4], float pixel_tolerance, float box_radius, float min_distance,
                  float max_distance, float floor_z, uint32_t render_options, uint32_t width,
                  uint32_t height, void* out_dev, void* stream);
/* The same ray caster over the instances of an assembly (codecad_amd/rendering/assembly_picture.py; the reference
 * renders an assembly as one union).  The table arguments are those of the interference entry points, from
 * hu_instance_table with full_programs = 1 (distance_only must be 0); then hu_ray_caster's.  The field at a point is the
 * least instance's value, the instance the LOWEST index that attains it.  colors_dev: n float4 {r, g, b, unused} in
 * [0, 1], the hue of each instance's flat colour ((0.7, 1, 0) is hu_ray_caster's).  out_dev as hu_ray_caster's;
 * part_ids_dev: int32[width*height], pixel (x, y) at y + height*x: the instance of the primary ray's last evaluation
 * where it hit, -1 where it did not; depth_dev: float[width*height], the distance along the primary ray where it hit,
 * +inf where not.  flags bit 0: evaluate every instance at every sample (else an instance whose last value and the
 * path travelled since prove that it cannot be the least is left out: the same bytes, |grad w| <= 1 assumed).
 * counters_dev: NULL, or two uint64 the launch adds to: instance programs run, instance programs asked for (samples x
 * n), both per wavefront.  Allocates nothing, synchronises nothing. */
int hu_ray_caster_instances(const void* table_dev, uint32_t n, int distance_only, uint32_t lane_bytes,
                            const float origin[4], const float forward[4], const float up[4], const float right[4],
                            float pixel_tolerance, float box_radius, float min_distance, float max_distance,
                            float floor_z, uint32_t render_options, uint32_t width, uint32_t height,
                            const void* colors_dev, void* out_dev, int32_t* part_ids_dev, float* depth_dev,
                            uint32_t flags, uint64_t* counters_dev, void* stream);
/* rendering/bitmap.cl:1-4, launched by rendering/bitmap.py:22-26: inside/outside picture of a 2D
 * shape, sample (x, y) at origin + step_size*(x, height-y-1).  out_dev as above. */
int hu_bitmap(hu_tape t, const float origin[4], float step_size, uint32_t width, uint32_t height,
              void* out_dev, void* stream);

/* ---- 2D contouring ----------------------------------------- */
/* rendering/polygon2d.cl:82-93, launched by rendering/polygon2d.py:101-112 with global size
 * grid = (gx-1, gy-1, 2) over the float4 corner samples corners_dev[gx*gy] that hu_grid_eval wrote
 * for dims (gx, gy, 1).  Per triangular half cell (index t + 2*(y + (gy-1)*x)): vertices_dev
 * float2[cells] (written where the contour crosses the cell), links_dev uint32[cells] (next cell
 * along the contour, 0xffffffff = empty cell, top bits = where it leaves the block,
 * polygon2d.cl:5-36), starts_dev uint32[(gx-1)+(gy-1)] + *start_counter_dev (caller zeroes): cells
 * that begin a chain entering through the block's boundary, in unspecified order. */
int hu_process_polygon(const float box_corner[2], float box_step, const void* corners_dev,
                       const uint32_t grid[2], void* vertices_dev, uint32_t* links_dev,
                       uint32_t* starts_dev, uint32_t* start_counter_dev, void* stream);
/* The same for ALL leaf blocks of a 2D subdivision in one launch (the per-block loop of
 * polygon2d.py:84-126).  corners_dev: float4[n_blocks][dims[0]*dims[1]] as written by
 * hu_grid_eval_blocks(layout 0) over dims (gx, gy, 1); block corner = (float)(int_corner *
 * resolution + origin).  Outputs are per block, consecutive; start_counters_dev: uint32[n_blocks]. */
int hu_process_polygon_blocks(const void* corners_dev, const int32_t* blocks_dev, uint32_t n_blocks,
                              double resolution, const double origin[3], float step,
                              const uint32_t dims[2], void* vertices_dev, uint32_t* links_dev,
                              uint32_t* starts_dev, uint32_t* start_counters_dev, void* stream);

/* ---- leaf-block consumer: marching cubes ------------------- */
/* Replaces the per-block copy + `mcubes.marching_cubes(block, 0)` of rendering/mesh.py:53-63 (PyMCubes
 * 0.0.6, a dependency that is not part of the reference tree) for ALL leaf blocks at once.
 * fields_dev: float[n_blocks][dims[0]*dims[1]*dims[2]], each block an array [A0][A1][A2] (last index
 * fastest), inside = value <= 0; for blocks written by hu_grid_eval_blocks(layout 1) over (sx, sy, sz)
 * samples pass dims = (sy, sx, sz).  The unit of work is a segment (up to 32 consecutive samples along
 * the last axis: a row of a 16^3 block), 256 segments per workgroup: hu_mesh_workgroups gives the
 * number n of workgroups, the number of (uint32, uint32) entries wg_counts_dev must hold (n + 1 + scan
 * scratch) and the total number of segments.
 * hu_mesh_count: masks_dev uint32[segments] <- one inside bit per sample; wg_counts_dev[0..n) <-
 * exclusive prefix of (vertices, triangles) per workgroup; entry n holds the totals (read it back to
 * size the outputs; block b starts at workgroup b*n/n_blocks).  Asynchronous.
 * hu_mesh_emit (same fields, masks and counts): vertices_dev double[total_vertices][3] in world
 * coordinates exactly as mesh.py:65-68 computes them (swap the first two array axes, negate y, * step,
 * + block corner, all in fp64; block corner = int_corner*resolution + origin), plus y_offset on y (0 =
 * the reference's placement, which sits (A0-1)*step below the true one; (A0-1)*step = true positions);
 * triangles_dev uint32[total_triangles][3], global vertex ids, anticlockwise seen from outside the solid;
 * seg_info_dev: scratch uint32[4*segments].  Order: vertices by owning sample then axis, triangles by
 * cell -- deterministic, no atomics.  At most 2^32 - 1 vertices per call. */
int hu_mesh_workgroups(uint32_t n_blocks, const uint32_t dims[3], uint64_t* n_workgroups,
                       uint64_t* count_entries, uint64_t* segments);
int hu_mesh_count(const float* fields_dev, uint32_t n_blocks, const uint32_t dims[3],
                  uint32_t* masks_dev, uint32_t* wg_counts_dev, void* stream);
int hu_mesh_emit(const float* fields_dev, const int32_t* blocks_dev, uint32_t n_blocks,
                 double resolution, const double origin[3], double step, const uint32_t dims[3],
                 double y_offset, const uint32_t* masks_dev, const uint32_t* wg_counts_dev,
                 uint32_t* seg_info_dev, double* vertices_dev, uint32_t* triangles_dev, void* stream);
/* Binary STL records of an indexed mesh (rendering/stl_renderer.py:8-24, which fills a numpy-stl 1.8.0 mesh
 * triangle by triangle on the host and saves it): records_dev (16-byte aligned, 50*n_triangles bytes) <-
 * per triangle the normal, the three corners -- vertices_dev rounded to float32 -- and a zero attribute
 * word, little endian, i.e. the body of the file after its 80-byte header and uint32 count.  normal =
 * (v1-v0) x (v2-v0) in float32, unnormalised, as numpy-stl's update_normals computes it on save.  Every
 * index in triangles_dev must be a valid vertex.  Asynchronous. */
int hu_mesh_stl(const double* vertices_dev, const uint32_t* triangles_dev, uint64_t n_triangles,
                void* records_dev, void* stream);

/* Order a list of integer block corners (int32[4] rows, e.g. the leaf list of hu_subdivision_level) by
 * (x, y, z) on the device, in place, so that per-block output comes out in a reproducible order (the
 * kernels append survivors in the order workgroups finished).  Two calls: with scratch_dev NULL (or too
 * small) only *needed is set; then with scratch_bytes >= *needed the list is sorted; synchronises the
 * stream.  Corners must lie within +-2^20 resolution units. */
int hu_sort_blocks(int32_t* blocks_dev, uint32_t n_blocks, void* scratch_dev, size_t scratch_bytes,
                   size_t* needed, void* stream);

/* Per-tape specialisation (the reference's generate_fixed_eval_source_code, nodes/codegen.py:137-204):
 * unroll the decoded program into straight-line gfx950 code with hipRTC, using the op library
 * headers found in `include_dir` (codecad_amd/csrc).  Afterwards every launch with this tape runs
 * the specialised kernels; results are identical to the interpreter's.  Costs one compilation
 * (seconds); returns HU_ERR_UNSUPPORTED with the compiler log if hipRTC cannot build it. */
int hu_tape_specialize(hu_tape t, const char* include_dir);
/* The same with an on-disk cache of the compiled code objects: `cache_dir` (NULL or "" = no cache) holds one
 * file per (generated source, op library headers, compiler options, hipRTC/HIP version); a hit loads in
 * milliseconds instead of compiling for seconds -- the counterpart of pyopencl's program cache behind the
 * reference's `Program(...).build()` (cl_util/opencl_manager.py:116-141).  The directory is created if its
 * parent exists; unreadable, truncated or stale files are ignored and rebuilt; an unwritable directory is not
 * an error.  only_if_cached != 0: load when cached, otherwise leave the tape interpreted and return HU_OK.
 * `*from_cache` (may be NULL) <- 1 if the kernels came from the cache. */
int hu_tape_specialize_cached(hu_tape t, const char* include_dir, const char* cache_dir,
                              int only_if_cached, int* from_cache);
/* The same for a subset of the per-tape KERNELS: bit i of `groups` is kernel i of the list below, and the HU_SPEC_*
 * constants are the sets a kind of launch needs (its FAMILY).  Compiling only what is about to be used takes a fraction
 * of the time of all nineteen kernels, and a tape's kernels may be built one by one, side by side in several processes
 * (round 4: a tape's first kernel is ready after its OWN compilation, not after its family's).  Kernels that are loaded
 * already are skipped; a launch whose kernel is not loaded runs the interpreter (a launch over boxes whose mask kernel is
 * not loaded yet treats every operand as alive: same bits).
 *   bit 0, 1    k_grid_eval (float4, float)            bit 10      k_box_masks (box pruning, every launch over boxes)
 *   bit 2, 3    k_grid_eval_blocks (float4, float)     bit 11, 12  k_grid_eval_ragged (float4, float)
 *   bit 4..7    k_classify ([MASS][BATCH])             bit 13, 14  k_grid_eval_blocks_ragged (float4, float)
 *   bit 8, 9    k_ray_caster, k_bitmap                 bit 15, 16  k_grid_eval_runs (float4, float)
 *   bit 17, 18  k_grid_eval_blocks_runs (float4, float)
 * (ragged: boxes that may end anywhere, for extents that are no multiples of (4, 4, 8); runs: the in-place form over runs of
 * cells, where boxes would be mostly padding -- 2D grids)
 * With a cache directory: the image of exactly the requested set is taken when it is there, else the images of its single
 * kernels (what the background builds leave behind); what is still missing is built as ONE image (only_if_cached = 0). */
enum hu_spec_group {
    HU_SPEC_DENSE = 0x19c03,    /* hu_grid_eval, hu_grid_eval_pymcubes, hu_grid_eval_slab */
    HU_SPEC_BLOCKS = 0x6640c,   /* hu_grid_eval_blocks[_indirect] */
    HU_SPEC_CLASSIFY = 0x04f0,  /* hu_subdivision_step / _level[_indirect], hu_mass_properties / _level[_indirect] */
    HU_SPEC_RENDER = 0x0300,    /* hu_ray_caster, hu_bitmap */
    HU_SPEC_ALL = 0x7ffff
};
int hu_tape_specialize_groups(hu_tape t, const char* include_dir, const char* cache_dir, int only_if_cached,
                              uint32_t groups, int* from_cache);
/* *out_flag <- the per-tape kernels that are loaded (hu_spec_group bits; 0: everything is interpreted) */
int hu_tape_specialized(hu_tape t, int* out_flag);
/* Box pruning of the tape's per-tape code (no counterpart in the reference, whose kernels evaluate every primitive for
 * every sample): *bits <- the operands of min / max that can be decided per 16^3 box of a launch (0: nothing in this tape
 * can be bounded, or it is interpreted), *words <- 32-bit words of a box's mask.  Launches over boxes run the tape's mask
 * kernel first, on their stream; HU_PRUNE=0 in the environment builds tapes without it.  Results are bit-identical either
 * way. */
int hu_tape_prune_info(hu_tape t, int* bits, int* words);
/* A precompiled header for the per-tape builds (host only): hipRTC's runtime header + the op library of `include_dir`,
 * made in `dir` by the clang++ that sits next to the hipRTC in use, if there is one; the builds then skip parsing those
 * ~16 000 lines (a quarter of a family's build, most of a small kernel's).  `path` (may be NULL) <- the file, or "" when
 * none could be made (no such clang, no libhiprtc-builtins.so, unwritable directory): the builds then run as before.
 * Two files, their paths separated by a newline: big sources are built with -O1 (HU_RTC_BIG_KB), and clang takes a header
 * only at the optimisation level it was made at.
 * The per-tape builds look for it in <directory of libhip_util.so>/pch (where the library's build puts it) and in their
 * cache directory (where they make it themselves when it is missing).  HU_RTC_PCH=0 switches it off.  No counterpart in
 * the reference (pyopencl's build has no headers to parse). */
int hu_spec_pch_prepare(const char* include_dir, const char* dir, char* path, size_t capacity);
/* The HIP source hu_tape_specialize would compile for this tape (host only, no device needed):
 * `*needed` receives its size including the terminator; it is copied when `capacity` suffices. */
int hu_tape_source(const float* tape, size_t n_floats, char* buf, size_t capacity, size_t* needed);
/* A readable listing of a tape's decoded programs, one record per line (host only, no device needed): which = 0 the
 * full program, 1 the distance-only program (empty for tapes with a rounded blend), 2 / 3 the same as the
 * interpreter runs them, transformed primitives fused into single records.  Same calling convention. */
int hu_tape_listing(const float* tape, size_t n_floats, int which, char* buf, size_t capacity, size_t* needed);
/* The tape's coordinate limit (host only, no device needed): per-tape code launched on samples whose |coordinates| all
 * stay below it skips the range tests of the fast square root in its rectangle and extrusion corners (a handle that
 * hu_tape_specialize made holds the same number, from the same analysis).  +inf: the tape has no such corner; 0: no
 * launch may skip them (a half extent below 2^-25, an op the analysis does not bound, a tape it does not cover). */
int hu_tape_coordinate_limit(const float* tape, size_t n_floats, double* out_limit);
/* Compile that source with hipRTC without loading it (host only, no device needed): checks that the
 * op library headers in `include_dir` build under hipRTC and that all ten kernels are present.
 * `*code_bytes` (may be NULL) receives the code object size. */
int hu_tape_compile_check(const float* tape, size_t n_floats, const char* include_dir, size_t* code_bytes);
/* The same through the cache of hu_tape_specialize_cached (host only): a miss compiles and stores, a hit
 * only reads.  `*from_cache` (may be NULL) <- 1 on a hit. */
int hu_tape_compile_cached(const float* tape, size_t n_floats, const char* include_dir,
                           const char* cache_dir, size_t* code_bytes, int* from_cache);
/* ... for a subset of the kernels (hu_spec_group bits), as ONE image named after the set */
int hu_tape_compile_groups(const float* tape, size_t n_floats, const char* include_dir, const char* cache_dir,
                           uint32_t groups, size_t* code_bytes, int* from_cache);

/* Device self-test of the arithmetic contract: the kernels compute sqrt(x) and 1/sqrt(x) with a
 * short hardware-seeded sequence instead of the compiler's IEEE expansion (csrc/interp.hpp
 * sqrt_cr / sqrt_inv_cr).  This runs both on ALL 2^32 binary32 inputs, one and two voxels per
 * lane, and counts disagreements with the IEEE results: counts[0..2] = mismatches of sqrt_cr,
 * sqrt_inv_cr's root, sqrt_inv_cr's reciprocal (all must be 0); counts[3] = inputs on the fast
 * path.  Synchronous, about 0.1 s. */
int hu_selftest_math(uint64_t counts[4]);
/* ... and of the three-operand minimum / maximum per-tape code uses for min(min(a, b), c) / max(max(a, b), c)
 * (csrc/interp.hpp min3_ / max3_): every ordered triple of 64 special values (zeros of both signs, denormals,
 * infinities, quiet and signalling NaNs) and 2^26 random triples, one and two voxels per lane, against the two
 * instructions they replace: counts[0], counts[1] = disagreements of min3, max3 (must be 0); counts[2] = triples.
 * Synchronous. */
int hu_selftest_minmax3(uint64_t counts[3]);

#ifdef __cplusplus
}
#endif
#endif /* HIP_UTIL_H */
