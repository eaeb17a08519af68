// tools/experiments/store_patterns.hip -- STORES ALONE: a 512^3 float4 grid (2 GiB, z fastest, then y, then x -- the layout
// grid_eval's ABI fixes) written by workgroups of 256 lanes in different orders, nothing else in the kernels.  The question
// (DESIGN.md section 5.1): the dense kernel over 16^3 boxes is held at 0.39 ms by its store stream where runs along z reach
// 0.32 ms -- is it the 128-byte segments, the 256-byte rows of a box, or the footprint of the boxes in flight?
// Second part ("what separates boxes from runs"): arms that change ONE thing from an anchor -- the
// bytes a workgroup owns (runs of 1024 ... 4096 voxels, boxes of 512 and 1024), the order in time inside a 16^3 box (the
// four wavefronts on four columns, or abreast on one x slice), the order over workgroups (chunks of the box list dealt to
// the XCDs in eighths, the walk inside an eighth, groups of boxes), the occupancy, and grids whose strides are no powers of
// two -- each measured like bench.py's hbm_regime (forty warm launches, events around ten), in rounds, with the two anchors
// ("runs along z", "boxes 16^3, order 1") measured again before every arm.
// Usage: store_patterns [reps of the first part, 0 skips it] [rounds of the second part, 0 skips it]
// Build: hipcc -O3 --offload-arch=gfx950 -o tools/experiments/build/store_patterns tools/experiments/store_patterns.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <functional>
#include <string>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr uint32_t N = 512;

__device__ __forceinline__ float4 value(uint32_t x, uint32_t y, uint32_t z) { return make_float4((float)x, (float)y, (float)z, 1.0f); }

// runs along z: a workgroup writes 512 consecutive voxels (two per lane, 64 lanes apart)
__global__ void __launch_bounds__(256) k_runs(float4* out)
{
    const size_t base = (size_t)blockIdx.x * 512u;
    for (int i = 0; i < 2; ++i) {
        const size_t lin = base + (threadIdx.x & 63u) + 128u * (threadIdx.x >> 6) + 64u * i;
        out[lin] = value((uint32_t)(lin >> 18), (uint32_t)(lin >> 9) & 511u, (uint32_t)lin & 511u);
    }
}

// a box of BX x BY x BZ voxels per workgroup (4096 voxels), a lane walks along x; a wavefront's store instruction covers
// LZ voxels along z, 64 / LZ / LX rows along y and LX planes (LX = 2: the second voxel of a lane two planes on, as box_eval)
template <int BX, int BY, int BZ, int LZ, int ORDER>
__global__ void __launch_bounds__(256) k_boxes(float4* out)
{
    constexpr uint32_t nbx = N / BX, nby = N / BY, nbz = N / BZ;
    uint32_t b = blockIdx.x;
    if (ORDER == 1) {   // contiguous chunks per XCD (workgroup i runs on XCD i % 8)
        const uint32_t per = (nbx * nby * nbz) / 8u;
        b = (b & 7u) * per + (b >> 3);
    }
    uint32_t qz, qy, qx;
    if (ORDER == 2) { qx = b % nbx; qz = (b / nbx) % nbz; qy = b / (nbx * nbz); }   // x fastest
    else { qz = b % nbz; qy = (b / nbz) % nby; qx = b / (nbz * nby); }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the (y, z) face of the box: BY x BZ columns, 64 * 4 lanes x ... each lane takes columns so that a wavefront covers
    // LZ along z and 32 / LZ (x 2 planes) or 64 / LZ rows
    constexpr uint32_t rows_per_wave = 32u / LZ;            // with two planes per instruction
    constexpr uint32_t cols = BY * BZ;                       // columns of the face
    constexpr uint32_t per_wave_cols = rows_per_wave * LZ;   // columns a wavefront covers at once (32)
    const uint32_t lz = lane % LZ, ly = (lane / LZ) % rows_per_wave, lx = lane / 32u;
    for (uint32_t c = wave * per_wave_cols; c < cols; c += 4u * per_wave_cols) {
        // tile of the face: LZ along z, rows_per_wave along y
        const uint32_t tiles_z = BZ / LZ;
        const uint32_t tile = c / per_wave_cols;
        const uint32_t z = (tile % tiles_z) * LZ + lz, y = (tile / tiles_z) * rows_per_wave + ly;
        for (uint32_t x = lx; x < BX; x += 4u) {
            for (uint32_t i = 0; i < 2u; ++i) {
                const uint32_t X = qx * BX + x + 2u * i, Y = qy * BY + y, Z = qz * BZ + z;
                out[((size_t)X * N + Y) * N + Z] = value(X, Y, Z);
            }
        }
    }
}

// ---- second part: one generic kernel per family, grid extents at run time ----
struct Grid { uint32_t nx, ny, nz; };
// ORDER OVER WORKGROUPS.  The box list (as `walk` numbers it) is cut into chunks of `chunk` boxes, taken one after the
// other by `chunk` consecutive workgroups; inside a chunk XCD k (workgroup i runs on XCD i % 8) takes a contiguous eighth.
// chunk >= boxes: order 1 of the first part; chunk = 8: launch order; chunk = the boxes of one or two x slabs: what the
// whole chip has in flight tiles whole slabs.  A bijection for any count and any chunk.
// walk 0: z fastest, then y, then x; 1: y fastest, then z, then x; 2: groups of gx x gy x gz boxes (z fastest inside a
// group and over the groups; the box counts must be multiples of the group's)
struct Order { uint32_t chunk, walk, gx, gy, gz; };
__device__ __forceinline__ uint32_t chunked(uint32_t g, uint32_t total, uint32_t chunk)
{
    const uint32_t t0 = g / chunk * chunk, n = min(chunk, total - t0), l = g - t0;
    const uint32_t k = l & 7u, q = n >> 3, r = n & 7u;
    return t0 + k * q + min(k, r) + (l >> 3);
}
__device__ __forceinline__ void box_of(uint32_t b, const Order& o, uint32_t nbx, uint32_t nby, uint32_t nbz, uint32_t& qx, uint32_t& qy, uint32_t& qz)
{
    if (o.walk == 1u) { qy = b % nby; qz = (b / nby) % nbz; qx = b / (nby * nbz); }
    else if (o.walk == 2u) {
        const uint32_t gs = o.gx * o.gy * o.gz, G = b / gs, w = b % gs, ngz = nbz / o.gz, ngy = nby / o.gy;
        qz = (G % ngz) * o.gz + w % o.gz; qy = ((G / ngz) % ngy) * o.gy + (w / o.gz) % o.gy; qx = (G / (ngz * ngy)) * o.gx + w / (o.gz * o.gy);
    } else { qz = b % nbz; qy = (b / nbz) % nby; qx = b / (nbz * nby); }
}

// runs along z of V voxels per workgroup, a wavefront on a contiguous quarter (V = 512: k_runs)
template <int V>
__global__ void __launch_bounds__(256) k_runs_v(float4* out, Grid g)
{
    const size_t base = (size_t)blockIdx.x * V + (threadIdx.x >> 6) * (V / 4) + (threadIdx.x & 63u);
#pragma unroll
    for (int i = 0; i < V / 256; ++i) {
        const size_t lin = base + 64u * i;
        const uint32_t z = (uint32_t)(lin % g.nz), y = (uint32_t)((lin / g.nz) % g.ny), x = (uint32_t)(lin / ((size_t)g.nz * g.ny));
        out[lin] = value(x, y, z);
    }
}

// a box of BX x BY x BZ voxels per workgroup in BRICKS: a wavefront's store instruction covers LZ voxels along z, 32 / LZ
// rows and two planes, its second instruction the planes two on (k_boxes, box_eval) -- 4 x (32 / LZ) x LZ voxels.
// ABREAST = 0: a wavefront takes a (y, z) column of bricks and walks it along x, then the column four on (box_eval today:
// a workgroup writes into up to sixteen planes at a time); 1: the four wavefronts take the bricks of one x slice side by
// side and step along x together (16^3: all sixteen rows of four planes, then the next four)
template <int BX, int BY, int BZ, int LZ, int ABREAST>
__global__ void __launch_bounds__(256) k_arm(float4* out, Grid g, Order o)
{
    constexpr uint32_t RY = 32u / LZ, tiles_z = BZ / LZ, tiles_y = BY / RY, cols = tiles_z * tiles_y, slices = BX / 4u, bricks = cols * slices;
    static_assert(BZ % LZ == 0 && BY % RY == 0 && BX % 4 == 0 && bricks % 4u == 0u && (ABREAST || cols % 4u == 0u), "bricks must tile the box and split over four wavefronts");
    const uint32_t nbx = g.nx / BX, nby = g.ny / BY, nbz = g.nz / BZ;
    uint32_t qx, qy, qz;
    box_of(chunked(blockIdx.x, gridDim.x, o.chunk), o, nbx, nby, nbz, qx, qy, qz);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lz = lane % LZ, ly = (lane / LZ) % RY, lx = lane / 32u;
    const auto brick = [&](uint32_t col, uint32_t slice) {
        const uint32_t Z = qz * BZ + (col % tiles_z) * LZ + lz, Y = qy * BY + (col / tiles_z) * RY + ly;
#pragma unroll
        for (uint32_t i = 0; i < 2u; ++i) {
            const uint32_t X = qx * BX + slice * 4u + lx + 2u * i;
            out[((size_t)X * g.ny + Y) * g.nz + Z] = value(X, Y, Z);
        }
    };
    if (ABREAST) {
        for (uint32_t t = wave; t < bricks; t += 4u) brick(t % cols, t / cols);
    } else {
        for (uint32_t col = wave; col < cols; col += 4u)
            for (uint32_t s = 0; s < slices; ++s) brick(col, s);
    }
}

template <class F> float time_it(F launch, int reps)
{
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    for (int i = 0; i < 3; ++i) launch();
    std::vector<float> ms;
    for (int r = 0; r < reps; ++r) {
        hipEventRecord(a, 0);
        launch();
        hipEventRecord(b, 0);
        hipEventSynchronize(b);
        float t = 0; hipEventElapsedTime(&t, a, b); ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int check(float4* out, std::vector<float4>& host, const char* name)
{
    // every voxel written with its own coordinates? (a sample of planes)
    for (uint32_t x : {0u, 17u, 255u, 511u}) {
        if (hipMemcpy(host.data(), out + (size_t)x * N * N, (size_t)N * N * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t z = 0; z < N; ++z) {
                const float4 v = host[(size_t)y * N + z];
                if (v.x != (float)x || v.y != (float)y || v.z != (float)z) { std::printf("%s: wrong voxel at %u %u %u\n", name, x, y, z); return 1; }
            }
    }
    return 0;
}

#define RUN_BOX(BX, BY, BZ, LZ, ORDER) RUN_BOX_LDS(BX, BY, BZ, LZ, ORDER, 0)
// LDS: dynamic shared memory the kernel never touches -- it only limits the workgroups (of four wavefronts) per CU: 160 KiB / LDS
#define RUN_BOX_LDS(BX, BY, BZ, LZ, ORDER, LDS)                                                                                 \
    do {                                                                                                                        \
        CHECK(hipMemset(out, 0xff, bytes));                                                                                     \
        const float ms = time_it([&] { hipLaunchKernelGGL((k_boxes<BX, BY, BZ, LZ, ORDER>), dim3(boxes), dim3(256), LDS, 0, out); }, reps); \
        char name[112]; std::snprintf(name, sizeof name, "boxes %2d x %2d x %3d, %2d voxels along z per store, order %d, %2d KiB LDS", BX, BY, BZ, LZ, ORDER, LDS / 1024); \
        if (check(out, host, name)) return 1;                                                                                   \
        std::printf("%-70s %.4f ms  %.2f TB/s\n", name, ms, bytes / ms * 1e-9);                                                \
    } while (0)

int first_part(float4* out, std::vector<float4>& host, int reps)
{
    const size_t bytes = (size_t)N * N * N * sizeof(float4);
    const uint32_t boxes = N * N * N / 4096u;
    {
        CHECK(hipMemset(out, 0xff, bytes));
        const float ms = time_it([&] { hipLaunchKernelGGL(k_runs, dim3(N * N * N / 512u), dim3(256), 0, 0, out); }, reps);
        if (check(out, host, "runs")) return 1;
        std::printf("%-70s %.4f ms  %.2f TB/s\n", "runs along z (512 voxels per workgroup)", ms, bytes / ms * 1e-9);
    }
    for (int lds : {16, 27, 32, 40, 53, 64}) {      // 10, 5 (6 would be 26.6), 5, 4, 3, 2 workgroups per CU
        const float ms = time_it([&] { hipLaunchKernelGGL(k_runs, dim3(N * N * N / 512u), dim3(256), lds * 1024, 0, out); }, reps);
        std::printf("runs along z, %2d KiB of idle LDS per workgroup %31s %.4f ms  %.2f TB/s\n", lds, "", ms, bytes / ms * 1e-9);
    }
    RUN_BOX_LDS(16, 16, 16, 8, 0, 27 * 1024);
    RUN_BOX_LDS(16, 16, 16, 8, 0, 32 * 1024);
    RUN_BOX_LDS(16, 16, 16, 8, 0, 40 * 1024);
    RUN_BOX_LDS(16, 16, 16, 8, 0, 53 * 1024);
    RUN_BOX_LDS(16, 16, 16, 8, 0, 64 * 1024);
    RUN_BOX_LDS(16, 16, 16, 8, 1, 40 * 1024);
    RUN_BOX_LDS(16, 16, 16, 16, 0, 40 * 1024);
    RUN_BOX_LDS(16, 4, 64, 32, 0, 40 * 1024);
    RUN_BOX_LDS(8, 8, 64, 32, 0, 40 * 1024);
    RUN_BOX(16, 16, 16, 8, 0);     // box_eval today: 128-byte segments, 16^3 boxes, z fastest box order
    RUN_BOX(16, 16, 16, 16, 0);    // 256-byte segments
    RUN_BOX(16, 16, 16, 8, 1);     // contiguous chunks per XCD
    RUN_BOX(16, 16, 16, 8, 2);     // x fastest box order
    RUN_BOX(16, 8, 32, 8, 0);
    RUN_BOX(16, 8, 32, 32, 0);
    RUN_BOX(16, 4, 64, 16, 0);
    RUN_BOX(16, 4, 64, 32, 0);
    RUN_BOX(16, 2, 128, 32, 0);
    RUN_BOX(8, 8, 64, 32, 0);
    RUN_BOX(8, 4, 128, 32, 0);
    RUN_BOX(4, 16, 64, 32, 0);
    RUN_BOX(16, 4, 64, 32, 1);
    RUN_BOX(16, 4, 64, 32, 2);
    RUN_BOX(32, 2, 64, 32, 0);
    RUN_BOX(64, 1, 64, 32, 0);
    return 0;
}

// ---- second part ----
struct Arm {
    std::string name;
    Grid g;
    std::function<void()> launch;
    std::vector<float> ms, vs_box;      // per round: its time, and that over the box anchor's measured just before it
};

// as bench.py's hbm_regime: forty warm launches, then events around ten back to back
float measure(const std::function<void()>& launch)
{
    static hipEvent_t a = nullptr, b = nullptr;
    if (!a) { hipEventCreate(&a); hipEventCreate(&b); }
    for (int i = 0; i < 40; ++i) launch();
    hipEventRecord(a, 0);
    for (int i = 0; i < 10; ++i) launch();
    hipEventRecord(b, 0);
    hipEventSynchronize(b);
    float t = 0;
    hipEventElapsedTime(&t, a, b);
    return t / 10.0f;
}

int check_grid(const float4* out, std::vector<float4>& host, const Grid& g, const char* name)
{
    for (uint32_t x : {0u, 17u, g.nx / 2u - 1u, g.nx - 1u}) {
        if (hipMemcpy(host.data(), out + (size_t)x * g.ny * g.nz, (size_t)g.ny * g.nz * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (uint32_t y = 0; y < g.ny; ++y)
            for (uint32_t z = 0; z < g.nz; ++z) {
                const float4 v = host[(size_t)y * g.nz + z];
                if (v.x != (float)x || v.y != (float)y || v.z != (float)z) { std::printf("%s: wrong voxel at %u %u %u\n", name, x, y, z); return 1; }
            }
    }
    return 0;
}

struct Stats { float lo, med, hi; };
Stats stats(std::vector<float> v)
{
    std::sort(v.begin(), v.end());
    return {v.front(), v[v.size() / 2], v.back()};
}

template <int V> Arm runs_arm(float4* out, Grid g, uint32_t lds)
{
    char name[128];
    std::snprintf(name, sizeof name, "runs along z, %4d voxels per workgroup, %2u KiB LDS, grid %u x %u x %u", V, lds / 1024u, g.nx, g.ny, g.nz);
    const uint32_t groups = (uint32_t)((size_t)g.nx * g.ny * g.nz / V);
    return {name, g, [=] { hipLaunchKernelGGL((k_runs_v<V>), dim3(groups), dim3(256), lds, 0, out, g); }, {}, {}};
}
template <int BX, int BY, int BZ, int LZ, int ABREAST> Arm box_arm(float4* out, Grid g, Order o, const char* order_name, uint32_t lds)
{
    char name[160];
    std::snprintf(name, sizeof name, "boxes %2d x %2d x %2d, %2d along z per store, %s, %s, %2u KiB LDS, grid %u x %u x %u", BX, BY, BZ, LZ,
                  ABREAST ? "abreast" : "columns", order_name, lds / 1024u, g.nx, g.ny, g.nz);
    const uint32_t nbx = g.nx / BX, nby = g.ny / BY, nbz = g.nz / BZ;
    if (g.nx % BX || g.ny % BY || g.nz % BZ || (o.walk == 2u && (nbx % o.gx || nby % o.gy || nbz % o.gz))) { std::printf("%s: does not tile\n", name); std::exit(1); }
    return {name, g, [=] { hipLaunchKernelGGL((k_arm<BX, BY, BZ, LZ, ABREAST>), dim3(nbx * nby * nbz), dim3(256), lds, 0, out, g, o); }, {}, {}};
}

int second_part(float4* out, std::vector<float4>& host, int rounds)
{
    const Grid G{N, N, N}, Gz{N, N, 496}, Gy{N, 496, N};
    constexpr uint32_t ALL = 1u << 30, K = 1024u;
    const Order o1{ALL, 0, 1, 1, 1};     // order 1 of the first part: a contiguous eighth of the boxes per XCD, z fastest
    const uint32_t boxes = N * N * N / 4096u;
    const std::function<void()> anchor_runs = [=] { hipLaunchKernelGGL(k_runs, dim3(N * N * N / 512u), dim3(256), 0, 0, out); };
    const std::function<void()> anchor_box = [=] { hipLaunchKernelGGL((k_boxes<16, 16, 16, 8, 1>), dim3(boxes), dim3(256), 0, 0, out); };
    std::vector<Arm> arms;
    // controls: the generic kernels as the anchors
    arms.push_back(runs_arm<512>(out, G, 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, o1, "order 1", 0));
    // (a) the bytes a workgroup owns, apart from the pattern
    arms.push_back(runs_arm<1024>(out, G, 0));
    arms.push_back(runs_arm<2048>(out, G, 0));
    arms.push_back(runs_arm<4096>(out, G, 0));
    arms.push_back(box_arm<8, 8, 8, 8, 1>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<4, 4, 32, 8, 1>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<4, 4, 32, 32, 1>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<4, 8, 16, 8, 1>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<4, 8, 16, 16, 1>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<8, 8, 16, 8, 0>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<8, 8, 16, 16, 1>(out, G, o1, "order 1", 0));
    // (b) the order in time inside a 16^3 box
    arms.push_back(box_arm<16, 16, 16, 8, 1>(out, G, o1, "order 1", 0));
    arms.push_back(box_arm<16, 16, 16, 16, 1>(out, G, o1, "order 1", 0));
    // (c) the order over workgroups
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{ALL, 1, 1, 1, 1}, "eighths walked y fastest", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{ALL, 2, 2, 2, 2}, "eighths in groups 2 x 2 x 2", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{ALL, 2, 4, 4, 1}, "eighths in groups 4 x 4 x 1", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{ALL, 2, 1, 4, 4}, "eighths in groups 1 x 4 x 4", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{8, 0, 1, 1, 1}, "launch order", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{256, 0, 1, 1, 1}, "chunks of 1/4 x slab", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{512, 0, 1, 1, 1}, "chunks of 1/2 x slab", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{1024, 0, 1, 1, 1}, "chunks of 1 x slab", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{2048, 0, 1, 1, 1}, "chunks of 2 x slabs (the chip's residents)", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{4096, 0, 1, 1, 1}, "chunks of 4 x slabs", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 1>(out, G, Order{1024, 0, 1, 1, 1}, "chunks of 1 x slab", 0));
    arms.push_back(box_arm<16, 16, 16, 8, 1>(out, G, Order{2048, 0, 1, 1, 1}, "chunks of 2 x slabs (the chip's residents)", 0));
    arms.push_back(box_arm<8, 8, 8, 8, 1>(out, G, Order{4096, 0, 1, 1, 1}, "chunks of 1 x slab", 0));
    arms.push_back(box_arm<8, 8, 8, 8, 1>(out, G, Order{2048, 0, 1, 1, 1}, "chunks of 1/2 x slab (the chip's residents)", 0));
    // (d) occupancy: LDS the kernel never touches (32 / 40 / 53 KiB: 5 / 4 / 3 workgroups per CU)
    for (uint32_t lds : {32u, 40u, 53u}) {
        arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, o1, "order 1", lds * K));
        arms.push_back(box_arm<16, 16, 16, 8, 1>(out, G, o1, "order 1", lds * K));
        arms.push_back(box_arm<16, 16, 16, 8, 0>(out, G, Order{1024, 0, 1, 1, 1}, "chunks of 1 x slab", lds * K));
        arms.push_back(box_arm<16, 16, 16, 8, 1>(out, G, Order{1024, 0, 1, 1, 1}, "chunks of 1 x slab", lds * K));
        arms.push_back(box_arm<8, 8, 8, 8, 1>(out, G, o1, "order 1", lds * K));
        arms.push_back(box_arm<8, 8, 16, 8, 0>(out, G, o1, "order 1", lds * K));
    }
    // (e) strides that are no powers of two (times per byte: the column "per 2 GiB")
    for (const Grid& g : {Gz, Gy}) {
        arms.push_back(runs_arm<512>(out, g, 0));
        arms.push_back(box_arm<16, 16, 16, 8, 0>(out, g, o1, "order 1", 0));
        arms.push_back(box_arm<16, 16, 16, 8, 1>(out, g, o1, "order 1", 0));
        arms.push_back(box_arm<16, 16, 16, 8, 0>(out, g, Order{(g.ny / 16u) * (g.nz / 16u), 0, 1, 1, 1}, "chunks of 1 x slab", 0));
        arms.push_back(box_arm<8, 8, 8, 8, 1>(out, g, o1, "order 1", 0));
    }

    const double full = (double)N * N * N * sizeof(float4);
    for (Arm& a : arms) {       // every voxel written with its own coordinates?
        if (hipMemset(out, 0xff, (size_t)full) != hipSuccess) return 1;
        a.launch();
        if (check_grid(out, host, a.g, a.name.c_str())) return 1;
    }
    std::vector<float> runs_ms, box_ms;
    for (int r = 0; r < rounds; ++r)
        for (Arm& a : arms) {
            runs_ms.push_back(measure(anchor_runs));
            box_ms.push_back(measure(anchor_box));
            a.ms.push_back(measure(a.launch));
            a.vs_box.push_back(a.ms.back() / box_ms.back());
        }
    const Stats sr = stats(runs_ms), sb = stats(box_ms);
    std::printf("\n# second part: %d rounds; per arm forty warm launches, then the average of ten; both anchors measured before every arm\n", rounds);
    std::printf("# anchor, runs along z (512 voxels per workgroup):   median %.4f ms, min %.4f, max %.4f, spread %.4f over %zu measurements\n", sr.med, sr.lo, sr.hi, sr.hi - sr.lo, runs_ms.size());
    std::printf("# anchor, boxes 16^3, order 1:                       median %.4f ms, min %.4f, max %.4f, spread %.4f over %zu measurements\n", sb.med, sb.lo, sb.hi, sb.hi - sb.lo, box_ms.size());
    std::printf("# an arm counts if its median is below the box anchor's by more than twice that spread: below %.4f ms per 2 GiB\n", sb.med - 2.0f * (sb.hi - sb.lo));
    std::printf("%-112s %8s %8s %8s %7s %10s %8s\n", "# arm", "median", "min", "max", "TB/s", "per 2 GiB", "vs box");
    for (const Arm& a : arms) {
        const Stats s = stats(a.ms), v = stats(a.vs_box);
        const double bytes = (double)a.g.nx * a.g.ny * a.g.nz * sizeof(float4);
        std::printf("%-112s %8.4f %8.4f %8.4f %7.2f %10.4f %8.3f\n", a.name.c_str(), s.med, s.lo, s.hi, bytes / s.med * 1e-9, s.med * full / bytes, v.med);
    }
    return 0;
}

int main(int argc, char** argv)
{
    const int reps = argc > 1 ? std::atoi(argv[1]) : 15, rounds = argc > 2 ? std::atoi(argv[2]) : 3;
    float4* out = nullptr;
    CHECK(hipMalloc((void**)&out, (size_t)N * N * N * sizeof(float4)));
    std::vector<float4> host((size_t)N * N);
    int rc = 0;
    if (reps > 0) rc = first_part(out, host, reps);
    if (rc == 0 && rounds > 0) rc = second_part(out, host, rounds);
    hipFree(out);
    return rc;
}
