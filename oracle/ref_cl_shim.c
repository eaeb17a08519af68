/* oracle/ref_cl_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The host side of oracle/_ref/libref_polygon2d.so (recipe: oracle/ref_cl.py).  The reference's
 * rendering/polygon2d.cl is compiled as it stands, as OpenCL C, to an x86-64 object; it calls no
 * generated evaluate() and leaves six OpenCL builtins undefined.  This file, compiled as C by the
 * same clang (so that vector arguments travel alike), defines those six under their mangled names,
 * keeps the work-item ids in per-thread variables and runs the kernel once per work item of the
 * (gx-1, gy-1, 2) launch.  Nothing here restates the kernel.
 *
 * Arithmetic: dot is a.x*b.x + a.y*b.y in plain binary32 (REF_FMA_DOT: fma(a.x, b.x, a.y*b.y), one of
 * the roundings the OpenCL specification allows; only the README's measurement builds that).
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

typedef float cl_f2 __attribute__((ext_vector_type(2)));
typedef float cl_f4 __attribute__((ext_vector_type(4)));
typedef unsigned int cl_u2 __attribute__((ext_vector_type(2)));

static __thread size_t work_id[3], work_size[3];

size_t ref_get_global_id(unsigned int d) __asm__("_Z13get_global_idj");
size_t ref_get_global_size(unsigned int d) __asm__("_Z15get_global_sizej");
unsigned int ref_atomic_inc(volatile unsigned int *p) __asm__("_Z10atomic_incPU8CLglobalVj");
float ref_dot(cl_f2 a, cl_f2 b) __asm__("_Z3dotDv2_fS_");
cl_f2 ref_convert_float2(cl_u2 v) __asm__("_Z14convert_float2Dv2_j");
float ref_fabs(float x) __asm__("_Z4fabsf");

/* OpenCL 1.2 6.12.1: an id of a dimension the launch does not have is 0, its size 1 */
size_t ref_get_global_id(unsigned int d) { return d < 3 ? work_id[d] : 0; }
size_t ref_get_global_size(unsigned int d) { return d < 3 ? work_size[d] : 1; }
/* the work items run one after another */
unsigned int ref_atomic_inc(volatile unsigned int *p) { return (*p)++; }
float ref_dot(cl_f2 a, cl_f2 b)
{
#ifdef REF_FMA_DOT
    return __builtin_fmaf(a.x, b.x, a.y * b.y);
#else
    return a.x * b.x + a.y * b.y;
#endif
}
cl_f2 ref_convert_float2(cl_u2 v) { return (cl_f2){ (float)v.x, (float)v.y }; }
float ref_fabs(float x) { return __builtin_fabsf(x); }

/* the kernel of the reference, defined by the object compiled from its own file */
void process_polygon(cl_f2 box_corner, float box_step, cl_f4 *corners, cl_f2 *vertices, unsigned int *links,
                     unsigned int *starts, unsigned int *start_counter);

/* corners: float4[gx*gy], index y + gy*x.  vertices: float2[cells], links: uint[cells], cells = (gx-1)*(gy-1)*2;
 * starts: room for every half cell on the boundary, 2*((gx-1)+(gy-1)) is always enough.  Vertices are
 * prefilled with 0xff bytes: the kernel does not write those of empty cells. */
int ref_process_polygon(const float corner[2], float step, const float *corners, uint32_t gx, uint32_t gy, float *vertices,
                        uint32_t *links, uint32_t *starts, uint32_t *counter)
{
    if (gx < 2 || gy < 2) return -1;
    const size_t cells = (size_t)(gx - 1) * (gy - 1) * 2;
    memset(vertices, 0xff, cells * 2 * sizeof(float));
    *counter = 0;
    work_size[0] = gx - 1;
    work_size[1] = gy - 1;
    work_size[2] = 2;
    const cl_f2 c = { corner[0], corner[1] };
    for (size_t x = 0; x < work_size[0]; ++x)
        for (size_t y = 0; y < work_size[1]; ++y)
            for (size_t t = 0; t < 2; ++t) {
                work_id[0] = x;
                work_id[1] = y;
                work_id[2] = t;
                process_polygon(c, step, (cl_f4 *)corners, (cl_f2 *)vertices, links, starts, counter);
            }
    return 0;
}
