// pt_refit_device.h -- the device helpers of the bottom-up refit (pt_lbvh_gpu.hip: the scheme's description is there), shared with the
// kernels that refit a lane's tree from a published pose (pt_publish.hip).  Every function is inlined: a kernel that uses them compiles
// to what it compiled to when they stood in its own file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pt_api.h"

namespace pt {

namespace {

// order-preserving float <-> uint mapping for atomicMin / atomicMax
__device__ __forceinline__ uint32_t f2ord(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}

__device__ __forceinline__ void leaf_box(const float4 s, float pad, float lo[3], float hi[3])
{
    lo[0] = s.x - s.w - pad; lo[1] = s.y - s.w - pad; lo[2] = s.z - s.w - pad;
    hi[0] = s.x + s.w + pad; hi[1] = s.y + s.w + pad; hi[2] = s.z + s.w + pad;
}

__device__ __forceinline__ void child_box(const float4* __restrict__ sorted, const PtBvhNode* nodes, int c, float pad, float lo[3], float hi[3])
{
    if (c < 0) {
        leaf_box(sorted[~c], pad, lo, hi);
    } else {
        const PtBvhNode* nd = &nodes[c];
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = fminf(nd->lo0[a], nd->lo1[a]); hi[a] = fmaxf(nd->hi0[a], nd->hi1[a]); }
    }
}

__device__ __forceinline__ float refit_padding(const uint32_t* __restrict__ hdr_ro)
{
    // padding = 2^-17 * max |coordinate| of the scene bounds (lbvh_padding in pt_lbvh.cpp)
    float smax = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) smax = fmaxf(smax, fmaxf(fabsf(ord2f(hdr_ro[6 + a])), fabsf(ord2f(hdr_ro[9 + a]))));
    return smax * 7.62939453125e-06f;
}

__device__ __forceinline__ void write_node_boxes(const float4* __restrict__ sorted, PtBvhNode* nodes, int i, int c0, int c1, float pad)
{
    float lo[3], hi[3];
    PtBvhNode* nd = &nodes[i];
    child_box(sorted, nodes, c0, pad, lo, hi);
#pragma unroll
    for (int a = 0; a < 3; a++) { nd->lo0[a] = lo[a]; nd->hi0[a] = hi[a]; }
    child_box(sorted, nodes, c1, pad, lo, hi);
#pragma unroll
    for (int a = 0; a < 3; a++) { nd->lo1[a] = lo[a]; nd->hi1[a] = hi[a]; }
}

constexpr int kRefitSmall = 1024;  // up to this many spheres one workgroup does every pass (barriers instead of launches)

}  // namespace

}  // namespace pt
