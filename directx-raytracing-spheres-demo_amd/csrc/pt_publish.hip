// pt_publish.hip -- the kernels of pt_physics_publish (row N24, DESIGN.md spec S28).  All three move float4 records with one 16-byte load
// and one 16-byte store per lane; the small-scene take goes on to refit the lane's tree as refit_fused_small_kernel (pt_lbvh_gpu.hip) does.
#include "pt_publish.h"

#include <cmath>

#include "pt_lbvh_gpu.h"
#include "pt_refit_device.h"

namespace pt {

namespace {

// slot[0, n) = sph, slot[n, 2n) = rot
__global__ __launch_bounds__(256) void physics_publish_kernel(const float4* __restrict__ sph, const float4* __restrict__ rot, uint32_t n, float4* __restrict__ slot)
{
    const uint32_t total = 2u * n;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) slot[i] = i < n ? sph[i] : rot[i - n];
}

// the copies of a take for body i < t.n (every destination has room for the parts that are set: launch_lane_take*)
__device__ __forceinline__ void take_side_copies(const PublishTake& t, uint32_t i)
{
    if (t.rot) t.rot[i] = t.cur[t.n + i];
    if (t.prev_pose) {
        t.prev_pose[i] = t.prev[i];
        if (t.prev_rot) t.prev_pose[t.n + i] = t.prev[t.n + i];
    }
}

__global__ __launch_bounds__(256) void lane_take_kernel(const PublishTake t)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < t.n; i += gridDim.x * blockDim.x) {
        if (t.sph) t.sph[i] = t.cur[i];
        take_side_copies(t, i);
    }
}

// refit_fused_small_kernel with a published slot as its source and the take's other copies riding along: ONE launch at the head of the
// frame of a simulated small scene.  1 < n <= kRefitSmall; thread i owns body i, Morton slot i and node i (n - 1 nodes).
__global__ __launch_bounds__(kRefitSmall) void lane_take_small_kernel(const PublishTake t, const uint32_t* __restrict__ sorted_id, float4* __restrict__ sorted,
                                                                      PtBvhNode* nodes, uint32_t* hdr)
{
    __shared__ uint32_t s_level[kRefitSmall];
    __shared__ float4 s_sph[kRefitSmall];
    __shared__ float4 s_sorted[kRefitSmall];
    __shared__ uint32_t s_hdr[16];
    const int i = threadIdx.x;
    const int n = (int)t.n;
    if (i < 12) s_hdr[i] = ((i / 3) & 1) ? 0u : 0xFFFFFFFFu;
    float v[12];
#pragma unroll
    for (int a = 0; a < 3; a++) { v[a] = INFINITY; v[3 + a] = -INFINITY; v[6 + a] = INFINITY; v[9 + a] = -INFINITY; }
    if (i < n) {
        const float4 sp = t.cur[i];
        s_sph[i] = sp;
        t.sph[i] = sp;
        take_side_copies(t, (uint32_t)i);
        const float c[3] = { sp.x, sp.y, sp.z };
#pragma unroll
        for (int a = 0; a < 3; a++) { v[a] = c[a]; v[3 + a] = c[a]; v[6 + a] = c[a] - sp.w; v[9 + a] = c[a] + sp.w; }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const bool is_min = (k / 3) % 2 == 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_down(v[k], off, 64);
            v[k] = is_min ? fminf(v[k], o) : fmaxf(v[k], o);
        }
    }
    __syncthreads();  // s_hdr initialised, s_sph complete
    if ((i & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            if ((k / 3) % 2 == 0) atomicMin(&s_hdr[k], f2ord(v[k])); else atomicMax(&s_hdr[k], f2ord(v[k]));
        }
    }
    if (i < n) {
        const uint32_t id = sorted_id[i];
        const float4 g = s_sph[id < (uint32_t)n ? id : 0u];  // (a leaf order is a permutation of [0, n): the clamp only keeps a damaged one inside LDS)
        s_sorted[i] = g;
        sorted[i] = g;
    }
    const bool is_node = i < n - 1;
    int c0 = 0, c1 = 0;
    if (is_node) { c0 = nodes[i].child0; c1 = nodes[i].child1; }
    s_level[i] = 0xFFFFFFFFu;
    __syncthreads();  // bounds reduced, s_sorted complete
    if (i < 12) hdr[i] = s_hdr[i];
    const float pad = refit_padding(s_hdr);
    bool done = !is_node;
    for (uint32_t pass = 1; pass <= 64u; pass++) {
        if (!done) {
            const bool r0 = c0 < 0 || s_level[c0] < pass, r1 = c1 < 0 || s_level[c1] < pass;
            if (r0 && r1) {
                write_node_boxes(s_sorted, nodes, i, c0, c1, pad);
                s_level[i] = pass;
                done = true;
            }
        }
        __syncthreads();
        if (s_level[0] != 0xFFFFFFFFu) break;
    }
    if (i == 0) hdr[12] = s_level[0];
}

uint32_t copy_grid(uint32_t items) { return items / 256u + 1u < 2048u ? items / 256u + 1u : 2048u; }

// a part that is asked for has its source
bool take_ok(const PublishTake& t)
{
    if (t.n == 0 || ((t.sph || t.rot) && !t.cur) || (t.prev_pose && !t.prev)) return false;
    return t.sph || t.rot || t.prev_pose;
}

}  // namespace

hipError_t launch_physics_publish(const float4* sph, const float4* rot, uint32_t n, float4* slot, hipStream_t stream)
{
    if (!sph || !rot || !slot || n == 0 || n > (1u << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(physics_publish_kernel, dim3(copy_grid(2u * n)), dim3(256), 0, stream, sph, rot, n, slot);
    return hipGetLastError();
}

hipError_t launch_lane_take(const PublishTake& t, hipStream_t stream)
{
    if (!take_ok(t)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_take_kernel, dim3(copy_grid(t.n)), dim3(256), 0, stream, t);
    return hipGetLastError();
}

hipError_t launch_lane_take_small(const PublishTake& t, PtBvhNode* d_nodes, float4* d_sorted, const uint32_t* d_sorted_id, uint32_t* d_hdr, hipStream_t stream)
{
    if (!take_ok(t) || !t.sph || !lbvh_gpu_refit_fused_possible(t.n) || !d_nodes || !d_sorted || !d_sorted_id || !d_hdr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_take_small_kernel, dim3(1), dim3(kRefitSmall), 0, stream, t, d_sorted_id, d_sorted, d_nodes, d_hdr);
    return hipGetLastError();
}

}  // namespace pt
