// pt_lightris.hip -- the kernels of row N16 (DESIGN.md spec S22) that fill what pt_lightris.h describes, wave64, 256 lanes a workgroup:
//   lr_pyramid_kernel  one workgroup reduces 1024 entries of a level through five levels (the wave-op scheme of MipmapGeneration.hlsl
//                      widened to wave64): a lane's four entries are one float4, __shfl_down by 1,2,3 / 4,8,12 / 16,32,48 lanes gives
//                      the next three levels, four LDS floats the fifth.  The first launch computes the leaves (the emitters' powers);
//                      a scene with more than 1024 emitters launches it again with level 5 (then 10, ...) as its leaves
//   lr_power_kernel    one lane per Power_RIS entry; every level is read with float4 global loads (the first nodes, which every lane
//                      reads, stay in L2; staging the levels of at most 256 entries in LDS was measured and lost: DESIGN.md section 10)
//   lr_regir_kernel    one lane per ReGIR slot; the workgroup's Power_RIS tile (one per 256 consecutive slots) is staged in LDS
// Every kernel calls the header's function for its element.  Cross-lane operations: __shfl_down and LDS with __syncthreads only.
#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_lightris.h"

namespace pt {

namespace {

constexpr uint32_t kLrThreads = 256;

// kFromPyramid = false: the entries are the leaves, computed here and stored; true: they are level `base` of the pyramid
template <bool kFromPyramid>
__global__ __launch_bounds__(kLrThreads) void lr_pyramid_kernel(LrBuild b, uint32_t lv, uint32_t base)
{
    __shared__ float wave_top[kLrThreads / 64u];
    const uint32_t lane = threadIdx.x, e1 = blockIdx.x * kLrThreads + lane;  // this lane's entry of level base + 1
    const uint32_t n_in = lr_level_size(lv, base);
    float* const level0 = b.pyramid + lr_level_offset(lv, base);
    float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (kFromPyramid) {
        if (4u * e1 + 3u < n_in) {  // (level sizes are powers of four: a quad is whole or absent, except the single entry of a top level)
            const float4 v = *reinterpret_cast<const float4*>(level0 + 4u * e1);
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        }
    } else {
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t j = 4u * e1 + k;
            if (j < b.n_lights) q[k] = lr_light_power(b.sph, b.mats, b.lights, j);
        }
        if (4u * e1 + 3u < n_in) {
            float4 v;
            v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
            *reinterpret_cast<float4*>(level0 + 4u * e1) = v;  // padding leaves are zeros: no clear is needed
        } else if (4u * e1 < n_in) {
            level0[4u * e1] = q[0];  // a pyramid of one emitter: the leaf is the top
        }
    }
    // level base + 1: the lane's own quad; the owner of a node of the next three levels is the first lane of its 4, 16, 64
    float v = lr_parent(q[0], q[1], q[2], q[3]);
    uint32_t idx = e1, level = base + 1u;
    if (level <= lv && idx < lr_level_size(lv, level)) b.pyramid[lr_level_offset(lv, level) + idx] = v;
#pragma unroll
    for (uint32_t step = 1u; step <= 16u; step *= 4u) {
        const float a1 = __shfl_down(v, step), a2 = __shfl_down(v, 2u * step), a3 = __shfl_down(v, 3u * step);
        v = lr_parent(v, a1, a2, a3);  // (meaningful in the owner lanes only)
        idx >>= 2;
        level++;
        if ((lane & (4u * step - 1u)) == 0u && level <= lv && idx < lr_level_size(lv, level)) b.pyramid[lr_level_offset(lv, level) + idx] = v;
    }
    if ((lane & 63u) == 0u) wave_top[lane >> 6] = v;
    __syncthreads();
    level++;
    if (lane == 0u && level <= lv && blockIdx.x < lr_level_size(lv, level))
        b.pyramid[lr_level_offset(lv, level) + blockIdx.x] = lr_parent(wave_top[0], wave_top[1], wave_top[2], wave_top[3]);
}

__global__ __launch_bounds__(kLrThreads) void lr_power_kernel(LrBuild b, uint32_t lv, uint32_t n_entries)
{
    const uint32_t i = blockIdx.x * kLrThreads + threadIdx.x;
    if (i >= n_entries) return;
    const uint32_t t = i / b.grid.tile_size, s = i - t * b.grid.tile_size;
    const float* const pyramid = b.pyramid;
    b.ris[i] = lr_power_entry(lv, t, s, b.frame_index, [&](uint32_t level, uint32_t node) {
        return *reinterpret_cast<const float4*>(pyramid + lr_level_offset(lv, level) + 4u * node);  // (level offsets are multiples of four)
    });
}

__global__ __launch_bounds__(kLrThreads) void lr_regir_kernel(LrBuild b, uint32_t n_slots)
{
    extern __shared__ LrEntry lr_tile[];
    // one tile per workgroup: its 256 slots share g >> 8 (blockIdx.x), so the tile is found from the workgroup's first slot
    const uint32_t tile = lr_regir_tile(blockIdx.x * kLrThreads, b.frame_index, b.grid.tile_count);
    const LrEntry* const src = b.ris + (size_t)tile * b.grid.tile_size;
    for (uint32_t i = threadIdx.x; i < b.grid.tile_size; i += kLrThreads) lr_tile[i] = src[i];
    __syncthreads();
    const uint32_t g = blockIdx.x * kLrThreads + threadIdx.x;
    if (g >= n_slots) return;
    b.ris[(size_t)b.grid.tile_size * b.grid.tile_count + g] =
        lr_regir_entry(b.grid, b.sph, b.mats, b.lights, g, b.frame_index, [&](uint32_t i) { return lr_tile[i]; });
}

}  // namespace

hipError_t launch_lr_pyramid(const LrBuild& b, hipStream_t stream)
{
    const uint32_t lv = lr_levels(b.n_lights);
    for (uint32_t base = 0; base == 0u || base < lv; base += kLrGroupLevels) {
        const uint32_t groups = (lr_level_size(lv, base) + kLrGroupLeaves - 1u) / kLrGroupLeaves;
        if (base == 0u) hipLaunchKernelGGL(lr_pyramid_kernel<false>, dim3(groups), dim3(kLrThreads), 0, stream, b, lv, base);
        else hipLaunchKernelGGL(lr_pyramid_kernel<true>, dim3(groups), dim3(kLrThreads), 0, stream, b, lv, base);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_lr_power(const LrBuild& b, hipStream_t stream)
{
    const uint32_t lv = lr_levels(b.n_lights), n = b.grid.tile_size * b.grid.tile_count;
    const uint32_t groups = (n + kLrThreads - 1u) / kLrThreads;
    hipLaunchKernelGGL(lr_power_kernel, dim3(groups), dim3(kLrThreads), 0, stream, b, lv, n);
    return hipGetLastError();
}

hipError_t launch_lr_regir(const LrBuild& b, hipStream_t stream)
{
    const uint32_t n = b.grid.grid * b.grid.grid * b.grid.grid * b.grid.lights_per_cell;
    const uint32_t lds = b.grid.tile_size * (uint32_t)sizeof(LrEntry);  // at most 64 KB
    return launch_kernel(lr_regir_kernel, (n + kLrThreads - 1u) / kLrThreads, kLrThreads, lds, stream, b, n);
}

}  // namespace pt
