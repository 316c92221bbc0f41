// pt_denoise.hip -- the NRD stand-in (row N9) for gfx950: pass (a) temporal, pass (b) variance, then one launch per a-trous step,
// all on the caller's stream.  One lane per pixel over 32 x 8 tiles (a wave covers 32 x 2 pixels, so each tap row of a wave is 512
// consecutive bytes of a float4 buffer); every lane calls the pt_denoise.h function of its pass, so the result is bit for bit that
// of tests/hostshim (DESIGN.md spec S15).  Both lobes go in every launch, so the guides are read once per pass.  Taps are plain
// global loads served by L2 and the Infinity Cache.  No LDS, no scratch.
#include "pt_kernels.h"
#include "pt_denoise.h"

namespace pt {

constexpr uint32_t kDnTileX = 32, kDnTileY = 8;

template <uint32_t kMode>
__global__ __launch_bounds__(kDnTileX * kDnTileY) void dn_temporal_kernel(DnBuffers b, DnParams P)
{
    const uint32_t x = blockIdx.x * kDnTileX + threadIdx.x, y = blockIdx.y * kDnTileY + threadIdx.y;
    if (x >= b.w || y >= b.h) return;
    dn_temporal_px<kMode>(b, P, (int)x, (int)y);
}

__global__ __launch_bounds__(kDnTileX * kDnTileY) void dn_variance_kernel(DnBuffers b)
{
    const uint32_t x = blockIdx.x * kDnTileX + threadIdx.x, y = blockIdx.y * kDnTileY + threadIdx.y;
    if (x >= b.w || y >= b.h) return;
    dn_variance_px(b, (int)x, (int)y);
}

template <uint32_t kMode, bool kLast>
__global__ __launch_bounds__(kDnTileX * kDnTileY) void dn_atrous_kernel(DnBuffers b, int src, int step)
{
    const uint32_t x = blockIdx.x * kDnTileX + threadIdx.x, y = blockIdx.y * kDnTileY + threadIdx.y;
    if (x >= b.w || y >= b.h) return;
    dn_atrous_px<kMode, kLast>(b, src, step, (int)x, (int)y);
}

template <uint32_t kMode>
static hipError_t launch_mode(const DnBuffers& b, const DnParams& P, uint32_t iterations, hipStream_t stream)
{
    const dim3 grid((b.w + kDnTileX - 1) / kDnTileX, (b.h + kDnTileY - 1) / kDnTileY), block(kDnTileX, kDnTileY);
    hipLaunchKernelGGL(dn_temporal_kernel<kMode>, grid, block, 0, stream, b, P);
    hipLaunchKernelGGL(dn_variance_kernel, grid, block, 0, stream, b);
    for (uint32_t it = 0; it < iterations; it++) {
        const int src = (int)(it & 1u), step = 1 << it;
        if (it + 1 == iterations) hipLaunchKernelGGL((dn_atrous_kernel<kMode, true>), grid, block, 0, stream, b, src, step);
        else hipLaunchKernelGGL((dn_atrous_kernel<kMode, false>), grid, block, 0, stream, b, src, step);
    }
    return hipGetLastError();
}

hipError_t launch_nrd_denoise(const DnBuffers& b, uint32_t mode, const DnParams& P, uint32_t iterations, hipStream_t stream)
{
    return mode == kNrdReblur ? launch_mode<kNrdReblur>(b, P, iterations, stream) : launch_mode<kNrdRelax>(b, P, iterations, stream);
}

}  // namespace pt
