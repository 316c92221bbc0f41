// pt_reblur.hip -- the ReBLUR stand-in (row N30) for gfx950: pass (a) temporal, pass (b) history fix and fast clamp, pass (c) blur and
// pass (d) post-blur, four launches on the caller's stream.  One lane per pixel over 32 x 8 tiles (a wave covers 32 x 2 pixels); every
// lane calls the pt_reblur.h function of its pass, so the result is bit for bit that of tests/hostshim (DESIGN.md spec S32).  Both
// lobes go in every launch, so a pixel's guides are read once per pass.  The blur's taps are per-lane gathers up to 64 pixels away:
// plain global loads served by L2 and the Infinity Cache.  No LDS, no atomics, no scratch.
#include "pt_kernels.h"
#include "pt_reblur.h"

namespace pt {

constexpr uint32_t kRbTileX = 32, kRbTileY = 8;

__global__ __launch_bounds__(kRbTileX * kRbTileY) void rb_temporal_kernel(RbBuffers b, RbParams P)
{
    const uint32_t x = blockIdx.x * kRbTileX + threadIdx.x, y = blockIdx.y * kRbTileY + threadIdx.y;
    if (x >= b.w || y >= b.h) return;
    rb_temporal_px(b, P, (int)x, (int)y);
}

__global__ __launch_bounds__(kRbTileX * kRbTileY) void rb_fix_kernel(RbBuffers b, RbParams P)
{
    const uint32_t x = blockIdx.x * kRbTileX + threadIdx.x, y = blockIdx.y * kRbTileY + threadIdx.y;
    if (x >= b.w || y >= b.h) return;
    rb_fix_px(b, P, (int)x, (int)y);
}

template <bool kPost>
__global__ __launch_bounds__(kRbTileX * kRbTileY) void rb_blur_kernel(RbBuffers b, RbParams P)
{
    const uint32_t x = blockIdx.x * kRbTileX + threadIdx.x, y = blockIdx.y * kRbTileY + threadIdx.y;
    if (x >= b.w || y >= b.h) return;
    rb_blur_px<kPost>(b, P, (int)x, (int)y);
}

hipError_t launch_nrd_reblur(const RbBuffers& b, const RbParams& P, hipStream_t stream)
{
    const dim3 grid((b.w + kRbTileX - 1) / kRbTileX, (b.h + kRbTileY - 1) / kRbTileY), block(kRbTileX, kRbTileY);
    hipLaunchKernelGGL(rb_temporal_kernel, grid, block, 0, stream, b, P);
    hipLaunchKernelGGL(rb_fix_kernel, grid, block, 0, stream, b, P);
    hipLaunchKernelGGL(rb_blur_kernel<false>, grid, block, 0, stream, b, P);
    hipLaunchKernelGGL(rb_blur_kernel<true>, grid, block, 0, stream, b, P);
    return hipGetLastError();
}

}  // namespace pt
