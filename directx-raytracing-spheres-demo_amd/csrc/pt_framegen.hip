// pt_framegen.hip -- the frame-interpolation stand-in (row N13) for gfx950: two launches per generated frame on the caller's stream,
// both with 32 x 8 workgroups, one lane per pixel, each lane calling pt_framegen.h (DESIGN.md spec S19), so the result is bit for bit
// that of tests/hostshim.
// Scatter, one lane per render pixel: a 4-byte depth and a 12-byte vector load (consecutive per row of the workgroup), the depth's copy
// into the history, and up to four no-return 64-bit vector global atomics (atomicMin on unsigned long long = global_atomic_umin_x2)
// into the motion field, which the API clears to all-ones in front of the launch.  A min is independent of the order of its operands,
// so the field does not depend on how the waves are scheduled.  At rest every lane hits its own entry only: consecutive 8-byte
// addresses per row.  Every target is tested against the image in float before it is converted, so no address leaves the field.
// Gather, one lane per output pixel: three rounds of dependent loads (field entry; the winner's vector and depth; eight colour taps and
// one previous depth), each round issued whole before its first use; the taps' addresses are clamped into the image and fall back to
// the lane's own pixel where a side is invalid, so no load is predicated on data.  No LDS, no scratch.
#include "pt_kernels.h"
#include "pt_framegen.h"

namespace pt {

__global__ __launch_bounds__(kFgBlockW * kFgBlockH) void framegen_scatter_kernel(FgBuffers b, FgParams P)
{
    const int x = (int)(blockIdx.x * kFgBlockW + threadIdx.x), y = (int)(blockIdx.y * kFgBlockH + threadIdx.y);
    if (x >= (int)P.w || y >= (int)P.h) return;
    fg_scatter_pixel(P, b, x, y);
}

__global__ __launch_bounds__(kFgBlockW * kFgBlockH) void framegen_gather_kernel(FgBuffers b, FgParams P)
{
    const int ox = (int)(blockIdx.x * kFgBlockW + threadIdx.x), oy = (int)(blockIdx.y * kFgBlockH + threadIdx.y);
    if (ox >= (int)P.W || oy >= (int)P.H) return;
    b.out[(size_t)oy * P.W + ox] = fg_gather_pixel(P, b, ox, oy, nullptr);
}

hipError_t launch_framegen(const FgBuffers& b, const FgParams& P, hipStream_t stream)
{
    const dim3 block(kFgBlockW, kFgBlockH);
    const dim3 grid_in((P.w + kFgBlockW - 1) / kFgBlockW, (P.h + kFgBlockH - 1) / kFgBlockH);
    const dim3 grid_out((P.W + kFgBlockW - 1) / kFgBlockW, (P.H + kFgBlockH - 1) / kFgBlockH);
    hipLaunchKernelGGL(framegen_scatter_kernel, grid_in, block, 0, stream, b, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(framegen_gather_kernel, grid_out, block, 0, stream, b, P);
    return hipGetLastError();
}

}  // namespace pt
