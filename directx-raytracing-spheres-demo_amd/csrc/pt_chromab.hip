// pt_chromab.hip -- chromatic aberration (row N29) for gfx950: one launch per call on the caller's stream.  A 32 x 8 workgroup covers
// 32 x 8 texels, one lane each.  The source taps of channel c are an affine image of the tile (scale 1 + k_c about the focus), so the
// workgroup first stages, per channel, the sanitised scalars of that image's 35 x 10 window (pt_chromab.h derives the size and the
// origin, which cab_origin makes with the lanes' own cab_pos) in LDS, three planes, 4,200 B: the 12 float4 gathers a lane would
// issue, of which it uses one dword each, become 12 ds_read_b32.  Then every lane calls cab_pixel of pt_chromab.h on the planes, so
// the result is bit for bit that of tests/hostshim/chromab_host.cpp (DESIGN.md spec S31).  Lanes outside the image take part in the
// staging and the barrier and return after it.
// Global access: a staged entry is one dword of a float4 texel (up to 1,050 per workgroup, at most 5 per lane); the three planes of a
// workgroup overlap in all but the fringe, so the lines of its window are fetched from memory once and twice more from cache.  A
// lane's own alpha is one dword load, the output one float4 store.
// LDS access: ds_read_b32 is served in the wave's two 32-lane halves with bank = dword address mod 32.  A half is one row of the
// workgroup (threadIdx.y fixed), whose taps of one kind (a, b, c or d) lie in one plane row at the dwords base + (i(x) - origin), i
// non-decreasing in x over a span of at most 35 dwords.  For k_c < 0 the step of i is 0 or 1 and the span at most 31: every dword a
// bank of its own, equal dwords a broadcast, no conflict.  For k_c > 0 the step is 1 or, at most three times per row, 2: the span is
// at most 35 dwords, so at most dwords 32, 33 and 34 share a bank with 0, 1 and 2 -- at most three 2-way conflicts, one extra cycle
// on a read of 32 lanes.  k_c = 0 is 32 consecutive dwords.  The staging's ds_write_b32 are consecutive dwords.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 26 VGPRs, 31 SGPRs, 0 B scratch, 4,200 B LDS, 8 waves per SIMD.
#include "pt_kernels.h"
#include "pt_chromab.h"

namespace pt {

__global__ __launch_bounds__(kCabBlockW * kCabBlockH) void chromab_kernel(const float4* __restrict__ color, float4* __restrict__ out, int w, int h, CabConfig k)
{
    __shared__ float s_v[3 * kCabPlane];
    const int X0 = (int)blockIdx.x * kCabBlockW, Y0 = (int)blockIdx.y * kCabBlockH;
    const int ox0 = cab_origin(X0, k.fx, k.k[0], w), ox1 = cab_origin(X0, k.fx, k.k[1], w), ox2 = cab_origin(X0, k.fx, k.k[2], w);
    const int oy0 = cab_origin(Y0, k.fy, k.k[0], h), oy1 = cab_origin(Y0, k.fy, k.k[1], h), oy2 = cab_origin(Y0, k.fy, k.k[2], h);
    const int tid = (int)(threadIdx.y * kCabBlockW + threadIdx.x);
    const float* __restrict__ scalars = reinterpret_cast<const float*>(color);
    for (int i = tid; i < 3 * kCabPlane; i += kCabBlockW * kCabBlockH) {
        const int ch = i / kCabPlane, r = i - ch * kCabPlane;
        const int ly = r / kCabWinW, lx = r - ly * kCabWinW;
        const int ox = ch == 0 ? ox0 : (ch == 1 ? ox1 : ox2), oy = ch == 0 ? oy0 : (ch == 1 ? oy1 : oy2);
        const int gx = cab_clamp_index(ox + lx, w), gy = cab_clamp_index(oy + ly, h);
        s_v[i] = up_sanitize(scalars[((size_t)gy * w + gx) * 4 + ch]);
    }
    __syncthreads();
    const int x = X0 + (int)threadIdx.x, y = Y0 + (int)threadIdx.y;
    if (x >= w || y >= h) return;
    CabWindow W;
    W.c[0].v = s_v;                 W.c[0].x0 = ox0; W.c[0].y0 = oy0; W.c[0].stride = kCabWinW;
    W.c[1].v = s_v + kCabPlane;     W.c[1].x0 = ox1; W.c[1].y0 = oy1; W.c[1].stride = kCabWinW;
    W.c[2].v = s_v + 2 * kCabPlane; W.c[2].x0 = ox2; W.c[2].y0 = oy2; W.c[2].stride = kCabWinW;
    const size_t o = (size_t)y * w + x;
    out[o] = cab_pixel(k, W, scalars[o * 4 + 3], x, y, w, h);
}

hipError_t launch_chromab(const float4* color, float4* out, uint32_t w, uint32_t h, const CabConfig& k, hipStream_t stream)
{
    const dim3 grid((w + kCabBlockW - 1) / kCabBlockW, (h + kCabBlockH - 1) / kCabBlockH), block(kCabBlockW, kCabBlockH);
    hipLaunchKernelGGL(chromab_kernel, grid, block, 0, stream, color, out, (int)w, (int)h, k);
    return hipGetLastError();
}

}  // namespace pt
