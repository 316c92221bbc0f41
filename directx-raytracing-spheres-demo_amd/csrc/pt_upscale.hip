// pt_upscale.hip -- the super-resolution stand-in (row N11) for gfx950: one launch per call on the caller's stream.  A 32 x 8 workgroup
// covers 32 x 8 output pixels, one lane each.  It first stages the input footprint of its pixels (at most kUpTileW x kUpTileH input
// pixels, because OutputSize >= InputSize) in LDS as sanitised t-space colour + depth (one float4) and three velocity planes, so that
// step 1's division runs once per input pixel and not nine times per output lane; then every lane calls up_pixel of pt_upscale.h on
// that tile, so the result is bit for bit that of tests/hostshim (DESIGN.md spec S17).  A lane's nine float4 taps are ds_read_b128.
// Each of that instruction's four 16-lane groups (lanes {0-3, 12-15, 20-27} and so on) lies in one output row, hence in one tile row,
// so the row stride plays no part: two lanes conflict when their texels differ by 16 (the same 16-B slot of the 256-B bank row).  At
// 1:1 a group's texels are those lane numbers, distinct modulo 16: conflict-free.  From 1.8x up (27 / 15) a group's texels span fewer
// than 16: conflict-free.  In between (1.5x, 1.7x) they span 16 to 28 and a few lanes meet 2-way, never more.  The velocity reads of the
// dilated tap are ds_read_b32 of nearly consecutive dwords.  The history is read with plain global loads (consecutive per wave at
// rest); output and history are whole float4 stores.  No scratch.
#include "pt_kernels.h"
#include "pt_upscale.h"

namespace pt {

constexpr uint32_t kUpBlockX = kUpBlockW, kUpBlockY = kUpBlockH;

template <bool kRestart>
__global__ __launch_bounds__(kUpBlockX * kUpBlockY) void upscale_kernel(UpBuffers b, UpParams P)
{
    __shared__ float4 s_tz[kUpTileW * kUpTileH];
    __shared__ float s_v[3][kUpTileW * kUpTileH];
    const int X0 = (int)(blockIdx.x * kUpBlockX), Y0 = (int)(blockIdx.y * kUpBlockY);
    const UpFootprint F = up_footprint(P, X0, Y0);
    const int fx0 = F.x0, fy0 = F.y0, fw = F.fw, fh = F.fh;
    for (int ly = (int)threadIdx.y; ly < fh; ly += (int)kUpBlockY)
        for (int lx = (int)threadIdx.x; lx < fw; lx += (int)kUpBlockX) {
            const size_t g = (size_t)(fy0 + ly) * P.w + (fx0 + lx);
            const int s = ly * kUpTileW + lx;
            s_tz[s] = up_stage_px(b.color[g], b.depth[g]);
            s_v[0][s] = b.velocity[3 * g];
            s_v[1][s] = b.velocity[3 * g + 1];
            s_v[2][s] = b.velocity[3 * g + 2];
        }
    __syncthreads();
    const int ox = X0 + (int)threadIdx.x, oy = Y0 + (int)threadIdx.y;
    if (ox >= (int)P.W || oy >= (int)P.H) return;
    UpTile T;
    T.tz = s_tz; T.vx = s_v[0]; T.vy = s_v[1]; T.vz = s_v[2];
    T.x0 = fx0; T.y0 = fy0; T.stride = kUpTileW;
    up_pixel<kRestart>(P, T, b, ox, oy);
}

hipError_t launch_upscale(const UpBuffers& b, const UpParams& P, bool restart, hipStream_t stream)
{
    const dim3 grid((P.W + kUpBlockX - 1) / kUpBlockX, (P.H + kUpBlockY - 1) / kUpBlockY), block(kUpBlockX, kUpBlockY);
    if (restart) hipLaunchKernelGGL(upscale_kernel<true>, grid, block, 0, stream, b, P);
    else hipLaunchKernelGGL(upscale_kernel<false>, grid, block, 0, stream, b, P);
    return hipGetLastError();
}

}  // namespace pt
