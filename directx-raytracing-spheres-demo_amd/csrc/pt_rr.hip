// pt_rr.hip -- the ray-reconstruction stand-in (row N15) for gfx950: two launches per call on the caller's stream (DESIGN.md spec S21).
//
// rr_prepare_kernel: one lane per render pixel, pure streaming: rr_prepare_px of pt_rr.h reads the seven inputs of its pixel and writes
// three float4 records (demodulated t-space colour + depth, normal + roughness, virtual motion + weight) into the context's work
// buffers, so the divisions of the demodulation and the matrix work of the virtual motion run once per render pixel.
//
// rr_resolve_kernel: a 32 x 8 workgroup covers 32 x 8 output pixels, one lane each.  It stages the footprint of its pixels (at most
// kRrTileW x kRrTileH = 36 x 12 input pixels) in LDS: two float4 records and the three motion planes, 432 * (32 + 12) B = 19008 B, so
// eight workgroups fit a CU's 160 KB.  Then every lane calls rr_pixel on that tile, so the result is bit for bit that of
// tests/hostshim/rr_host.cpp.  A lane whose nearest input pixel is a miss branches to up_pixel (9 taps) before the 25-tap loop, so a
// wave of sky lanes never executes that loop.
// The 25 taps are pairs of ds_read_b128 (colour + depth, normal + roughness) at one tile index.  As in pt_upscale.hip each of the
// instruction's four 16-lane groups lies in one output row, hence in one tile row, and two lanes conflict when their texels differ by
// 16: none at 1:1 (16 consecutive texels) and none from 1.8x up (a group spans fewer than 16 texels); in between (1.5x, 1.7x) a few
// lanes meet 2-way, never more.  The two arrays are separate allocations, so the pair of reads of one tap never conflicts with itself.
// The history's corners are plain global loads (consecutive per wave at rest); output and history are whole float4 stores.  No scratch.
#include "pt_kernels.h"
#include "pt_rr.h"

namespace pt {

constexpr uint32_t kRrPrepareBlock = 256;

__global__ __launch_bounds__(kRrPrepareBlock) void rr_prepare_kernel(RrBuffers b, RrParams R)
{
    const uint32_t i = blockIdx.x * kRrPrepareBlock + threadIdx.x;
    if (i >= R.up.w * R.up.h) return;  // (at most 2^28 render pixels)
    const RrRecord rec = rr_prepare_px(R, b, (int)(i % R.up.w), (int)(i / R.up.w));
    b.rec_tz[i] = rec.tz;
    b.rec_nr[i] = rec.nr;
    b.rec_virt[i] = rec.virt;
}

template <bool kRestart>
__global__ __launch_bounds__(kUpBlockW * kUpBlockH) void rr_resolve_kernel(RrBuffers b, RrParams R)
{
    __shared__ float4 s_tz[kRrTileW * kRrTileH];
    __shared__ float4 s_nr[kRrTileW * kRrTileH];
    __shared__ float s_v[3][kRrTileW * kRrTileH];
    const UpParams& P = R.up;
    const int X0 = (int)blockIdx.x * kUpBlockW, Y0 = (int)blockIdx.y * kUpBlockH;
    const UpFootprint F = rr_footprint(P, X0, Y0);
    for (int ly = (int)threadIdx.y; ly < F.fh; ly += kUpBlockH)
        for (int lx = (int)threadIdx.x; lx < F.fw; lx += kUpBlockW) {
            const size_t g = (size_t)(F.y0 + ly) * P.w + (F.x0 + lx);
            const int s = ly * kRrTileW + lx;
            s_tz[s] = b.rec_tz[g];
            s_nr[s] = b.rec_nr[g];
            s_v[0][s] = b.motion[3 * g];
            s_v[1][s] = b.motion[3 * g + 1];
            s_v[2][s] = b.motion[3 * g + 2];
        }
    __syncthreads();
    const int ox = X0 + (int)threadIdx.x, oy = Y0 + (int)threadIdx.y;
    if (ox >= (int)P.W || oy >= (int)P.H) return;
    RrTile T;
    T.tz = s_tz; T.nr = s_nr; T.vx = s_v[0]; T.vy = s_v[1]; T.vz = s_v[2];
    T.x0 = F.x0; T.y0 = F.y0; T.stride = kRrTileW;
    rr_pixel<kRestart>(R, T, b, ox, oy);
}

hipError_t launch_ray_reconstruction(const RrBuffers& b, const RrParams& R, bool restart, hipStream_t stream)
{
    const uint32_t n_in = R.up.w * R.up.h;
    hipLaunchKernelGGL(rr_prepare_kernel, dim3((n_in + kRrPrepareBlock - 1) / kRrPrepareBlock), dim3(kRrPrepareBlock), 0, stream, b, R);
    const dim3 grid((R.up.W + kUpBlockW - 1) / kUpBlockW, (R.up.H + kUpBlockH - 1) / kUpBlockH), block(kUpBlockW, kUpBlockH);
    if (restart) hipLaunchKernelGGL(rr_resolve_kernel<true>, grid, block, 0, stream, b, R);
    else hipLaunchKernelGGL(rr_resolve_kernel<false>, grid, block, 0, stream, b, R);
    return hipGetLastError();
}

}  // namespace pt
