// pt_nis.hip -- the sharpening stand-in (row N12) for gfx950: one launch per call on the caller's stream.  A 32 x 8 workgroup covers
// 32 x 8 texels, one lane each.  It first stages the lumas of its 36 x 12 footprint (two texels either side, coordinates clamped into
// the image) in LDS, 1,728 B, so that step 1's luma -- and its sqrt in Linear mode -- runs once per texel and not 25 times per lane;
// then every lane calls nis_pixel of pt_nis.h on that tile, so the result is bit for bit that of tests/hostshim (DESIGN.md spec S18).
// LDS access: a lane's 25 patch reads are ds_read_b32 (the compiler pairs some as ds_read2_b32, which bank the same way per dword).
// That instruction is served in the wave's two 32-lane halves with bank = dword address mod 32.  A half is one row of the workgroup
// (threadIdx.y fixed, threadIdx.x = 0..31) and for a given tap reads the dwords base + threadIdx.x of one tile row: 32 consecutive
// dwords, 32 distinct banks, whatever the row stride (36).  At the image's border the clamp makes neighbouring lanes read the same
// dword, which is a broadcast, not a conflict.  So the reads are free of bank conflicts; the staging's ds_write_b32 are consecutive
// dwords per half too.  A lane's own colour is one float4 global load (a line the staging just touched), the output one float4 store.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): HdrMode None 40 VGPRs, Linear 42, both 0 B scratch, 1,728 B LDS,
// 8 waves per SIMD.
#include "pt_kernels.h"
#include "pt_nis.h"

namespace pt {

template <uint32_t kHdr>
__global__ __launch_bounds__(kNisBlockW * kNisBlockH) void nis_kernel(const float4* __restrict__ color, float4* __restrict__ out, int w, int h, NisConfig k)
{
    __shared__ float s_y[kNisTileW * kNisTileH];
    const int x0 = (int)blockIdx.x * kNisBlockW - kNisBorder, y0 = (int)blockIdx.y * kNisBlockH - kNisBorder;
    const int tid = (int)(threadIdx.y * kNisBlockW + threadIdx.x);
    for (int i = tid; i < kNisTileW * kNisTileH; i += kNisBlockW * kNisBlockH) {
        const int ly = i / kNisTileW, lx = i - ly * kNisTileW;
        const int gx = nis_clamp_index(x0 + lx, w), gy = nis_clamp_index(y0 + ly, h);
        s_y[i] = nis_luma<kHdr>(color[(size_t)gy * w + gx]);
    }
    __syncthreads();
    const int x = x0 + kNisBorder + (int)threadIdx.x, y = y0 + kNisBorder + (int)threadIdx.y;
    if (x >= w || y >= h) return;
    NisTile T;
    T.y = s_y; T.x0 = x0; T.y0 = y0; T.stride = kNisTileW;
    const size_t o = (size_t)y * w + x;
    out[o] = nis_pixel<kHdr>(k, T, color[o], x, y, w, h);
}

hipError_t launch_nis(const float4* color, float4* out, uint32_t w, uint32_t h, const NisConfig& k, uint32_t hdr_mode, hipStream_t stream)
{
    const dim3 grid((w + kNisBlockW - 1) / kNisBlockW, (h + kNisBlockH - 1) / kNisBlockH), block(kNisBlockW, kNisBlockH);
    if (hdr_mode == kNisHdrLinear) hipLaunchKernelGGL(nis_kernel<kNisHdrLinear>, grid, block, 0, stream, color, out, (int)w, (int)h, k);
    else hipLaunchKernelGGL(nis_kernel<kNisHdrNone>, grid, block, 0, stream, color, out, (int)w, (int)h, k);
    return hipGetLastError();
}

}  // namespace pt
