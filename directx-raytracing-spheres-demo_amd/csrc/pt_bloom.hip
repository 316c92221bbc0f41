// pt_bloom.hip -- bloom (row N5) for gfx950: the 9 chain dispatches of PostProcessing::Bloom and the merge, one kernel
// launch each, on one stream.  One lane per output texel; every kernel calls the pt_bloom.h function of its step, so the
// result is bit for bit that of tests/hostshim (DESIGN.md spec S11).  Speed comes from the memory side only:
//   * 32x8 workgroups (a wave64 is a 32x2 patch): the 13 / 9 taps of neighbouring lanes overlap, and a 2-D patch keeps the
//     rows they share in the same L1 / L2 lines; texel loads and stores are float4 (global_load/store_dwordx4)
//   * the chain is one allocation (BloomChain), so the small levels of one call sit together in L2
// What was tried for the step-1 taps and the small tail launches: tools/experiments/README.md ("Bloom").
#include "pt_kernels.h"
#include "pt_bloom.h"

namespace pt {

constexpr uint32_t kBloomTx = 32, kBloomTy = 8;

template <bool kKaris>
__global__ __launch_bounds__(kBloomTx * kBloomTy) void bloom_down_kernel(TexView in, float4* __restrict__ out, u2 dims)
{
    const uint32_t x = blockIdx.x * kBloomTx + threadIdx.x, y = blockIdx.y * kBloomTy + threadIdx.y;
    if (x >= dims.x || y >= dims.y) return;
    const f3 r = bloom_downsample_px(in, dims, u2{x, y}, kKaris);
    out[(size_t)y * dims.x + x] = make_float4(r.x, r.y, r.z, 0.0f);
}

__global__ __launch_bounds__(kBloomTx * kBloomTy) void bloom_up_kernel(TexView in, float4* __restrict__ out, u2 dims)
{
    const uint32_t x = blockIdx.x * kBloomTx + threadIdx.x, y = blockIdx.y * kBloomTy + threadIdx.y;
    if (x >= dims.x || y >= dims.y) return;
    const f3 r = bloom_upsample_px(in, dims, u2{x, y});
    out[(size_t)y * dims.x + x] = make_float4(r.x, r.y, r.z, 0.0f);
}

// in and out may be the same buffer: each lane reads its own input texel before it writes it, and nothing else reads it
__global__ __launch_bounds__(kBloomTx * kBloomTy) void bloom_merge_kernel(const float4* in, TexView blur0, float4* out, u2 dims, float w1, float w2)
{
    const uint32_t x = blockIdx.x * kBloomTx + threadIdx.x, y = blockIdx.y * kBloomTy + threadIdx.y;
    if (x >= dims.x || y >= dims.y) return;
    const size_t i = (size_t)y * dims.x + x;
    out[i] = bloom_merge_px(in[i], blur0, dims, u2{x, y}, w1, w2);
}

static dim3 bloom_grid(uint32_t w, uint32_t h) { return dim3((w + kBloomTx - 1) / kBloomTx, (h + kBloomTy - 1) / kBloomTy); }

hipError_t launch_bloom(const float4* in, float4* out, float4* chain, uint32_t width, uint32_t height, float strength, hipStream_t stream)
{
    const BloomChain c = bloom_chain(width, height);
    const dim3 block(kBloomTx, kBloomTy);
    auto level = [&](uint32_t k) { return TexView{chain + c.off[k], c.w[k], c.h[k]}; };
    auto out_of = [&](uint32_t k) { return chain + c.off[k]; };
    auto dims = [&](uint32_t k) { return u2{c.w[k], c.h[k]}; };

    // steps 1-5: downsample; InputMipLevel is 0 in steps 1 and 2, so those two take the Karis average
    hipLaunchKernelGGL(bloom_down_kernel<true>, bloom_grid(c.w[0], c.h[0]), block, 0, stream, TexView{in, width, height}, out_of(0), dims(0));
    hipLaunchKernelGGL(bloom_down_kernel<true>, bloom_grid(c.w[1], c.h[1]), block, 0, stream, level(0), out_of(1), dims(1));
    for (uint32_t k = 2; k < kBloomMips; k++)
        hipLaunchKernelGGL(bloom_down_kernel<false>, bloom_grid(c.w[k], c.h[k]), block, 0, stream, level(k - 1), out_of(k), dims(k));
    // steps 6-9: upsample, each overwriting the level below the one it reads
    for (uint32_t k = kBloomMips - 1; k-- > 0;)
        hipLaunchKernelGGL(bloom_up_kernel, bloom_grid(c.w[k], c.h[k]), block, 0, stream, level(k + 1), out_of(k), dims(k));
    hipLaunchKernelGGL(bloom_merge_kernel, bloom_grid(width, height), block, 0, stream, in, level(0), out, u2{width, height}, 1.0f - strength, strength);
    return hipGetLastError();
}

}  // namespace pt
