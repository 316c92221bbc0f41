// pt_nrd.hip -- the NRD composition pass (row N8) for gfx950: one launch per call, one lane per pixel over the row-major
// width x height buffers.  Every kernel calls the pt_nrd.h function of its direction, so the result is bit for bit that of
// tests/hostshim (DESIGN.md spec S14).  The pass is pure streaming: a 1-D grid keeps every load and store of a wave on
// consecutive addresses (float4 buffers: global_load/store_dwordx4; the float3 albedos: dwordx3), a miss pixel reads its 4 bytes
// of depth and stops, and ReLAX pack does not read NormalRoughness.  No LDS, no scratch.
#include "pt_kernels.h"
#include "pt_nrd.h"

namespace pt {

constexpr uint32_t kNrdBlock = 256;

PT_HD f3 load_f3(const float* p, size_t i) { return make_f3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

template <uint32_t kMode>
__global__ __launch_bounds__(kNrdBlock) void nrd_pack_kernel(NrdBuffers b, uint32_t n, NrdHitDistParams P)
{
    const uint32_t i = blockIdx.x * kNrdBlock + threadIdx.x;
    if (i >= n) return;
    const float z = b.linear_depth[i];
    if (!is_finite(z)) return;
    const float roughness = kMode == kNrdReblur ? b.normal_roughness[i].w : 0.0f;
    float4 d = b.noisy_diffuse[i], s = b.noisy_specular[i];
    nrd_pack_px<kMode>(z, load_f3(b.diffuse_albedo, i), load_f3(b.specular_albedo, i), roughness, P, d, s);
    b.noisy_diffuse[i] = d;
    b.noisy_specular[i] = s;
}

template <uint32_t kMode>
__global__ __launch_bounds__(kNrdBlock) void nrd_compose_kernel(NrdBuffers b, uint32_t n)
{
    const uint32_t i = blockIdx.x * kNrdBlock + threadIdx.x;
    if (i >= n) return;
    if (!is_finite(b.linear_depth[i])) return;
    b.radiance[i] = nrd_compose_px<kMode>(b.radiance[i], load_f3(b.diffuse_albedo, i), load_f3(b.specular_albedo, i), b.denoised_diffuse[i],
                                          b.denoised_specular[i]);
}

hipError_t launch_nrd_composition(const NrdBuffers& b, uint32_t n_pixels, bool pack, uint32_t mode, NrdHitDistParams P, hipStream_t stream)
{
    const dim3 grid((n_pixels + kNrdBlock - 1) / kNrdBlock), block(kNrdBlock);
    if (pack) {
        if (mode == kNrdReblur) hipLaunchKernelGGL(nrd_pack_kernel<kNrdReblur>, grid, block, 0, stream, b, n_pixels, P);
        else hipLaunchKernelGGL(nrd_pack_kernel<kNrdRelax>, grid, block, 0, stream, b, n_pixels, P);
    } else {
        if (mode == kNrdReblur) hipLaunchKernelGGL(nrd_compose_kernel<kNrdReblur>, grid, block, 0, stream, b, n_pixels);
        else hipLaunchKernelGGL(nrd_compose_kernel<kNrdRelax>, grid, block, 0, stream, b, n_pixels);
    }
    return hipGetLastError();
}

}  // namespace pt
