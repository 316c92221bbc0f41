// pt_restir.hip -- the reservoir pass of row N10 (pt_restir_di, DESIGN.md spec S16) as two launches: one lane per pixel, one 8x8
// pixel block per wave64 (the PixelMap of the primary pass, so that the visibility rays of a wave stay coherent).
//   launch 1  ri_pass1_px: the pixel's surface record from the G-buffer, initial sampling, temporal resampling -- reads only the
//             previous call's slot, writes this call's record and reservoir
//   launch 2  ri_pass2_px: spatial resampling over every pixel's launch-1 result (hence the launch boundary), final shading
// Visibility rays go through the closest-hit walker the context's tree has (LDS copy, or the wide / binary walk in global memory).
#include "pt_trace.h"
#include "pt_restir.h"

namespace pt {

namespace {

// kPass2 = false: launch 1 (kTex unused: nothing is shaded with maps); kAlpha: the per-crossing alpha test of S10; kMode: the source of
// launch 1's candidates (spec S22; launch 2 has the Uniform form only and reads no `lr`)
template <bool kPass2, bool kLds, typename StackT, bool kTex, bool kAlpha, uint32_t kMode>
__global__ __launch_bounds__(kTraverseThreads) void restir_kernel(SceneView sv, PixelMap pm, RiBuffers b, RiParams p, LrView lr)
{
    extern __shared__ float4 smem[];
    const float4* nodes = sv.nodes;
    const float4* sph = sv.sph_sorted;
    const uint32_t* ids = sv.sorted_id;
    StackT* stack;
    if (kLds) {
        stage_scene(sv, smem);
        nodes = smem;
        sph = smem + sv.n_nodes * 4u;
        ids = reinterpret_cast<const uint32_t*>(smem + sv.n_nodes * 4u + sv.n);
        stack = reinterpret_cast<StackT*>(reinterpret_cast<char*>(smem) + scene_lds_bytes(sv.n_nodes, sv.n));
    } else {
        stack = reinterpret_cast<StackT*>(smem);
    }
    stack += threadIdx.x;
    RiScene sc;
    sc.sph = sv.sph; sc.mats = sv.mats; sc.lights = sv.lights; sc.n_lights = sv.n_lights;
    sc.lr = lr;
    const uint32_t stride = blockDim.x;
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { closest_hit_any<kLds, StackT, kAlpha>(sv, nodes, sph, ids, o, d, 0.0f, kInf, stack, stride, t, id); };
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        if (!pr.valid) continue;
        if (kPass2) ri_pass2_px(b, sc, p, pr.px, pr.py, trace, [&](uint32_t id, f3 o, f3 d, float t) { return hit_material<kTex>(sv, id, o, d, t, false).emission; });
        else ri_pass1_px<kMode>(b, sc, p, pr.px, pr.py, trace);
    }
}

// Launch 1 of pt_restir_di_ex (row N17, spec S23): kBrdf -- initial sampling mixes BRDF candidates in (ri_initial_mis); kFilter -- the
// boiling filter over the wave's 8x8 block before the reservoir is stored.  The filter is a wave-wide butterfly, so in its instances
// every lane of a wave reaches it: a slot outside the image or a pixel without a surface takes part with weight 0 (pm.n_slots is a
// multiple of 64 and the block size a multiple of the wave: a wave is inside the loop whole or not at all).
template <bool kLds, typename StackT, bool kAlpha, uint32_t kMode, bool kBrdf, bool kFilter>
__global__ __launch_bounds__(kTraverseThreads) void restir_ex_kernel(SceneView sv, PixelMap pm, RiBuffers b, RiParamsEx p, LrView lr, RiExtra x)
{
    extern __shared__ float4 smem[];
    const float4* nodes = sv.nodes;
    const float4* sph = sv.sph_sorted;
    const uint32_t* ids = sv.sorted_id;
    StackT* stack;
    if (kLds) {
        stage_scene(sv, smem);
        nodes = smem;
        sph = smem + sv.n_nodes * 4u;
        ids = reinterpret_cast<const uint32_t*>(smem + sv.n_nodes * 4u + sv.n);
        stack = reinterpret_cast<StackT*>(reinterpret_cast<char*>(smem) + scene_lds_bytes(sv.n_nodes, sv.n));
    } else {
        stack = reinterpret_cast<StackT*>(smem);
    }
    stack += threadIdx.x;
    RiScene sc;
    sc.sph = sv.sph; sc.mats = sv.mats; sc.lights = sv.lights; sc.n_lights = sv.n_lights;
    sc.lr = lr;
    sc.light_of = x.light_of; sc.pyramid = x.pyramid; sc.pyramid_levels = x.pyramid_levels;
    const uint32_t stride = blockDim.x;
    const float mult = ri_boiling_multiplier(p.boiling_strength);
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { closest_hit_any<kLds, StackT, kAlpha>(sv, nodes, sph, ids, o, d, 0.0f, kInf, stack, stride, t, id); };
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        RiReservoir r;
        if (!kFilter) {
            if (!pr.valid) continue;
            if (!ri_pass1_reservoir<kMode, kBrdf>(b, sc, p, pr.px, pr.py, trace, r)) continue;
        } else {
            const bool has = pr.valid && ri_pass1_reservoir<kMode, kBrdf>(b, sc, p, pr.px, pr.py, trace, r);
            const float w = has ? r.W : 0.0f;
            float sum = w;
            uint32_t n = w > 0.0f ? 1u : 0u;
            for (int k = 0; k < 6; k++) {
                sum += __shfl_xor(sum, 1 << k);
                n += __shfl_xor(n, 1 << k);
            }
            if (!has) continue;
            if (ri_boiled(w, sum, n, mult)) r = ri_empty_reservoir();
        }
        ri_store_reservoir(b.res, pr.py * b.w + pr.px, r);
    }
}

template <bool kAlpha, uint32_t kMode, bool kBrdf, bool kFilter>
hipError_t launch_ex_t(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsEx& p, const LrView& lr, const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    const bool lds_scene = sv.lds_scene != 0, small = sv.n_nodes < 32767u;
    const uint32_t threads = traverse_threads(lds_scene);
    const uint32_t lds = traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, lds_scene, threads);
    const void* fn = lds_scene ? (small ? (const void*)restir_ex_kernel<true, uint16_t, kAlpha, kMode, kBrdf, kFilter> : (const void*)restir_ex_kernel<true, uint32_t, kAlpha, kMode, kBrdf, kFilter>)
                               : (small ? (const void*)restir_ex_kernel<false, uint16_t, kAlpha, kMode, kBrdf, kFilter> : (const void*)restir_ex_kernel<false, uint32_t, kAlpha, kMode, kBrdf, kFilter>);
    if (lds > 48u * 1024u) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (lds_scene) {
        if (small) hipLaunchKernelGGL((restir_ex_kernel<true, uint16_t, kAlpha, kMode, kBrdf, kFilter>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr, x);
        else hipLaunchKernelGGL((restir_ex_kernel<true, uint32_t, kAlpha, kMode, kBrdf, kFilter>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr, x);
    } else {
        if (small) hipLaunchKernelGGL((restir_ex_kernel<false, uint16_t, kAlpha, kMode, kBrdf, kFilter>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr, x);
        else hipLaunchKernelGGL((restir_ex_kernel<false, uint32_t, kAlpha, kMode, kBrdf, kFilter>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr, x);
    }
    return hipGetLastError();
}

template <bool kAlpha, uint32_t kMode>
hipError_t launch_ex_mode(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsEx& p, const LrView& lr, const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    const bool brdf = p.brdf_samples != 0, filter = p.boiling_filter != 0;
    if (brdf && filter) return launch_ex_t<kAlpha, kMode, true, true>(sv, pm, b, p, lr, x, grid, stream);
    if (brdf) return launch_ex_t<kAlpha, kMode, true, false>(sv, pm, b, p, lr, x, grid, stream);
    return launch_ex_t<kAlpha, kMode, false, true>(sv, pm, b, p, lr, x, grid, stream);
}

template <bool kAlpha>
hipError_t launch_ex_alpha(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsEx& p, uint32_t mode, const LrView& lr, const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    if (mode == kLrPowerRis) return launch_ex_mode<kAlpha, kLrPowerRis>(sv, pm, b, p, lr, x, grid, stream);
    if (mode == kLrRegirRis) return launch_ex_mode<kAlpha, kLrRegirRis>(sv, pm, b, p, lr, x, grid, stream);
    return launch_ex_mode<kAlpha, kLrUniform>(sv, pm, b, p, LrView{}, x, grid, stream);
}

template <bool kPass2, bool kTex, bool kAlpha, uint32_t kMode = kLrUniform>
hipError_t launch_t(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParams& p, const LrView& lr, uint32_t grid, hipStream_t stream)
{
    const bool lds_scene = sv.lds_scene != 0, small = sv.n_nodes < 32767u;
    const uint32_t threads = traverse_threads(lds_scene);
    const uint32_t lds = traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, lds_scene, threads);
    const void* fn = lds_scene ? (small ? (const void*)restir_kernel<kPass2, true, uint16_t, kTex, kAlpha, kMode> : (const void*)restir_kernel<kPass2, true, uint32_t, kTex, kAlpha, kMode>)
                               : (small ? (const void*)restir_kernel<kPass2, false, uint16_t, kTex, kAlpha, kMode> : (const void*)restir_kernel<kPass2, false, uint32_t, kTex, kAlpha, kMode>);
    if (lds > 48u * 1024u) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (lds_scene) {
        if (small) hipLaunchKernelGGL((restir_kernel<kPass2, true, uint16_t, kTex, kAlpha, kMode>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr);
        else hipLaunchKernelGGL((restir_kernel<kPass2, true, uint32_t, kTex, kAlpha, kMode>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr);
    } else {
        if (small) hipLaunchKernelGGL((restir_kernel<kPass2, false, uint16_t, kTex, kAlpha, kMode>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr);
        else hipLaunchKernelGGL((restir_kernel<kPass2, false, uint32_t, kTex, kAlpha, kMode>), dim3(grid), dim3(threads), lds, stream, sv, pm, b, p, lr);
    }
    return hipGetLastError();
}

template <bool kAlpha>
hipError_t launch_pass1(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParams& p, uint32_t mode, const LrView& lr, uint32_t grid, hipStream_t stream)
{
    if (mode == kLrPowerRis) return launch_t<false, false, kAlpha, kLrPowerRis>(sv, pm, b, p, lr, grid, stream);
    if (mode == kLrRegirRis) return launch_t<false, false, kAlpha, kLrRegirRis>(sv, pm, b, p, lr, grid, stream);
    return launch_t<false, false, kAlpha>(sv, pm, b, p, LrView{}, grid, stream);
}

}  // namespace

hipError_t launch_restir_pass(int pass, const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParams& p, uint32_t mode, const LrView& lr,
                              uint32_t grid, hipStream_t stream)
{
    // the alpha-tested walk only where some sphere's hits are tested against a map; the textured emission only where textures exist
    const bool alpha = sv.tex_maps && sv.alpha_tested;
    if (pass == 0) return alpha ? launch_pass1<true>(sv, pm, b, p, mode, lr, grid, stream) : launch_pass1<false>(sv, pm, b, p, mode, lr, grid, stream);
    if (!sv.tex_maps) return launch_t<true, false, false>(sv, pm, b, p, LrView{}, grid, stream);
    return alpha ? launch_t<true, true, true>(sv, pm, b, p, LrView{}, grid, stream) : launch_t<true, true, false>(sv, pm, b, p, LrView{}, grid, stream);
}

hipError_t launch_restir_pass1_ex(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsEx& p, uint32_t mode, const LrView& lr,
                                  const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    if (!p.brdf_samples && !p.boiling_filter) return launch_restir_pass(0, sv, pm, b, p, mode, lr, grid, stream);
    const bool alpha = sv.tex_maps && sv.alpha_tested;
    return alpha ? launch_ex_alpha<true>(sv, pm, b, p, mode, lr, x, grid, stream) : launch_ex_alpha<false>(sv, pm, b, p, mode, lr, x, grid, stream);
}

}  // namespace pt
