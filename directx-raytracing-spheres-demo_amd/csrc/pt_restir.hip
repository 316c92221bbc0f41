// pt_restir.hip -- the reservoir pass of row N10 (pt_restir_di, DESIGN.md spec S16) as two launches: one lane per pixel, one 8x8
// pixel block per wave64 (the PixelMap of the primary pass, so that the visibility rays of a wave stay coherent).
//   launch 1  ri_pass1_px: the pixel's surface record from the G-buffer, initial sampling, temporal resampling -- reads only the
//             previous call's slot, writes this call's record and reservoir
//   launch 2  ri_pass2_px: spatial resampling over every pixel's launch-1 result (hence the launch boundary), final shading
// Visibility rays go through the closest-hit walker the context's tree has (LDS copy, or the wide / binary walk in global memory),
// chosen by with_tree_walk (pt_launch.h).
#include "pt_trace.h"
#include "pt_restir.h"

namespace pt {

namespace {

// kPass2 = false: launch 1 (kTex unused: nothing is shaded with maps); kAlpha: the per-crossing alpha test of S10; kMode: the source of
// launch 1's candidates (spec S22; launch 2 has the Uniform form only and reads no `lr`)
template <bool kPass2, bool kLds, typename StackT, bool kTex, bool kAlpha, uint32_t kMode>
__global__ __launch_bounds__(kTraverseThreads) void restir_kernel(SceneView sv, PixelMap pm, RiBuffers b, RiParams p, LrView lr)
{
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
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
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
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
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(restir_ex_kernel<kLds, StackT, kAlpha, kMode, kBrdf, kFilter>, grid, traverse_threads(kLds),
                             traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream, sv, pm, b, p, lr, x);
    });
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
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(restir_kernel<kPass2, kLds, StackT, kTex, kAlpha, kMode>, grid, traverse_threads(kLds),
                             traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream, sv, pm, b, p, lr);
    });
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
