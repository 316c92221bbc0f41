// pt_restir_full.hip -- the launches of pt_restir_di_full (row N22, DESIGN.md spec S26): the reservoir pass of pt_restir.hip with the
// visibility word, final shading's reuse of it, and pairwise MIS.  One lane per pixel, one 8x8 pixel block per wave64, the walker
// chosen by with_tree_walk, as there; the kernels of rows N10 / N16 / N17 stay in pt_restir.hip as they were.
//   launch 1  ri_pass1_full_reservoir: a sample whose initial visibility ray reached its emitter says so in the reservoir's eighth word,
//             and the word travels with the sample through temporal resampling (kPairwise: under bias mode 2)
//   launch 2  ri_pass2_full_px: kPairwise -- the spatial pass under bias mode 2; kReuse -- a young, near sample that was seen casts no
//             final ray.  A wave's time is its slowest lane's: a skipped ray saves time only where a whole wave skips (no compaction).
#include "pt_trace.h"
#include "pt_restir.h"

namespace pt {

namespace {

// Launch 1.  The boiling filter is a run-time switch here (p.boiling_filter is the same in every lane), so the loop has the shape of
// restir_ex_kernel's kFilter form: every lane of a wave reaches the butterfly, a slot outside the image or a pixel without a surface
// with weight 0 (pm.n_slots is a multiple of 64 and the block size a multiple of the wave).
template <bool kLds, typename StackT, bool kAlpha, uint32_t kMode, bool kBrdf, bool kPairwise>
__global__ __launch_bounds__(kTraverseThreads) void restir_full1_kernel(SceneView sv, PixelMap pm, RiBuffers b, RiParamsFull p, LrView lr, RiExtra x)
{
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
    RiScene sc;
    sc.sph = sv.sph; sc.mats = sv.mats; sc.lights = sv.lights; sc.n_lights = sv.n_lights;
    sc.lr = lr;
    sc.light_of = x.light_of; sc.pyramid = x.pyramid; sc.pyramid_levels = x.pyramid_levels;
    sc.alpha_class = sv.alpha_class;
    const uint32_t stride = blockDim.x;
    const float mult = ri_boiling_multiplier(p.boiling_strength);
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { closest_hit_any<kLds, StackT, kAlpha>(sv, nodes, sph, ids, o, d, 0.0f, kInf, stack, stride, t, id); };
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        RiReservoir r;
        const bool has = pr.valid && ri_pass1_full_reservoir<kMode, kBrdf, kPairwise>(b, sc, p, pr.px, pr.py, trace, r);
        if (p.boiling_filter) {
            const float w = has ? r.W : 0.0f;
            float sum = w;
            uint32_t n = w > 0.0f ? 1u : 0u;
            for (int k = 0; k < 6; k++) {
                sum += __shfl_xor(sum, 1 << k);
                n += __shfl_xor(n, 1 << k);
            }
            if (has && ri_boiled(w, sum, n, mult)) r = ri_empty_reservoir();
        }
        if (has) ri_store_reservoir(b.res, pr.py * b.w + pr.px, r);
    }
}

// Launch 2.  kTex: the emission at the point reached goes through the emissive map; kAlpha: as launch 1
template <bool kLds, typename StackT, bool kTex, bool kAlpha, bool kPairwise, bool kReuse>
__global__ __launch_bounds__(kTraverseThreads) void restir_full2_kernel(SceneView sv, PixelMap pm, RiBuffers b, RiParamsFull p)
{
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
    RiScene sc;
    sc.sph = sv.sph; sc.mats = sv.mats; sc.lights = sv.lights; sc.n_lights = sv.n_lights;
    sc.lr = LrView{};
    sc.alpha_class = sv.alpha_class;
    const uint32_t stride = blockDim.x;
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { closest_hit_any<kLds, StackT, kAlpha>(sv, nodes, sph, ids, o, d, 0.0f, kInf, stack, stride, t, id); };
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        if (!pr.valid) continue;
        ri_pass2_full_px<kPairwise, kReuse>(b, sc, p, pr.px, pr.py, trace, [&](uint32_t id, f3 o, f3 d, float t) { return hit_material<kTex>(sv, id, o, d, t, false).emission; });
    }
}

template <bool kAlpha, uint32_t kMode, bool kBrdf, bool kPairwise>
hipError_t launch1_t(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, const LrView& lr, const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(restir_full1_kernel<kLds, StackT, kAlpha, kMode, kBrdf, kPairwise>, grid, traverse_threads(kLds),
                             traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream, sv, pm, b, p, lr, x);
    });
}

template <bool kAlpha, uint32_t kMode>
hipError_t launch1_mode(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, const LrView& lr, const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    const bool brdf = p.brdf_samples != 0, pairwise = p.temporal_bias == kRiBiasPairwise;
    if (brdf && pairwise) return launch1_t<kAlpha, kMode, true, true>(sv, pm, b, p, lr, x, grid, stream);
    if (brdf) return launch1_t<kAlpha, kMode, true, false>(sv, pm, b, p, lr, x, grid, stream);
    if (pairwise) return launch1_t<kAlpha, kMode, false, true>(sv, pm, b, p, lr, x, grid, stream);
    return launch1_t<kAlpha, kMode, false, false>(sv, pm, b, p, lr, x, grid, stream);
}

template <bool kAlpha>
hipError_t launch1_alpha(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, uint32_t mode, const LrView& lr, const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    if (mode == kLrPowerRis) return launch1_mode<kAlpha, kLrPowerRis>(sv, pm, b, p, lr, x, grid, stream);
    if (mode == kLrRegirRis) return launch1_mode<kAlpha, kLrRegirRis>(sv, pm, b, p, lr, x, grid, stream);
    return launch1_mode<kAlpha, kLrUniform>(sv, pm, b, p, LrView{}, x, grid, stream);
}

template <bool kTex, bool kAlpha, bool kPairwise, bool kReuse>
hipError_t launch2_t(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, uint32_t grid, hipStream_t stream)
{
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(restir_full2_kernel<kLds, StackT, kTex, kAlpha, kPairwise, kReuse>, grid, traverse_threads(kLds),
                             traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream, sv, pm, b, p);
    });
}

template <bool kTex, bool kAlpha>
hipError_t launch2_tex(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, uint32_t grid, hipStream_t stream)
{
    const bool pairwise = p.spatial_bias == kRiBiasPairwise, reuse = p.sh.reuse != 0;
    if (pairwise && reuse) return launch2_t<kTex, kAlpha, true, true>(sv, pm, b, p, grid, stream);
    if (pairwise) return launch2_t<kTex, kAlpha, true, false>(sv, pm, b, p, grid, stream);
    return launch2_t<kTex, kAlpha, false, true>(sv, pm, b, p, grid, stream);
}

}  // namespace

hipError_t launch_restir_full(int pass, const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, uint32_t mode, const LrView& lr,
                              const RiExtra& x, uint32_t grid, hipStream_t stream)
{
    // the alpha-tested walk and the textured emission: where launch_restir_pass takes them
    const bool alpha = sv.tex_maps && sv.alpha_tested;
    if (pass == 0) return alpha ? launch1_alpha<true>(sv, pm, b, p, mode, lr, x, grid, stream) : launch1_alpha<false>(sv, pm, b, p, mode, lr, x, grid, stream);
    if (p.spatial_bias != kRiBiasPairwise && !p.sh.reuse) return hipErrorInvalidValue;  // (launch_restir_pass's launch 2: the caller's to send)
    if (!sv.tex_maps) return launch2_tex<false, false>(sv, pm, b, p, grid, stream);
    return alpha ? launch2_tex<true, true>(sv, pm, b, p, grid, stream) : launch2_tex<true, false>(sv, pm, b, p, grid, stream);
}

}  // namespace pt
