// pt_gbframe.hip -- the kernel of row N27's frame (pt_render_from_gbuffer; DESIGN.md spec S30) over pt_gbframe.h: one lane per pixel, one
// 8x8 pixel block per wave64 (PixelMap), grid-stride: gbframe_pixel.  Rays go through the closest-hit walker the context's tree has (LDS
// copy, or the wide / binary walk in global memory), chosen by with_tree_walk (pt_launch.h); the instances are those of pt_lens.hip.
#include "pt_trace.h"
#include "pt_gbframe.h"

namespace pt {

namespace {

template <bool kLds, typename StackT, bool kTex, bool kAlpha>
__global__ __launch_bounds__(kTraverseThreads) void gbframe_kernel(SceneView sv, PixelMap pm, GbFrame fr, GbInput in, float4* __restrict__ out, unsigned long long* __restrict__ counter)
{
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
    const uint32_t stride = blockDim.x;
    auto trace = [&](f3 o, f3 d, float tmin, float tmax, float& t, uint32_t& id) {
        closest_hit_any<kLds, StackT, kAlpha>(sv, nodes, sph, ids, o, d, tmin, tmax, stack, stride, t, id);
    };
    auto material = [&](uint32_t id, f3 o, f3 d, float t, bool primary) { return hit_material<kTex>(sv, id, o, d, t, primary); };
    auto env = [&](f3 d) {
        if (kTex && sv.env_tex != kNoTexture)
            return sv.env_cube ? environment_cube(sv.tex + sv.env_tex, sv.env_xf, d) : environment_texture(sv.tex[sv.env_tex], sv.env_xf, d);
        return environment_color(sv.env[0], sv.env[1], sv.env[2], sv.env[3], d);
    };
    uint32_t rays = 0;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        if (!pr.valid) continue;
        const f3 c = gbframe_pixel(fr, in, pr.px, pr.py, pr.out_index, trace, material, env, rays);
        out[pr.out_index] = make_float4(c.x, c.y, c.z, 1.0f);
    }
    block_atomic_add(counter, rays);
}

template <bool kTex, bool kAlpha>
hipError_t launch_t(const SceneView& sv, const PixelMap& pm, const GbFrame& fr, const GbInput& in, float4* out, unsigned long long* counter, uint32_t grid, hipStream_t stream)
{
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(gbframe_kernel<kLds, StackT, kTex, kAlpha>, grid, traverse_threads(kLds), traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream,
                             sv, pm, fr, in, out, counter);
    });
}

}  // namespace

hipError_t launch_gbframe(const SceneView& sv, const PixelMap& pm, const GbFrame& fr, const GbInput& in, float4* out, unsigned long long* counter, uint32_t grid,
                          hipStream_t stream)
{
    // the textured variants only where textures exist; the alpha-tested walk only where some sphere's hits are tested against a map
    if (!sv.tex_maps) return launch_t<false, false>(sv, pm, fr, in, out, counter, grid, stream);
    if (sv.alpha_tested) return launch_t<true, true>(sv, pm, fr, in, out, counter, grid, stream);
    return launch_t<true, false>(sv, pm, fr, in, out, counter, grid, stream);
}

}  // namespace pt
