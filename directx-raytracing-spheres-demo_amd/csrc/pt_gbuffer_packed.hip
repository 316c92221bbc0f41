// pt_gbuffer_packed.hip -- the G-buffer pass into the reference's texel formats (row N27, DESIGN.md spec S30; pt_render_gbuffer_packed):
// pt_gbuffer.hip's kernel -- one lane per pixel, one 8x8 pixel block per wave (PixelMap), the closest hit of the primary ray through the
// tree the context has (with_tree_walk), gbuffer_pixel -- with every store going through the packers of pt_pixfmt.h.  The 1- and 2-byte
// channels stay per-pixel stores: a texel the pass does not write keeps its value, so no store may be widened over a neighbour.
#include "pt_trace.h"
#include "pt_pixfmt.h"

namespace pt {

namespace {

template <bool kLds, typename StackT, bool kTex, bool kAlpha>
__global__ __launch_bounds__(kTraverseThreads) void gbuffer_packed_kernel(SceneView sv, PixelMap pm, GBufferFrame fr, GBufferScene sc, GBufferPackedOut out, uint32_t want)
{
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        if (!pr.valid) continue;
        f3 o, d;
        float tmin, tmax, t;
        uint32_t id;
        primary_ray(fr.cam, pr.px, pr.py, o, d, tmin, tmax);
        closest_hit_any<kLds, StackT, kAlpha>(sv, nodes, sph, ids, o, d, tmin, tmax, stack, blockDim.x, t, id);
        const GBufferPixel g = gbuffer_pixel<kTex>(fr, sc, pr.px, pr.py, t, id == kMissId ? kGbNoHit : id, want);
        const uint32_t i = pr.out_index;
        // `want` is uniform: each store sits behind a scalar branch, the per-pixel mask only sets the lanes
        if (want & kGbPosition) if (g.mask & kGbPosition) out.Position[i] = g.Position;
        if (want & kGbFlatNormal) if (g.mask & kGbFlatNormal) out.FlatNormal[i] = gbp_pack_normal(g.FlatNormal);
        if (want & kGbGeometricNormal) if (g.mask & kGbGeometricNormal) out.GeometricNormal[i] = gbp_pack_normal(g.GeometricNormal);
        if (want & kGbLinearDepth) if (g.mask & kGbLinearDepth) out.LinearDepth[i] = g.LinearDepth;
        if (want & kGbNormalizedDepth) if (g.mask & kGbNormalizedDepth) out.NormalizedDepth[i] = g.NormalizedDepth;
        if (want & kGbMotionVector) if (g.mask & kGbMotionVector) out.MotionVector[i] = gbp_pack_motion(g.MotionVector);
        if (want & kGbBaseColorMetalness) if (g.mask & kGbBaseColorMetalness) out.BaseColorMetalness[i] = gbp_pack_base_color_metalness(g.BaseColorMetalness);
        if (want & kGbDiffuseAlbedo) if (g.mask & kGbDiffuseAlbedo) out.DiffuseAlbedo[i] = gbp_pack_albedo(g.DiffuseAlbedo);
        if (want & kGbSpecularAlbedo) if (g.mask & kGbSpecularAlbedo) out.SpecularAlbedo[i] = gbp_pack_albedo(g.SpecularAlbedo);
        if (want & kGbNormalRoughness) if (g.mask & kGbNormalRoughness) out.NormalRoughness[i] = gbp_pack_normal_roughness(g.NormalRoughness);
        if (want & kGbIOR) if (g.mask & kGbIOR) out.IOR[i] = gbp_pack_ior(g.IOR);
        if (want & kGbTransmission) if (g.mask & kGbTransmission) out.Transmission[i] = gbp_pack_transmission(g.Transmission);
        if (want & kGbRadiance) if (g.mask & kGbRadiance) out.Radiance[i] = gbp_pack_radiance(g.Radiance);
    }
}

template <bool kTex, bool kAlpha>
hipError_t launch_t(const SceneView& sv, const PixelMap& pm, const GBufferFrame& fr, const GBufferScene& sc, const GBufferPackedOut& out, uint32_t want, uint32_t grid,
                    hipStream_t stream)
{
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(gbuffer_packed_kernel<kLds, StackT, kTex, kAlpha>, grid, traverse_threads(kLds), traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds),
                             stream, sv, pm, fr, sc, out, want);
    });
}

}  // namespace

hipError_t launch_gbuffer_packed(const SceneView& sv, const PixelMap& pm, const GBufferFrame& fr, const GBufferScene& sc, const GBufferPackedOut& out, uint32_t want,
                                 uint32_t grid, hipStream_t stream)
{
    // the textured variants only where textures exist; the alpha-tested walk only where some sphere's hits are tested against a map
    if (!sv.tex_maps) return launch_t<false, false>(sv, pm, fr, sc, out, want, grid, stream);
    if (sv.alpha_tested) return launch_t<true, true>(sv, pm, fr, sc, out, want, grid, stream);
    return launch_t<true, false>(sv, pm, fr, sc, out, want, grid, stream);
}

}  // namespace pt
