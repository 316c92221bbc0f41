// pt_sharc.hip -- the three kernels of rows N14, N18 and N19 (pt_render_sharc, pt_render_sharc_ex; DESIGN.md specs S20, S24 and S25) over pt_sharc.h:
//   update   one lane per path of the downscaled grid, one 8x8 block of paths per wave64 (PixelMap): sh_update_path
//   resolve  one lane per slot of the hash map, streaming: sh_resolve_slot, 128-bit loads and stores
//   query    one lane per pixel, one 8x8 pixel block per wave64: sh_query_pixel
// kEx: the instances of pt_render_sharc_ex with a DI or denoiser outputs (sh_update_path_ex, sh_query_pixel_ex, which stores the pixel itself)
// kFf: the anti-firefly filter of row N19 (spec S25): the kEx update (sh_update_path_ff) and the resolve (sh_resolve_slot_ff); the query does not read the flag
// Rays go through the closest-hit walker the context's tree has (LDS copy, or the wide / binary walk in global memory), chosen by
// with_tree_walk (pt_launch.h).
#include "pt_trace.h"
#include "pt_sharc.h"

namespace pt {

namespace {

template <bool kQuery, bool kLds, typename StackT, bool kTex, bool kAlpha, bool kEx, bool kFf>
__global__ __launch_bounds__(kTraverseThreads) void sharc_kernel(SceneView sv, PixelMap pm, ShFrame fr, ShGrid g, ShMap m, float4* __restrict__ out,
                                                                 unsigned long long* __restrict__ counters)
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
    uint32_t rays = 0, failed = 0;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pm.n_slots; slot += gridDim.x * blockDim.x) {
        const PixelRef pr = slot_to_pixel(pm, slot);
        if (!pr.valid) continue;
        if (kQuery && kEx) {
            sh_query_pixel_ex(fr, g, m, pr.px, pr.py, pr.out_index, trace, material, env, rays, out);
        } else if (kQuery) {
            const f3 c = sh_query_pixel(fr, g, m, pr.px, pr.py, trace, material, env, rays);
            out[pr.out_index] = make_float4(c.x, c.y, c.z, 1.0f);
        } else if (kEx && kFf) {
            (void)sh_update_path_ff(fr, g, m, pr.px, pr.py, trace, material, env, rays, failed);
        } else if (kEx) {
            sh_update_path_ex(fr, g, m, pr.px, pr.py, trace, material, env, rays, failed);
        } else {
            sh_update_path(fr, g, m, pr.px, pr.py, trace, material, env, rays, failed);
        }
    }
    block_atomic_add(counters, rays);
    if (!kQuery) block_atomic_add(counters + 1, failed);
}

template <bool kQuery, bool kEx, bool kFf, bool kTex, bool kAlpha>
hipError_t launch_t(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, float4* out, unsigned long long* counters,
                    uint32_t grid, hipStream_t stream)
{
    return with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return launch_kernel(sharc_kernel<kQuery, kLds, StackT, kTex, kAlpha, kEx, kFf>, grid, traverse_threads(kLds),
                             traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream, sv, pm, fr, g, m, out, counters);
    });
}

template <bool kQuery, bool kEx, bool kFf>
hipError_t launch_any(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, float4* out, unsigned long long* counters,
                      uint32_t grid, hipStream_t stream)
{
    // the textured variants only where textures exist; the alpha-tested walk only where some sphere's hits are tested against a map
    if (!sv.tex_maps) return launch_t<kQuery, kEx, kFf, false, false>(sv, pm, fr, g, m, out, counters, grid, stream);
    if (sv.alpha_tested) return launch_t<kQuery, kEx, kFf, true, true>(sv, pm, fr, g, m, out, counters, grid, stream);
    return launch_t<kQuery, kEx, kFf, true, false>(sv, pm, fr, g, m, out, counters, grid, stream);
}

constexpr uint32_t kResolveThreads = 256;

// one lane per slot: key (8 B) and two voxels (16 B each) in, one voxel out, the key only where the slot is evicted.  kFf: the
// anti-firefly clamp in front of the join (sh_resolve_slot_ff, spec S25)
template <bool kFf>
__global__ __launch_bounds__(kResolveThreads) void sharc_resolve_kernel(ShMap m, uint32_t accumulation_frames, uint32_t max_stale_frames)
{
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < m.capacity; slot += gridDim.x * blockDim.x) {
        if (m.keys[slot] == 0u) continue;  // (an empty slot's accumulators were cleared with the array and nothing adds to them)
        const uint4 acc = m.accum[slot], prev = m.resolved[slot];
        bool clear;
        const uint4 r = kFf ? sh_resolve_slot_ff(acc, prev, accumulation_frames, max_stale_frames, clear) : sh_resolve_slot(acc, prev, accumulation_frames, max_stale_frames, clear);
        m.accum[slot] = r;
        if (clear) m.keys[slot] = 0u;
    }
}

}  // namespace

hipError_t launch_sharc_update(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, unsigned long long* counters, uint32_t grid,
                               hipStream_t stream)
{
    return launch_any<false, false, false>(sv, pm, fr, g, m, nullptr, counters, grid, stream);
}

hipError_t launch_sharc_update_ex(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, unsigned long long* counters, uint32_t grid,
                                  bool ff, hipStream_t stream)
{
    if (ff) return launch_any<false, true, true>(sv, pm, fr, g, m, nullptr, counters, grid, stream);
    return launch_any<false, true, false>(sv, pm, fr, g, m, nullptr, counters, grid, stream);
}

hipError_t launch_sharc_query(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, float4* out, unsigned long long* counters,
                              uint32_t grid, hipStream_t stream)
{
    return launch_any<true, false, false>(sv, pm, fr, g, m, out, counters, grid, stream);
}

hipError_t launch_sharc_query_ex(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, float4* out, unsigned long long* counters,
                                 uint32_t grid, hipStream_t stream)
{
    return launch_any<true, true, false>(sv, pm, fr, g, m, out, counters, grid, stream);
}

hipError_t launch_sharc_resolve(const ShMap& m, uint32_t accumulation_frames, uint32_t max_stale_frames, bool ff, hipStream_t stream)
{
    const uint32_t grid = std::min((m.capacity + kResolveThreads - 1u) / kResolveThreads, 4096u);
    if (ff) hipLaunchKernelGGL(sharc_resolve_kernel<true>, dim3(grid), dim3(kResolveThreads), 0, stream, m, accumulation_frames, max_stale_frames);
    else hipLaunchKernelGGL(sharc_resolve_kernel<false>, dim3(grid), dim3(kResolveThreads), 0, stream, m, accumulation_frames, max_stale_frames);
    return hipGetLastError();
}

}  // namespace pt
