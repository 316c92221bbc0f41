// sharc_ff_host.h -- TEST SHIM: one pt_render_sharc_ex call with IsAntiFireflyEnabled (row N19, DESIGN.md spec S25) over csrc/pt_sharc.h
// compiled as plain host C++, for sharc_ff_host.cpp (the library the tests load) and sharc_ff_sanitize.cpp (the stand-alone sanitizer
// program).  The scene, the frame, the extras and the culled closest-hit test are sharc_ex_host.h's.  Not part of the product.
#pragma once

#include "sharc_ex_host.h"

namespace shhost {

// run_call_ex of sharc_ex_host.h with the filter's flag: ff = false runs the functions run_call_ex runs; ff = true the update through
// sh_update_path_ff (with or without a DI, as the entry point launches it) and the resolve through sh_resolve_slot_ff.
// ff_counters: {slots the resolve clamped, walks the update's weight threshold stopped} (statistics the device does not keep).
inline void run_call_ff(const HostScene& hs, const PtCamera* cam, const Frame& f, uint64_t* keys, uint4* accum, uint4* resolved, float* out, uint64_t* counters,
                        const Extras& x, bool ff, uint64_t* ff_counters)
{
    const CulledTrace culled(hs);
    auto trace = [&](f3 o, f3 d, float tmin, float tmax, float& t, uint32_t& id) { culled.trace(o, d, tmin, tmax, t, id); };
    auto material = [&](uint32_t id, f3 o, f3 d, float t, bool primary) { return hs.material(id, o, d, t, primary); };
    auto env = [&](f3 d) { return hs.environment(d); };
    ShMap m{};
    m.keys = keys; m.accum = accum; m.resolved = resolved; m.capacity = f.capacity;
    ShFrame fr = f.fr;
    fr.di_diffuse = x.di_diffuse; fr.di_specular = x.di_specular;
    fr.di_w = f.w; fr.di_h = f.h;
    fr.dn_mode = x.mode;
    fr.spec_hit_dist = x.spec_hit_dist; fr.dn_diffuse = x.diffuse; fr.dn_specular = x.specular;
    uint32_t rays = 0, failed = 0;
    counters[0] = counters[1] = 0;
    ff_counters[0] = ff_counters[1] = 0;
    if (keys && (f.stages & (kShStageUpdate | kShStageResolve))) std::memset(accum, 0, (size_t)f.capacity * sizeof(uint4));
    const uint32_t gw = f.w / f.downscale, gh = f.h / f.downscale;
    if (keys && (f.stages & kShStageUpdate) && gw && gh) {
        ShFrame fu = fr;
        fu.cam = camera_params(*cam, gw, gh);
        for (uint32_t y = 0; y < gh; y++)
            for (uint32_t xx = 0; xx < gw; xx++) {
                rays = failed = 0;
                if (ff) ff_counters[1] += sh_update_path_ff(fu, f.g, m, xx, y, trace, material, env, rays, failed);
                else sh_update_path_ex(fu, f.g, m, xx, y, trace, material, env, rays, failed);
                counters[0] += rays; counters[1] += failed;
            }
    }
    if (keys && (f.stages & kShStageResolve)) {
        for (uint32_t s = 0; s < f.capacity; s++) {
            if (keys[s] == 0u) continue;
            bool clear;
            if (ff) {  // (the count from the clamp alone, on a copy; the voxel from the function the kernel calls)
                uint4 a = accum[s];
                ff_counters[0] += sh_ff_clamp(a, resolved[s]) ? 1u : 0u;
            }
            const uint4 r = ff ? sh_resolve_slot_ff(accum[s], resolved[s], f.acc_frames, f.max_stale, clear) : sh_resolve_slot(accum[s], resolved[s], f.acc_frames, f.max_stale, clear);
            accum[s] = r;
            if (clear) keys[s] = 0u;
        }
        std::swap(m.accum, m.resolved);
    }
    if (f.stages & kShStageQuery) {
        for (uint32_t y = 0; y < f.rect.h; y++)
            for (uint32_t xx = 0; xx < f.rect.w; xx++) {
                rays = 0;
                sh_query_pixel_ex(fr, f.g, m, f.rect.x + xx, f.rect.y + y, y * f.rect.w + xx, trace, material, env, rays, reinterpret_cast<float4*>(out));
                counters[0] += rays;
            }
    }
}

}  // namespace shhost
