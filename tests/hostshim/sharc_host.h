// sharc_host.h -- TEST SHIM: the scene and the frame loop that sharc_host.cpp (the library the tests load) and sharc_sanitize.cpp (the
// stand-alone sanitizer program) run csrc/pt_sharc.h with, compiled as plain host C++.  The scene arrives as the C-ABI receives it and is
// converted the way pt_set_scene / pt_set_textures convert it for the device; the closest-hit query is brute force (nearest t, ties ->
// lowest id, the alpha test of spec S10 per crossing), which the device walkers equal bit for bit.  Not part of the product.
#pragma once

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_sharc.h"
#include <cstring>
#include <utility>
#include <vector>

namespace shhost {

using namespace pt;

enum : uint32_t { kShStageUpdate = PT_SHARC_UPDATE, kShStageResolve = PT_SHARC_RESOLVE, kShStageQuery = PT_SHARC_QUERY };

// What a voxel's radiance estimates, sampled without the cache: the radiance one path brings back along the ray (o, d) as the update
// pass would trace it (its roughness floor, no luminance cut-off), every vertex counted.  false: the ray left the scene.  P / front_normal:
// the first vertex, whose voxel the sample belongs to.  
template <typename TraceFn, typename MaterialFn, typename EnvFn>
inline bool sh_path_radiance(const ShFrame& fr, f3 o, f3 d, float tmin, float tmax, uint32_t& rng, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                            f3& radiance, f3& P, f3& front_normal)
{
    f3 T = make_f3(1.0f, 1.0f, 1.0f);
    radiance = make_f3(0.0f, 0.0f, 0.0f);
    for (uint32_t bounce = 0;; bounce++) {
        float t;
        uint32_t id;
        trace(o, d, tmin, tmax, t, id);
        if (id == 0xFFFFFFFFu) {
            if (bounce == 0u) return false;
            radiance = radiance + T * env(d);
            return true;
        }
        HitMaterial hm = material(id, o, d, t, bounce == 0u);
        hm.bsdf.Roughness = pt_max(hm.bsdf.Roughness, fr.roughness_threshold);
        if (bounce == 0u) { P = hm.hf.P; front_normal = hm.hf.front ? hm.hf.N : -hm.hf.N; }
        radiance = radiance + T * hm.emission;
        if (bounce == fr.bounces) return true;
        const Surf surf = surf_init(hm.hf.front, hm.hf.N, hm.Ns);
        const f3 V = -d;
        float w[3];
        lobe_weights(hm.bsdf, surf, V, w);
        float rnd[4];
        rnd[0] = rng_float(rng); rnd[1] = rng_float(rng); rnd[2] = rng_float(rng); rnd[3] = rng_float(rng);
        f3 L;
        int lobe;
        if (!bsdf_sample(hm.bsdf, surf, V, w, rnd, L, lobe)) return true;
        float pdf;
        f3 f;
        if (!bsdf_pdf_eval(hm.bsdf, surf, L, V, w, lobe, pdf, f)) return true;
        if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) return true;
        T = T * (f * pt_rcp(pdf));
        if (fr.rr_enabled && bounce > 3u) {
            const float p = pt_max(T.x, pt_max(T.y, T.z));
            if (rng_float(rng) >= p) return true;
            T = T * pt_rcp(p);
        }
        o = spawn_origin(hm.hf.P, hm.hf.N, hm.hf.offset, L);
        d = L;
        tmin = 0.0f; tmax = kInf;
    }
}

struct HostScene {
    std::vector<float4> sph, mats, rots;
    std::vector<uint32_t> tex_maps, cls;  // cls: 0 visible, 1 tested per crossing, 2 invisible (pt_device.h's alpha classes)
    std::vector<TexView> views;
    float env[4] = { 0, 0, 0, 1 };
    bool tex = false;

    void set(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env_rgba, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
             const uint32_t* maps, const float* rot)
    {
        tex = n_tex != 0;
        for (int k = 0; k < 4; k++) env[k] = env_rgba[k];
        sph.resize(n);
        mats.resize(4 * (size_t)n);
        std::memcpy(sph.data(), spheres, (size_t)n * sizeof(float4));
        if (n_tex) {
            tex_maps.assign((size_t)n * 8u, 0xFFFFFFFFu);
            for (uint32_t i = 0; i < n; i++) tex_maps[(size_t)i * 8u + 7u] = 0u;
            if (maps) std::memcpy(tex_maps.data(), maps, tex_maps.size() * sizeof(uint32_t));
        }
        cls.assign(n, 0u);
        for (uint32_t i = 0; i < n; i++) {
            PtMaterial m = materials[i];
            const float f0d = dielectric_f0(m.IOR), inv_ior = 1.0f / m.IOR;
            std::memcpy(&m._pad[0], &f0d, 4);
            std::memcpy(&m._pad[1], &inv_ior, 4);
            m.AlphaMode &= ~kMaterialHasMaps;
            if (n_tex && tex_maps[(size_t)i * 8u + 7u]) m.AlphaMode |= kMaterialHasMaps;
            std::memcpy(&mats[4 * (size_t)i], &m, sizeof m);
            if (materials[i].AlphaMode != PT_ALPHA_OPAQUE) {
                const float* bc = materials[i].BaseColor;
                const bool sampled = n_tex && tex_maps[(size_t)i * 8u + kMapBaseColor] != kNoTexture && (bc[0] > 0.0f || bc[1] > 0.0f || bc[2] > 0.0f || bc[3] > 0.0f);
                cls[i] = sampled ? 1u : (bc[3] >= materials[i].AlphaCutoff ? 0u : 2u);
            }
        }
        views.resize(n_tex);
        for (uint32_t k = 0; k < n_tex; k++) views[k] = TexView{ reinterpret_cast<const float4*>(texels) + tex_info[3 * k], tex_info[3 * k + 1], tex_info[3 * k + 2] };
        rots.resize(n);
        for (uint32_t i = 0; i < n; i++) { rots[i].x = rots[i].y = rots[i].z = 0.0f; rots[i].w = 1.0f; }
        if (rot) std::memcpy(rots.data(), rot, (size_t)n * sizeof(float4));
    }

    bool crossing_is_opaque(uint32_t id, f3 C, f3 o, f3 d, float t) const
    {
        const float base_alpha = mats[id * 4 + 0].w, cutoff = mats[id * 4 + 3].y;
        const uint32_t map = tex_maps[(size_t)id * 8u + kMapBaseColor];
        const f3 N = normalize(mad(t, d, o) - C);
        float4 q;
        f3 n_mesh;
        const f2 uv = hit_uv_rot(rots.data(), id, N, q, n_mesh);
        float s[4];
        sample_bilinear(views[map], uv, s);
        return base_alpha * s[3] >= cutoff;
    }

    void trace(f3 o, f3 d, float tmin, float tmax, float& t_out, uint32_t& id_out) const
    {
        float best = kInf;
        uint32_t best_id = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < (uint32_t)sph.size(); i++) {
            if (cls[i] == 2u) continue;
            const f3 C = make_f3(sph[i].x, sph[i].y, sph[i].z);
            float t;
            if (!intersect_sphere(o, d, tmin, tmax, C, sph[i].w, t)) continue;
            bool ok = true;
            while (cls[i] == 1u && !crossing_is_opaque(i, C, o, d, t)) {
                float t2;
                if (!intersect_sphere(o, d, t, tmax, C, sph[i].w, t2)) { ok = false; break; }
                t = t2;
            }
            if (ok && t < best) { best = t; best_id = i; }
        }
        t_out = best; id_out = best_id;
    }

    HitMaterial material(uint32_t id, f3 o, f3 d, float t, bool primary) const
    {
        return tex ? hit_material_at<true>(sph.data(), mats.data(), views.data(), tex_maps.data(), rots.data(), id, o, d, t, primary)
                   : hit_material_at<false>(sph.data(), mats.data(), nullptr, nullptr, nullptr, id, o, d, t, primary);
    }

    f3 environment(f3 d) const { return environment_color(env[0], env[1], env[2], env[3], d); }
};

// prm = {RenderSize w, h, FrameIndex, Bounces, SamplesPerPixel, IsRussianRouletteEnabled, capacity, DownscaleFactor, AccumulationFrames,
//        MaxStaleFrames, IsHashGridVisualizationEnabled, stages, rect x, y, w, h}, defaults applied;
// fprm = {ThroughputThreshold, SceneScale, RoughnessThreshold}
struct Frame {
    ShFrame fr{};
    ShGrid g{};
    uint32_t w, h, capacity, downscale, acc_frames, max_stale, stages;
    PtRect rect;

    Frame(const PtCamera* cam, const uint32_t* prm, const float* fprm)
    {
        w = prm[0]; h = prm[1];
        fr.cam = camera_params(*cam, w, h);
        fr.frame_index = prm[2]; fr.bounces = prm[3]; fr.spp = prm[4]; fr.rr_enabled = prm[5];
        fr.throughput_threshold = fprm[0];
        fr.inv_spp = 1.0f / (float)fr.spp;
        fr.roughness_threshold = fprm[2];
        fr.visualize = prm[10];
        g.cam_pos = make_f3(cam->Position[0], cam->Position[1], cam->Position[2]);
        g.scene_scale = fprm[1];
        capacity = prm[6]; downscale = prm[7]; acc_frames = prm[8]; max_stale = prm[9]; stages = prm[11];
        rect = PtRect{ prm[12], prm[13], prm[14], prm[15] };
    }
};

// One pt_render_sharc call over caller-owned arrays, stage by stage as the entry point queues them.  keys = null: the cache is off
// (query only).  accum / resolved swap at the resolve, as the context's arrays do: the caller swaps its own pointers after a call with
// the resolve stage.  out: rect.w * rect.h float4.  counters: {rays, failed inserts}.
inline void run_call(const HostScene& hs, const PtCamera* cam, const Frame& f, uint64_t* keys, uint4* accum, uint4* resolved, float* out, uint64_t* counters)
{
    auto trace = [&](f3 o, f3 d, float tmin, float tmax, float& t, uint32_t& id) { hs.trace(o, d, tmin, tmax, t, id); };
    auto material = [&](uint32_t id, f3 o, f3 d, float t, bool primary) { return hs.material(id, o, d, t, primary); };
    auto env = [&](f3 d) { return hs.environment(d); };
    ShMap m{};
    m.keys = keys; m.accum = accum; m.resolved = resolved; m.capacity = f.capacity;
    uint32_t rays = 0, failed = 0;
    counters[0] = counters[1] = 0;
    if (keys && (f.stages & (kShStageUpdate | kShStageResolve))) std::memset(accum, 0, (size_t)f.capacity * sizeof(uint4));
    const uint32_t gw = f.w / f.downscale, gh = f.h / f.downscale;
    if (keys && (f.stages & kShStageUpdate) && gw && gh) {
        ShFrame fu = f.fr;
        fu.cam = camera_params(*cam, gw, gh);
        for (uint32_t y = 0; y < gh; y++)
            for (uint32_t x = 0; x < gw; x++) {
                rays = failed = 0;
                sh_update_path(fu, f.g, m, x, y, trace, material, env, rays, failed);
                counters[0] += rays; counters[1] += failed;
            }
    }
    if (keys && (f.stages & kShStageResolve)) {
        for (uint32_t s = 0; s < f.capacity; s++) {
            if (keys[s] == 0u) continue;
            bool clear;
            const uint4 r = sh_resolve_slot(accum[s], resolved[s], f.acc_frames, f.max_stale, clear);
            accum[s] = r;
            if (clear) keys[s] = 0u;
        }
        std::swap(m.accum, m.resolved);
    }
    if (f.stages & kShStageQuery) {
        for (uint32_t y = 0; y < f.rect.h; y++)
            for (uint32_t x = 0; x < f.rect.w; x++) {
                rays = 0;
                const f3 c = sh_query_pixel(f.fr, f.g, m, f.rect.x + x, f.rect.y + y, trace, material, env, rays);
                counters[0] += rays;
                float* px = out + 4u * ((size_t)y * f.rect.w + x);
                px[0] = c.x; px[1] = c.y; px[2] = c.z; px[3] = 1.0f;
            }
    }
}

}  // namespace shhost
