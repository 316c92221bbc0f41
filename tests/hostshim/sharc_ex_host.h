// sharc_ex_host.h -- TEST SHIM: one pt_render_sharc_ex call (row N18, DESIGN.md spec S24) over csrc/pt_sharc.h compiled as plain host C++,
// for sharc_ex_host.cpp (the library the tests load) and sharc_ex_sanitize.cpp (the stand-alone sanitizer program).  The scene and the
// frame are sharc_host.h's, and so is the closest-hit test, here behind a conservative cull (CulledTrace).  Not part of the product.
#pragma once

#include "sharc_host.h"

namespace shhost {

// the extras of a call: the DI (null = none: RenderSize texels for a call with the update stage, else rect-sized like `out`), the
// denoiser mode and its outputs (rect-sized, indexed like `out`)
struct Extras {
    const float4* di_diffuse = nullptr;
    const float4* di_specular = nullptr;
    uint32_t mode = 0;
    float* spec_hit_dist = nullptr;
    float4* diffuse = nullptr;
    float4* specular = nullptr;
};

// HostScene::trace behind a conservative cull, so that a scene of tens of thousands of spheres (the tree with the 32-bit stack) stays
// testable: per ray one branch-free pass in double over every sphere, then HostScene::trace's own test on the spheres it keeps.  The
// pass forms intersect_sphere's disc = r^2 - |f + bp d|^2 in double.  intersect_sphere's fp32 disc differs from it by a few
// 2^-24 |f|^2 (each component of l carries a few ulps of |f|), and a sphere is dropped only if the double value lies below
// -1e-4 (|f|^2 + r^2), hundreds of times that error: intersect_sphere would have returned false for it.  A NaN keeps the sphere.
struct CulledTrace {
    const HostScene& hs;
    std::vector<double> cx, cy, cz, r2;
    mutable std::vector<double> keep;

    explicit CulledTrace(const HostScene& scene) : hs(scene)
    {
        const size_t n = hs.sph.size();
        cx.resize(n); cy.resize(n); cz.resize(n); r2.resize(n); keep.resize(n);
        for (size_t i = 0; i < n; i++) { cx[i] = hs.sph[i].x; cy[i] = hs.sph[i].y; cz[i] = hs.sph[i].z; r2[i] = (double)hs.sph[i].w * (double)hs.sph[i].w; }
    }

    // (a function of its own, so that asking for its loop to be vectorised leaves the code of the exact test as the build flags make it)
    __attribute__((noinline, optimize("O3"))) static void cull(size_t n, const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ pz,
                                                               const double* __restrict__ pr, double* __restrict__ k, double ox, double oy, double oz, double dx,
                                                               double dy, double dz)
    {
        for (size_t i = 0; i < n; i++) {
            const double fx = ox - px[i], fy = oy - py[i], fz = oz - pz[i];
            const double bp = -(fx * dx + fy * dy + fz * dz);
            const double lx = fx + bp * dx, ly = fy + bp * dy, lz = fz + bp * dz;
            k[i] = pr[i] - (lx * lx + ly * ly + lz * lz) + 1e-4 * (fx * fx + fy * fy + fz * fz + pr[i]);
        }
    }

    void trace(f3 o, f3 d, float tmin, float tmax, float& t_out, uint32_t& id_out) const
    {
        const size_t n = cx.size();
        const double* k = keep.data();
        cull(n, cx.data(), cy.data(), cz.data(), r2.data(), keep.data(), o.x, o.y, o.z, d.x, d.y, d.z);
        float best = kInf;
        uint32_t best_id = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < (uint32_t)n; i++) {
            if (k[i] < 0.0 || hs.cls[i] == 2u) continue;
            const f3 C = make_f3(hs.sph[i].x, hs.sph[i].y, hs.sph[i].z);
            float t;
            if (!intersect_sphere(o, d, tmin, tmax, C, hs.sph[i].w, t)) continue;
            bool ok = true;
            while (hs.cls[i] == 1u && !hs.crossing_is_opaque(i, C, o, d, t)) {
                float t2;
                if (!intersect_sphere(o, d, t, tmax, C, hs.sph[i].w, t2)) { ok = false; break; }
                t = t2;
            }
            if (ok && t < best) { best = t; best_id = i; }
        }
        t_out = best; id_out = best_id;
    }
};

// run_call of sharc_host.h through the _ex functions, stage by stage as the entry point queues them: the update reads the DI before the
// query writes the outputs, which may be the DI's buffers
inline void run_call_ex(const HostScene& hs, const PtCamera* cam, const Frame& f, uint64_t* keys, uint4* accum, uint4* resolved, float* out, uint64_t* counters,
                        const Extras& x)
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
    if (keys && (f.stages & (kShStageUpdate | kShStageResolve))) std::memset(accum, 0, (size_t)f.capacity * sizeof(uint4));
    const uint32_t gw = f.w / f.downscale, gh = f.h / f.downscale;
    if (keys && (f.stages & kShStageUpdate) && gw && gh) {
        ShFrame fu = fr;
        fu.cam = camera_params(*cam, gw, gh);
        for (uint32_t y = 0; y < gh; y++)
            for (uint32_t xx = 0; xx < gw; xx++) {
                rays = failed = 0;
                sh_update_path_ex(fu, f.g, m, xx, y, trace, material, env, rays, failed);
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
            for (uint32_t xx = 0; xx < f.rect.w; xx++) {
                rays = 0;
                sh_query_pixel_ex(fr, f.g, m, f.rect.x + xx, f.rect.y + y, y * f.rect.w + xx, trace, material, env, rays, reinterpret_cast<float4*>(out));
                counters[0] += rays;
            }
    }
}

}  // namespace shhost
