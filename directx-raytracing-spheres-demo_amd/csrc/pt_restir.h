// pt_restir.h -- the reservoir pass that makes row N10's direct light (pt_restir_di, DESIGN.md spec S16): a stand-in for the RTXDI
// passes the reference runs before its frame (DIInitialSampling.hlsl, DITemporalResampling.hlsl, DISpatialResampling.hlsl,
// DIFinalShading.hlsl over Shaders/RTXDIAppBridge.hlsli; the RTXDI SDK itself is a submodule the reference tree does not contain).
// Per-pixel functions, one per pass, that compile on the device (pt_restir.hip) and as host C++ (the bit-parity tests); the
// visibility query is a functor `trace(o, d, t, id)` -- the ordinary closest-hit query, as di_estimate takes it -- and the radiance
// of the point a visibility ray reached a functor `emit(sphere, o, d, t)`.
//
// A sample is (emitter j of the scene's emitter list, u1, u2); at a surface it becomes a direction through sample_sphere_cone, so a
// reused sample is re-aimed from the surface that reuses it.  Target function: luminance((Le_j (f_d + f_s)) inv_pdf), Le_j the
// emitter's untextured radiance, without visibility.
//
// The initial candidates come from one of three sources (row N16, spec S22, pt_lightris.h): uniformly from the emitter list (S16 as
// it was; pt_restir_di), from a Power_RIS tile, or from a ReGIR cell with the Power_RIS tile as its fallback (pt_restir_di_sampled).
//
// Row N17 (spec S23, pt_restir_di_ex): BRDF candidates mixed into initial sampling by the balance heuristic (ri_initial_mis) and the
// boiling filter over launch 1's temporal result (ri_boiling_*); both off: the code of rows N10 / N16, untouched.
//
// Row N22 (spec S26, pt_restir_di_full): the visibility word a reservoir carries and final shading's reuse of it (ri_vis_*,
// ri_final_reuse), and pairwise MIS (bias mode 2: ri_temporal_pairwise, ri_spatial_pairwise).  The arithmetic is this project's own,
// written from the reference's shaders and from recollection of RTXDI (the SDK is not vendored): no parity with the SDK is claimed.
// Both live in launches of their own (ri_pass1_full_*, ri_pass2_full_px); the functions of rows N10 / N16 / N17 compile as they did.
//
// Out of scope: ReGIR's onion mode; environment candidates (the reference's bridge stubs them to 0, RTXDIAppBridge.hlsli:503-511);
// checkerboard rendering; writing the final ray's result back into the history; discardInvisibleSamples; a ray-traced pairwise
// variant; the DLSS-RR SpecularHitDistance write; dropping pt_render_with_di's whole-stream wait for buffers this pass produced.
#pragma once

#include "pt_light.h"
#include "pt_lightris.h"
#include "pt_texture.h"

namespace pt {

constexpr uint32_t kRiInitialRngSalt = 0x52494E31u;   // each pass has its own per-pixel stream: rng_init(px, py, FrameIndex ^ salt)
constexpr uint32_t kRiTemporalRngSalt = 0x52495431u;
constexpr uint32_t kRiSpatialRngSalt = 0x52495331u;
constexpr float kRiMinRoughness = 0.05f;       // RAB_GetGBufferSurface: mirror-like pixels get no DI (RTXDIAppBridge.hlsli:295)
constexpr float kRiDepthThreshold = 0.1f;      // reuse: relative depth difference accepted
constexpr float kRiNormalThreshold = 0.5f;     // reuse: dot of the shading normals accepted
constexpr uint32_t kRiNoHit = 0xFFFFFFFFu;
constexpr float kRiOwnSphere = 1e-3f;          // |d^2 - r^2| <= this * r^2: the surface lies on the emitter itself
constexpr uint32_t kRiDefaultInitialSamples = 8, kRiMaxInitialSamples = 32, kRiDefaultHistory = 20, kRiDefaultSpatialSamples = 1,
                   kRiMaxSpatialSamples = 32, kRiNeighbourTable = 32;
constexpr float kRiDefaultRadius = 32.0f, kRiMaxRadius = 16384.0f;
constexpr uint32_t kRiMaxBrdfSamples = 8;
constexpr float kRiMinU = 5.9604644775390625e-08f;  // 2^-24: the lower clamp of an inverted cone sample (u1, u2 lie in (0, 1])
enum : uint32_t { kRiBiasOff = 0, kRiBiasBasic = 1, kRiBiasPairwise = 2, kRiBiasRaytraced = 3 };

// The compact surface record the first launch writes per pixel (four float4 planes and one float plane): later passes and the next
// frame's temporal pass read it instead of eight G-buffer channels.  depth = +inf: no surface.
struct RiRecord {
    float4 r0;  // P, PositionOffset
    float4 r1;  // shading normal, roughness
    float4 r2;  // base colour, metalness
    float4 r3;  // geometric normal (signed octahedral), linear depth, IOR
    float transmission;
};

struct RiReservoir {
    uint32_t light;  // index into the emitter list
    float u1, u2;    // the cone sample
    float W;         // unbiased contribution weight; 0: the sample carries no light
    float M;         // candidates seen
    float p_hat;     // target function of the sample at the surface that holds it
    uint32_t age;    // frames since the sample was drawn
    uint32_t vis;    // row N22: what is known of the sample's visibility (ri_vis_*); 0: nothing -- all that rows N10 / N16 / N17 write
};

struct RiBuffers {
    uint32_t w, h;
    // what RAB_GetGBufferSurface reads, as pt_render_gbuffer writes it (first launch only)
    const float4* position;
    const float* geometric_normal;  // float2
    const float* linear_depth;
    const float* motion_vector;     // float3
    const float4* base_color_metalness;
    const float4* normal_roughness;
    const float* ior;
    const float* transmission;
    // the context's history: this call's slot and the previous call's
    float4* rec[4];
    float* rec_t;
    float4* res[2];
    const float4* prev_rec[4];
    const float* prev_rec_t;
    const float4* prev_res[2];
    float4* out_diffuse;
    float4* out_specular;
};

struct RiScene {
    const float4* sph;        // original order
    const float4* mats;       // PtMaterial as 4 float4
    const uint32_t* lights;   // ids of the emissive spheres
    uint32_t n_lights;
    LrView lr;                // the presampled candidates of spec S22 (read by ri_initial<kLrPowerRis / kLrRegirRis> only; all zero: none)
    // row N17 (read by ri_initial_mis only; null / 0: BRDF candidates are off)
    const uint32_t* light_of; // per sphere: its index in `lights`, or kRiNoHit
    const float* pyramid;     // S22's power pyramid, every level (the presampled modes: the source pdf of an emitter a BRDF ray found)
    uint32_t pyramid_levels;
    // row N22 (read by ri_final_reuse only): per sphere its alpha class (pt_device.h; 0: every crossing is accepted), or null: all 0
    const uint32_t* alpha_class;
};

struct RiParams {
    uint32_t frame_index, initial_samples, temporal, temporal_bias, max_history, spatial, spatial_bias, spatial_samples;
    float radius;
    uint32_t history_valid;   // 0: the history restarts with this call
    f3 cam_pos, prev_cam_pos;
};

// ... with what row N17 adds (launch 1 of pt_restir_di_ex; the launches of rows N10 / N16 keep RiParams as their argument); all zero: off
struct RiParamsEx : RiParams {
    uint32_t brdf_samples;    // BRDF candidates of initial sampling
    uint32_t boiling_filter;
    float boiling_strength;
};

// ... and with what row N22 adds (the launches of pt_restir_di_full): final shading's reuse of the visibility word
struct RiShading {
    uint32_t reuse;           // 0: every final ray is cast
    uint32_t max_age;         // the sample's age at most this ...
    float max_dist2;          // ... and the square of its pixel offset at most this (MaxDistance * MaxDistance in float32)
};
struct RiParamsFull : RiParamsEx {
    RiShading sh;
};

PT_HD float4 ri_float4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

// Packing::DecodeUnitVector(v, true): the inverse of encode_unit_vector (pt_gbuffer.h)
PT_HD f3 decode_unit_vector(float ex, float ey)
{
    const float z = 1.0f - pt_abs(ex) - pt_abs(ey);
    float x = ex, y = ey;
    if (z < 0.0f) {
        x = (1.0f - pt_abs(ey)) * (ex >= 0.0f ? 1.0f : -1.0f);
        y = (1.0f - pt_abs(ex)) * (ey >= 0.0f ? 1.0f : -1.0f);
    }
    return normalize(make_f3(x, y, z));
}

PT_HD RiRecord ri_empty_record()
{
    RiRecord r;
    r.r0 = r.r1 = r.r2 = ri_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.r3 = ri_float4(0.0f, 0.0f, kInf, 1.0f);
    r.transmission = 0.0f;
    return r;
}

// RAB_GetGBufferSurface's reads (RTXDIAppBridge.hlsli:292-331)
PT_HD RiRecord ri_record_from_gbuffer(const RiBuffers& b, uint32_t i)
{
    const float depth = b.linear_depth[i];
    if (!is_finite(depth)) return ri_empty_record();
    const float4 nr = b.normal_roughness[i];
    if (nr.w < kRiMinRoughness) return ri_empty_record();
    RiRecord r;
    r.r0 = b.position[i];
    r.r1 = nr;
    r.r2 = b.base_color_metalness[i];
    r.r3 = ri_float4(b.geometric_normal[2u * i], b.geometric_normal[2u * i + 1u], depth, b.ior[i]);
    r.transmission = r.r2.w < 1.0f ? b.transmission[i] : 0.0f;
    return r;
}

PT_HD void ri_store_record(float4* const rec[4], float* rec_t, uint32_t i, const RiRecord& r)
{
    rec[0][i] = r.r0; rec[1][i] = r.r1; rec[2][i] = r.r2; rec[3][i] = r.r3;
    rec_t[i] = r.transmission;
}

template <typename P4>
PT_HD RiRecord ri_load_record(P4 const rec[4], const float* rec_t, uint32_t i)
{
    RiRecord r;
    r.r3 = rec[3][i];
    if (!is_finite(r.r3.z)) return ri_empty_record();
    r.r0 = rec[0][i]; r.r1 = rec[1][i]; r.r2 = rec[2][i];
    r.transmission = r.r2.w < 1.0f ? rec_t[i] : 0.0f;
    return r;
}

PT_HD RiReservoir ri_empty_reservoir()
{
    RiReservoir r;
    r.light = 0u; r.u1 = r.u2 = 1.0f; r.W = 0.0f; r.M = 0.0f; r.p_hat = 0.0f; r.age = 0u; r.vis = 0u;
    return r;
}

PT_HD void ri_store_reservoir(float4* const res[2], uint32_t i, const RiReservoir& r)
{
    res[0][i] = ri_float4(as_float(r.light), r.u1, r.u2, r.W);
    res[1][i] = ri_float4(r.M, r.p_hat, as_float(r.age), as_float(r.vis));
}

template <typename P4>
PT_HD RiReservoir ri_load_reservoir(P4 const res[2], uint32_t i)
{
    const float4 a = res[0][i], c = res[1][i];
    RiReservoir r;
    r.light = as_uint(a.x); r.u1 = a.y; r.u2 = a.z; r.W = a.w; r.M = c.x; r.p_hat = c.y; r.age = as_uint(c.z); r.vis = as_uint(c.w);
    return r;
}

// RAB_Surface: what every candidate of a pixel shares (view vector, SurfaceVectors, BSDFSample, lobe weights)
struct RiSurface {
    bool valid;
    f3 P, Ng;
    float offset, depth;
    f3 V;
    Surf surf;
    Bsdf bsdf;
    float w[3];
};

// RTXDIAppBridge.hlsli:333-345
PT_HD RiSurface ri_surface(const RiRecord& r, f3 cam_pos)
{
    RiSurface s;
    s.valid = is_finite(r.r3.z);
    s.P = make_f3(r.r0.x, r.r0.y, r.r0.z);
    s.offset = r.r0.w;
    s.depth = r.r3.z;
    s.Ng = make_f3(0.0f, 0.0f, 1.0f);
    s.V = s.Ng;
    if (!s.valid) {
        s.surf = surf_init(true, s.Ng, s.Ng);
        s.bsdf = bsdf_init(make_f3(0.0f, 0.0f, 0.0f), 0.0f, 1.0f, 1.5f, 0.0f, true);
        s.w[0] = s.w[1] = s.w[2] = 0.0f;
        return s;
    }
    s.V = normalize(cam_pos - s.P);
    s.Ng = decode_unit_vector(r.r3.x, r.r3.y);
    const bool front = dot(s.Ng, s.V) > 0.0f;
    s.surf = surf_init(front, s.Ng, make_f3(r.r1.x, r.r1.y, r.r1.z));
    s.bsdf = bsdf_init(make_f3(r.r2.x, r.r2.y, r.r2.z), r.r2.w, r.r1.w, r.r3.w, r.transmission, front);
    lobe_weights(s.bsdf, s.surf, s.V, s.w);
    return s;
}

// a sample aimed from a surface: RAB_SamplePolymorphicLight + RAB_GetLightSampleTargetPdfForSurface
struct RiShade {
    uint32_t sphere;   // the emitter's sphere id
    f3 L;
    float inv_pdf;
    f3 f_d, f_s;       // the two reflective lobes times cos; zero where the sample carries nothing
    f3 le;             // the emitter's untextured radiance
    float p_hat;
};

PT_HD RiShade ri_shade(const RiScene& sc, const RiSurface& s, uint32_t j, float u1, float u2)
{
    RiShade e;
    e.sphere = sc.lights[j < sc.n_lights ? j : sc.n_lights - 1u];
    const float4 ls = sc.sph[e.sphere];
    const float4 lm = sc.mats[e.sphere * 4u + 1u];  // {EmissiveStrength, EmissiveColor}
    e.le = make_f3(lm.y, lm.z, lm.w) * lm.x;
    const f3 C = make_f3(ls.x, ls.y, ls.z);
    const LightSample c = sample_sphere_cone(s.P, C, ls.w, u1, u2);
    e.L = c.L;
    e.inv_pdf = c.inv_pdf;
    e.f_d = e.f_s = make_f3(0.0f, 0.0f, 0.0f);
    e.p_hat = 0.0f;
    const f3 wv = C - s.P;
    const float r2 = ls.w * ls.w;
    const bool own = pt_abs(dot(wv, wv) - r2) <= kRiOwnSphere * r2;
    if (s.valid && c.valid && !own && dot(s.surf.FrontNg, c.L) > 0.0f) {
        bsdf_eval_reflective_lobes(s.bsdf, s.surf, c.L, s.V, s.w, e.f_d, e.f_s);
        const float p = luminance((e.le * (e.f_d + e.f_s)) * c.inv_pdf);
        if (p > 0.0f && is_finite(p)) e.p_hat = p;
        else e.f_d = e.f_s = make_f3(0.0f, 0.0f, 0.0f);
    }
    return e;
}

// N4's visibility rule: the emitter must be the first thing a closest-hit ray from the spawn origin meets
template <typename TraceFn>
PT_HD bool ri_visible(const RiSurface& s, const RiShade& e, TraceFn&& trace, f3& so, float& t2)
{
    so = spawn_origin(s.P, s.Ng, s.offset, e.L);
    uint32_t id2 = kRiNoHit;
    t2 = kInf;
    trace(so, e.L, t2, id2);
    return id2 == e.sphere;
}

// one step of streaming RIS: returns true when the candidate replaces the selected sample
PT_HD bool ri_stream(float& w_sum, float w, float rnd)
{
    w_sum += w;
    return w > 0.0f && rnd * w_sum <= w;
}

// ---- initial sampling (DIInitialSampling.hlsl): InitialSamples candidates through RIS, one visibility ray.  kMode = the candidates'
// source (spec S22): uniform over the emitter list (source weight n_lights), an entry of the pixel block's Power_RIS tile, or an entry
// of the ReGIR cell of the jittered surface point (outside the grid: the Power_RIS tile).  The per-candidate draws are (u0, u1, u2, rnd)
// in every mode; an invalid entry weighs 0 and still counts in M.
template <uint32_t kMode = kLrUniform, typename TraceFn>
PT_HD RiReservoir ri_initial(const RiScene& sc, const RiParams& p, const RiSurface& s, uint32_t px, uint32_t py, TraceFn&& trace)
{
    RiReservoir r = ri_empty_reservoir();
    float w_sum = 0.0f;
    uint32_t rng = rng_init(px, py, p.frame_index ^ kRiInitialRngSalt);
    const float nl = (float)sc.n_lights;
    const LrEntry* src = nullptr;  // the tile or cell the pixel's candidates come from
    uint32_t src_n = 0u;
    if (kMode != kLrUniform) {
        bool in_cell = false;
        if (kMode == kLrRegirRis) {
            const float x0 = rng_float(rng), x1 = rng_float(rng), x2 = rng_float(rng);
            uint32_t cell = 0u;
            in_cell = lr_cell_of(s.P, make_f3(x0, x1, x2), p.cam_pos, sc.lr.grid, sc.lr.cell_size, cell);
            if (in_cell) {
                src = sc.lr.ris + ((size_t)sc.lr.tile_size * sc.lr.tile_count + (size_t)cell * sc.lr.lights_per_cell);
                src_n = sc.lr.lights_per_cell;
            }
        }
        if (!in_cell) {
            src = sc.lr.ris + (size_t)lr_pixel_tile(px, py, p.frame_index, sc.lr.tile_count) * sc.lr.tile_size;
            src_n = sc.lr.tile_size;
        }
    }
    for (uint32_t i = 0; i < p.initial_samples; i++) {
        const float u0 = rng_float(rng), u1 = rng_float(rng), u2 = rng_float(rng), rnd = rng_float(rng);
        if (kMode == kLrUniform) {
            const uint32_t j = pick_light(u0, sc.n_lights);
            const RiShade e = ri_shade(sc, s, j, u1, u2);
            if (ri_stream(w_sum, e.p_hat * nl, rnd)) { r.light = j; r.u1 = u1; r.u2 = u2; r.p_hat = e.p_hat; }
        } else {
            const LrEntry c = src[pick_light(u0, src_n)];
            float w = 0.0f, p_hat = 0.0f;
            if (c.light != kLrInvalid) {
                p_hat = ri_shade(sc, s, c.light, u1, u2).p_hat;
                w = p_hat * c.inv_pdf;
            }
            if (ri_stream(w_sum, w, rnd)) { r.light = c.light; r.u1 = u1; r.u2 = u2; r.p_hat = p_hat; }
        }
    }
    r.M = (float)p.initial_samples;
    r.W = r.p_hat > 0.0f ? w_sum / (r.M * r.p_hat) : 0.0f;
    if (r.W > 0.0f) {  // enableInitialVisibility: an occluded sample keeps M and carries nothing
        const RiShade e = ri_shade(sc, s, r.light, r.u1, r.u2);
        f3 so;
        float t2;
        if (!ri_visible(s, e, trace, so, t2)) r.W = 0.0f;
    }
    return r;
}

// ---- row N17 (spec S23): BRDF candidates and the boiling filter
// The inverse of sample_sphere_cone: the (u1, u2) whose direction from P towards the sphere (C, r) is L.  1 - cos(theta) is formed
// as (lx^2 + ly^2) / (1 + lz) in the basis of the cone's axis -- the forward function's cancellation-free form.  P inside the sphere: (1, 1).
PT_HD void invert_sphere_cone(f3 P, f3 C, float r, f3 L, float& u1, float& u2)
{
    u1 = u2 = 1.0f;
    const f3 w = C - P;
    const float d2 = dot(w, w), r2 = r * r;
    if (!(d2 > r2)) return;
    const f3 wn = w * pt_rcp(pt_sqrt(d2));
    const float sin2 = r2 / d2;
    const float cos_max = sqrt01(1.0f - sin2);
    const float omc = sin2 / (1.0f + cos_max);
    const f3 l = rotate_vector(get_basis(wn), L);
    const float k = (l.x * l.x + l.y * l.y) / (1.0f + l.z);
    const float a = k / omc;
    u1 = !(a > kRiMinU) ? kRiMinU : (a > 1.0f ? 1.0f : a);
    float t = atan2_spec(l.y, l.x) * 0.15915494309189533577f;
    if (!(t > 0.0f)) t += 1.0f;
    u2 = !(t > kRiMinU) ? kRiMinU : (t > 1.0f ? 1.0f : t);
}

// the pdf with which the light technique proposes emitter j, as the BRDF side prices it: 1 / n_lights, or in the presampled modes
// power_j / sum of powers from S22's pyramid (leaf over top; the top is the mean of 4^levels leaves) -- RAB_EvaluateLocalLightSourcePdf
template <uint32_t kMode>
PT_HD float ri_source_pdf(const RiScene& sc, uint32_t j)
{
    if (kMode == kLrUniform) return 1.0f / (float)sc.n_lights;
    const float top = sc.pyramid[lr_level_offset(sc.pyramid_levels, sc.pyramid_levels)] * (float)lr_level_size(sc.pyramid_levels, 0u);
    return top > 0.0f ? sc.pyramid[j] / top : 0.0f;
}

// the balance-heuristic RIS weight of a candidate: p_hat over the mixture density of its (emitter, u1, u2); 0 where it carries nothing
PT_HD float ri_mis_weight(float p_hat, float w_l, float p_src, float w_b, float p_brdf, float inv_pdf)
{
    if (!(p_hat > 0.0f)) return 0.0f;
    const float w = p_hat / (w_l * p_src + w_b * (p_brdf * inv_pdf));
    return w > 0.0f && is_finite(w) ? w : 0.0f;
}

// Initial sampling with p.brdf_samples BRDF candidates behind the p.initial_samples local ones.  The local candidates' draws and source
// are ri_initial's; a BRDF candidate draws (r0, r1, r2, r3, rnd), and where bsdf_sample's direction leaves above the geometric horizon
// a closest-hit ray looks for an emitter: the candidate is then (emitter, invert_sphere_cone), shaded like any other.  One loop casts
// the BRDF rays and, as its last turn, the selected sample's visibility ray: one walker call site.
template <uint32_t kMode, typename TraceFn>
PT_HD RiReservoir ri_initial_mis(const RiScene& sc, const RiParamsEx& p, const RiSurface& s, uint32_t px, uint32_t py, TraceFn&& trace)
{
    RiReservoir r = ri_empty_reservoir();
    float w_sum = 0.0f;
    uint32_t rng = rng_init(px, py, p.frame_index ^ kRiInitialRngSalt);
    const float n_all = (float)(p.initial_samples + p.brdf_samples);
    const float w_l = (float)p.initial_samples / n_all, w_b = (float)p.brdf_samples / n_all;
    const LrEntry* src = nullptr;
    uint32_t src_n = 0u;
    if (kMode != kLrUniform) {
        bool in_cell = false;
        if (kMode == kLrRegirRis) {
            const float x0 = rng_float(rng), x1 = rng_float(rng), x2 = rng_float(rng);
            uint32_t cell = 0u;
            in_cell = lr_cell_of(s.P, make_f3(x0, x1, x2), p.cam_pos, sc.lr.grid, sc.lr.cell_size, cell);
            if (in_cell) {
                src = sc.lr.ris + ((size_t)sc.lr.tile_size * sc.lr.tile_count + (size_t)cell * sc.lr.lights_per_cell);
                src_n = sc.lr.lights_per_cell;
            }
        }
        if (!in_cell) {
            src = sc.lr.ris + (size_t)lr_pixel_tile(px, py, p.frame_index, sc.lr.tile_count) * sc.lr.tile_size;
            src_n = sc.lr.tile_size;
        }
    }
    for (uint32_t i = 0; i < p.initial_samples; i++) {
        const float u0 = rng_float(rng), u1 = rng_float(rng), u2 = rng_float(rng), rnd = rng_float(rng);
        uint32_t j = kLrInvalid;
        float p_sel = 0.0f;
        if (kMode == kLrUniform) {
            j = pick_light(u0, sc.n_lights);
            p_sel = 1.0f / (float)sc.n_lights;
        } else {
            const LrEntry c = src[pick_light(u0, src_n)];
            j = c.light;
            p_sel = 1.0f / c.inv_pdf;
        }
        float w = 0.0f, p_hat = 0.0f;
        if (j != kLrInvalid) {
            const RiShade e = ri_shade(sc, s, j, u1, u2);
            p_hat = e.p_hat;
            if (p_hat > 0.0f) w = ri_mis_weight(p_hat, w_l, p_sel, w_b, bsdf_pdf_all(s.bsdf, s.surf, e.L, s.V, s.w), e.inv_pdf);
        }
        if (ri_stream(w_sum, w, rnd)) { r.light = j; r.u1 = u1; r.u2 = u2; r.p_hat = p_hat; }
    }
    for (uint32_t k = 0; k <= p.brdf_samples; k++) {
        const bool last = k == p.brdf_samples;
        f3 L = make_f3(0.0f, 0.0f, 1.0f);
        float rnd = 1.0f;
        uint32_t want = kRiNoHit;
        bool cast = false;
        if (!last) {
            float q[4];
            q[0] = rng_float(rng); q[1] = rng_float(rng); q[2] = rng_float(rng); q[3] = rng_float(rng);
            rnd = rng_float(rng);
            int lobe;
            cast = bsdf_sample(s.bsdf, s.surf, s.V, s.w, q, L, lobe) && dot(s.surf.FrontNg, L) > 0.0f;
        } else {
            r.M = n_all;
            r.W = r.p_hat > 0.0f ? w_sum / (r.M * r.p_hat) : 0.0f;
            if (r.W > 0.0f) {  // enableInitialVisibility, whichever technique produced the sample
                const RiShade e = ri_shade(sc, s, r.light, r.u1, r.u2);
                L = e.L;
                want = e.sphere;
                cast = true;
            }
        }
        uint32_t id = kRiNoHit;
        float t = kInf;
        if (cast) trace(spawn_origin(s.P, s.Ng, s.offset, L), L, t, id);
        if (last) {
            if (cast && id != want) r.W = 0.0f;
        } else {
            float w = 0.0f, p_hat = 0.0f, u1 = 1.0f, u2 = 1.0f;
            uint32_t j = kRiNoHit;
            if (cast && id != kRiNoHit) j = sc.light_of[id];
            if (j != kRiNoHit) {
                const float4 ls = sc.sph[id];
                invert_sphere_cone(s.P, make_f3(ls.x, ls.y, ls.z), ls.w, L, u1, u2);
                const RiShade e = ri_shade(sc, s, j, u1, u2);
                p_hat = e.p_hat;
                if (p_hat > 0.0f) w = ri_mis_weight(p_hat, w_l, ri_source_pdf<kMode>(sc, j), w_b, bsdf_pdf_all(s.bsdf, s.surf, e.L, s.V, s.w), e.inv_pdf);
            }
            if (ri_stream(w_sum, w, rnd)) { r.light = j; r.u1 = u1; r.u2 = u2; r.p_hat = p_hat; }
        }
    }
    return r;
}

// The boiling filter (DITemporalResampling.hlsl:41-46) over one 8x8 pixel block = one wave64: a reservoir whose W exceeds the mean
// of the block's nonzero W times the multiplier is emptied.
PT_HD float ri_boiling_multiplier(float strength)
{
    const float s = !(strength > 1e-6f) ? 1e-6f : (strength > 1.0f ? 1.0f : strength);
    return 10.0f / s - 9.0f;
}
PT_HD bool ri_boiled(float W, float sum, uint32_t n, float mult)
{
    const float avg = n ? sum / (float)n : 0.0f;
    return W > avg * mult;
}
// the host form of the wave's reduction: six butterfly levels, level k adding the partial sums of lanes that differ in bit k of the
// block's row-major lane index (what __shfl_xor(v, 1 << k) does); every lane ends with the same bits, lane 0's are returned
inline float ri_boiling_sum64(const float w[64], uint32_t& n)
{
    float v[64], t[64];
    n = 0u;
    for (uint32_t l = 0; l < 64u; l++) { v[l] = w[l]; n += w[l] > 0.0f ? 1u : 0u; }
    for (uint32_t k = 0; k < 6u; k++) {
        for (uint32_t l = 0; l < 64u; l++) t[l] = v[l] + v[l ^ (1u << k)];
        for (uint32_t l = 0; l < 64u; l++) v[l] = t[l];
    }
    return v[0];
}

// ---- row N22 (spec S26, part 1): the visibility word.  Bit 0: the visibility ray cast from the surface that drew the sample reached
// its emitter; bits 8-15 and 16-23: the pixel offset (dx, dy) the sample has travelled since, each a biased int8 (value + 128, |value|
// <= 127) where 0 means saturated and stays so.  The word 0 therefore says nothing and moves to itself.
constexpr uint32_t kRiVisSeen = 1u;
constexpr uint32_t kRiVisFresh = kRiVisSeen | (128u << 8) | (128u << 16);  // seen by this pixel: offset (0, 0)

PT_HD uint32_t ri_vis_axis(uint32_t byte, int d)
{
    if (byte == 0u) return 0u;
    d = d < -256 ? -256 : (d > 256 ? 256 : d);
    const int v = (int)byte - 128 + d;
    return v < -127 || v > 127 ? 0u : (uint32_t)(v + 128);
}
// the word of a sample that pixel (x + dx, y + dy) takes from pixel (x, y)
PT_HD uint32_t ri_vis_moved(uint32_t vis, int dx, int dy)
{
    return (vis & 0xFF0000FFu) | (ri_vis_axis((vis >> 8) & 0xFFu, dx) << 8) | (ri_vis_axis((vis >> 16) & 0xFFu, dy) << 16);
}
// final shading may take the sample's visibility as known (the emitter's alpha class is the caller's to check)
PT_HD bool ri_vis_usable(const RiShading& sh, const RiReservoir& r)
{
    if (!sh.reuse || !(r.vis & kRiVisSeen) || r.age > sh.max_age) return false;
    const uint32_t bx = (r.vis >> 8) & 0xFFu, by = (r.vis >> 16) & 0xFFu;
    if (bx == 0u || by == 0u) return false;
    const float dx = (float)((int)bx - 128), dy = (float)((int)by - 128);
    return dx * dx + dy * dy <= sh.max_dist2;
}

// ---- temporal resampling (DITemporalResampling.hlsl): the reservoir of the reprojected pixel of the previous call.  kVis (row N22):
// the selected sample's visibility word travels with it
template <bool kVis = false, typename TraceFn>
PT_HD RiReservoir ri_temporal(const RiBuffers& b, const RiScene& sc, const RiParams& p, const RiSurface& s, const RiReservoir& cur, uint32_t px,
                              uint32_t py, f3 mv, TraceFn&& trace)
{
    if (!p.temporal || !p.history_valid) return cur;
    const float fx = pt_floor((float)px + mv.x + 0.5f), fy = pt_floor((float)py + mv.y + 0.5f);
    if (!(fx >= 0.0f && fx < (float)b.w && fy >= 0.0f && fy < (float)b.h)) return cur;
    const uint32_t qi = (uint32_t)fy * b.w + (uint32_t)fx;
    const RiSurface ps = ri_surface(ri_load_record(b.prev_rec, b.prev_rec_t, qi), p.prev_cam_pos);
    if (!ps.valid) return cur;
    const float expected = s.depth + mv.z;
    if (!(pt_abs(ps.depth - expected) <= kRiDepthThreshold * expected)) return cur;
    if (!(dot(s.surf.Ns, ps.surf.Ns) >= kRiNormalThreshold)) return cur;
    RiReservoir prev = ri_load_reservoir(b.prev_res, qi);
    if (!(prev.M > 0.0f)) return cur;
    prev.M = pt_min(prev.M, (float)p.max_history * cur.M);
    uint32_t rng = rng_init(px, py, p.frame_index ^ kRiTemporalRngSalt);
    const float rnd = rng_float(rng);
    RiReservoir r = cur;
    float w_sum = cur.p_hat * cur.W * cur.M;
    const RiShade e = ri_shade(sc, s, prev.light, prev.u1, prev.u2);  // the history's sample, re-aimed from this surface
    if (ri_stream(w_sum, e.p_hat * prev.W * prev.M, rnd)) {
        r.light = prev.light; r.u1 = prev.u1; r.u2 = prev.u2; r.p_hat = e.p_hat; r.age = prev.age + 1u;
        if (kVis) r.vis = ri_vis_moved(prev.vis, (int)px - (int)fx, (int)py - (int)fy);
    }
    r.M = cur.M + prev.M;
    r.W = 0.0f;
    if (!(r.p_hat > 0.0f)) return r;
    float Z = r.M;
    if (p.temporal_bias != kRiBiasOff) {
        Z = cur.M;  // this surface holds the sample with p_hat > 0
        const RiShade ep = ri_shade(sc, ps, r.light, r.u1, r.u2);
        bool counts = ep.p_hat > 0.0f;
        if (counts && p.temporal_bias == kRiBiasRaytraced) {
            f3 so;
            float t2;
            counts = ri_visible(ps, ep, trace, so, t2);
        }
        if (counts) Z += prev.M;
    }
    r.W = w_sum / (Z * r.p_hat);
    if (!is_finite(r.W)) r.W = 0.0f;
    return r;
}

// neighbour k of the fixed table (a golden-angle spiral over the unit disc) scaled by the radius and turned by `rot` (one turn = 1),
// reflected into view as RAB_ClampSamplePositionIntoView does; false: the pixel itself
PT_HD bool ri_neighbour(const RiBuffers& b, float radius, uint32_t px, uint32_t py, uint32_t k, float rot, uint32_t& qx, uint32_t& qy)
{
    const float rr = pt_sqrt(((float)k + 0.5f) * (1.0f / (float)kRiNeighbourTable)) * radius;
    float a = pt_fma((float)k, 0.61803399f, rot);
    a = a - pt_floor(a);
    float sn, cs;
    sincos_2pi(a, sn, cs);
    int x = (int)px + (int)pt_floor(pt_fma(rr, cs, 0.5f)), y = (int)py + (int)pt_floor(pt_fma(rr, sn, 0.5f));
    const int w = (int)b.w, h = (int)b.h;
    if (x < 0) x = -x;
    if (y < 0) y = -y;
    if (x >= w) x = 2 * w - x - 1;
    if (y >= h) y = 2 * h - y - 1;
    x = x < 0 ? 0 : (x >= w ? w - 1 : x);  // (an image narrower than the radius)
    y = y < 0 ? 0 : (y >= h ? h - 1 : y);
    qx = (uint32_t)x; qy = (uint32_t)y;
    return !(qx == px && qy == py);
}

// RAB_AreMaterialsSimilar (RTXDIAppBridge.hlsli:380-385)
PT_HD bool ri_materials_similar(const Bsdf& a, const Bsdf& c)
{
    return pt_abs(a.Roughness - c.Roughness) <= 0.5f * pt_max(a.Roughness, c.Roughness)
        && pt_abs(luminance(a.F0) - luminance(c.F0)) <= 0.25f && pt_abs(luminance(a.Albedo) - luminance(c.Albedo)) <= 0.25f;
}

PT_HD bool ri_neighbour_surface(const RiBuffers& b, const RiParams& p, const RiSurface& s, uint32_t qi, RiSurface& ns)
{
    ns = ri_surface(ri_load_record(b.rec, b.rec_t, qi), p.cam_pos);
    return ns.valid && pt_abs(ns.depth - s.depth) <= kRiDepthThreshold * s.depth && dot(s.surf.Ns, ns.surf.Ns) >= kRiNormalThreshold
        && ri_materials_similar(s.bsdf, ns.bsdf);
}

// ---- spatial resampling (DISpatialResampling.hlsl): SpatialSamples neighbours of this call's temporal result.  kVis: as ri_temporal's
template <bool kVis = false, typename TraceFn>
PT_HD RiReservoir ri_spatial(const RiBuffers& b, const RiScene& sc, const RiParams& p, const RiSurface& s, const RiReservoir& centre, uint32_t px,
                             uint32_t py, TraceFn&& trace)
{
    if (!p.spatial) return centre;
    uint32_t rng = rng_init(px, py, p.frame_index ^ kRiSpatialRngSalt);
    const uint32_t start = rng_next(rng) & (kRiNeighbourTable - 1u);
    const float rot = rng_float(rng);
    RiReservoir r = centre;
    float w_sum = centre.p_hat * centre.W * centre.M;
    uint32_t accepted = 0u;
    for (uint32_t i = 0; i < p.spatial_samples; i++) {
        const float rnd = rng_float(rng);
        uint32_t qx, qy;
        if (!ri_neighbour(b, p.radius, px, py, (start + i) & (kRiNeighbourTable - 1u), rot, qx, qy)) continue;
        const uint32_t qi = qy * b.w + qx;
        RiSurface ns;
        if (!ri_neighbour_surface(b, p, s, qi, ns)) continue;
        const RiReservoir nr = ri_load_reservoir(b.res, qi);
        if (!(nr.M > 0.0f)) continue;
        accepted |= 1u << i;
        const RiShade e = ri_shade(sc, s, nr.light, nr.u1, nr.u2);
        if (ri_stream(w_sum, e.p_hat * nr.W * nr.M, rnd)) {
            r.light = nr.light; r.u1 = nr.u1; r.u2 = nr.u2; r.p_hat = e.p_hat; r.age = nr.age;
            if (kVis) r.vis = ri_vis_moved(nr.vis, (int)px - (int)qx, (int)py - (int)qy);
        }
        r.M += nr.M;
    }
    if (!accepted) return centre;
    r.W = 0.0f;
    if (!(r.p_hat > 0.0f)) return r;
    float Z = r.M;
    if (p.spatial_bias != kRiBiasOff) {
        Z = centre.M;
        for (uint32_t i = 0; i < p.spatial_samples; i++) {
            if (!(accepted & (1u << i))) continue;
            uint32_t qx, qy;
            (void)ri_neighbour(b, p.radius, px, py, (start + i) & (kRiNeighbourTable - 1u), rot, qx, qy);
            const uint32_t qi = qy * b.w + qx;
            const RiSurface ns = ri_surface(ri_load_record(b.rec, b.rec_t, qi), p.cam_pos);
            const RiShade en = ri_shade(sc, ns, r.light, r.u1, r.u2);
            bool counts = en.p_hat > 0.0f;
            if (counts && p.spatial_bias == kRiBiasRaytraced) {
                f3 so;
                float t2;
                counts = ri_visible(ns, en, trace, so, t2);
            }
            if (counts) Z += b.res[1][qi].x;
        }
    }
    r.W = w_sum / (Z * r.p_hat);
    if (!is_finite(r.W)) r.W = 0.0f;
    return r;
}

// ---- row N22 (spec S26, part 2): pairwise MIS, bias mode 2.  The canonical reservoir (M_c, sample y_c, on surface c) against k
// accepted neighbours (M_i, y_i, on surface i), p_x(y) the target function of y re-aimed from x (no visibility):
//   neighbour i streams with  p_c(y_i) W_i m_i / k,   m_i = M_i p_i(y_i) / (M_i p_i(y_i) + (M_c / k) p_c(y_i))       (0 where that sum is not > 0)
//   the canonical streams last with  p_c(y_c) W_c m_c,   m_c = (1 / k) sum_i (M_c / k) p_c(y_c) / (M_i p_i(y_c) + (M_c / k) p_c(y_c))   (a term counts 1 there)
//   W = w_sum / p_c(y_selected), M = M_c + sum_i M_i.  The k + 1 weights sum to 1 at every y.
// p_i(y_i) and p_c(y_c) are the p_hat the reservoirs store.  Every product and sum is one float32 operation in the order written in
// ri_pairwise_neighbour / ri_pairwise_canonical_term (DESIGN.md spec S26 freezes it).
struct RiPairwise {
    float kf, mc;      // k and M_c / k
    float w_sum, m_c;  // the stream's weight so far; the canonical's terms so far
};

PT_HD RiPairwise ri_pairwise_begin(float M_c, uint32_t k)
{
    RiPairwise s;
    s.kf = (float)k;
    s.mc = M_c / s.kf;
    s.w_sum = 0.0f;
    s.m_c = 0.0f;
    return s;
}
// the weight neighbour i's sample streams with: pc_yi = p_c(y_i), pi_yi = p_i(y_i)
PT_HD float ri_pairwise_neighbour(const RiPairwise& s, float M_i, float W_i, float pi_yi, float pc_yi)
{
    const float a = M_i * pi_yi, b = s.mc * pc_yi, d = a + b;
    const float m = d > 0.0f ? a / d : 0.0f;
    return ((pc_yi * W_i) * m) / s.kf;
}
// pair i's term of the canonical weight: pc_yc = p_c(y_c), pi_yc = p_i(y_c)
PT_HD float ri_pairwise_canonical_term(const RiPairwise& s, float M_i, float pc_yc, float pi_yc)
{
    const float c = s.mc * pc_yc, d = M_i * pi_yc + c;
    return d > 0.0f ? c / d : 1.0f;
}
// the canonical sample streams last; `centre` is restored where it wins; then W of whatever was selected
PT_HD void ri_pairwise_end(RiPairwise& s, const RiReservoir& centre, float rnd, RiReservoir& r)
{
    const float w_c = (centre.p_hat * centre.W) * (s.m_c / s.kf);
    if (ri_stream(s.w_sum, w_c, rnd)) { r.light = centre.light; r.u1 = centre.u1; r.u2 = centre.u2; r.p_hat = centre.p_hat; r.age = centre.age; r.vis = centre.vis; }
    r.W = r.p_hat > 0.0f ? s.w_sum / r.p_hat : 0.0f;
    if (!is_finite(r.W)) r.W = 0.0f;
}

// ri_temporal under pairwise MIS: k = 1, the neighbour is the reprojected history reservoir (M capped as there) on the previous call's
// surface seen from prev_cam_pos.  Draws ri_temporal's rnd, then one more for the canonical sample.  The visibility word travels.
PT_HD RiReservoir ri_temporal_pairwise(const RiBuffers& b, const RiScene& sc, const RiParams& p, const RiSurface& s, const RiReservoir& cur, uint32_t px,
                                       uint32_t py, f3 mv)
{
    if (!p.temporal || !p.history_valid) return cur;
    const float fx = pt_floor((float)px + mv.x + 0.5f), fy = pt_floor((float)py + mv.y + 0.5f);
    if (!(fx >= 0.0f && fx < (float)b.w && fy >= 0.0f && fy < (float)b.h)) return cur;
    const uint32_t qi = (uint32_t)fy * b.w + (uint32_t)fx;
    const RiSurface ps = ri_surface(ri_load_record(b.prev_rec, b.prev_rec_t, qi), p.prev_cam_pos);
    if (!ps.valid) return cur;
    const float expected = s.depth + mv.z;
    if (!(pt_abs(ps.depth - expected) <= kRiDepthThreshold * expected)) return cur;
    if (!(dot(s.surf.Ns, ps.surf.Ns) >= kRiNormalThreshold)) return cur;
    RiReservoir prev = ri_load_reservoir(b.prev_res, qi);
    if (!(prev.M > 0.0f)) return cur;
    prev.M = pt_min(prev.M, (float)p.max_history * cur.M);
    uint32_t rng = rng_init(px, py, p.frame_index ^ kRiTemporalRngSalt);
    const float rnd = rng_float(rng);
    RiReservoir r = cur;
    RiPairwise pw = ri_pairwise_begin(cur.M, 1u);
    const RiShade e = ri_shade(sc, s, prev.light, prev.u1, prev.u2);  // the history's sample, re-aimed from this surface
    if (ri_stream(pw.w_sum, ri_pairwise_neighbour(pw, prev.M, prev.W, prev.p_hat, e.p_hat), rnd)) {
        r.light = prev.light; r.u1 = prev.u1; r.u2 = prev.u2; r.p_hat = e.p_hat; r.age = prev.age + 1u;
        r.vis = ri_vis_moved(prev.vis, (int)px - (int)fx, (int)py - (int)fy);
    }
    pw.m_c += ri_pairwise_canonical_term(pw, prev.M, cur.p_hat, ri_shade(sc, ps, cur.light, cur.u1, cur.u2).p_hat);
    ri_pairwise_end(pw, cur, rng_float(rng), r);
    r.M = cur.M + prev.M;
    return r;
}

// ri_spatial under pairwise MIS.  Every neighbour's weight depends on k, the number of accepted neighbours, so the acceptance tests run
// first (records only: no sample is shaded); the second loop shades p_c(y_i) and p_i(y_c) while neighbour i's record is in registers,
// which replaces both loops of the Basic form.  Draws ri_spatial's numbers, then one more for the canonical sample.
PT_HD RiReservoir ri_spatial_pairwise(const RiBuffers& b, const RiScene& sc, const RiParams& p, const RiSurface& s, const RiReservoir& centre, uint32_t px,
                                      uint32_t py)
{
    if (!p.spatial) return centre;
    uint32_t rng = rng_init(px, py, p.frame_index ^ kRiSpatialRngSalt);
    const uint32_t start = rng_next(rng) & (kRiNeighbourTable - 1u);
    const float rot = rng_float(rng);
    uint32_t accepted = 0u, k = 0u;
    for (uint32_t i = 0; i < p.spatial_samples; i++) {
        uint32_t qx, qy;
        if (!ri_neighbour(b, p.radius, px, py, (start + i) & (kRiNeighbourTable - 1u), rot, qx, qy)) continue;
        const uint32_t qi = qy * b.w + qx;
        RiSurface ns;
        if (!ri_neighbour_surface(b, p, s, qi, ns)) continue;
        if (!(b.res[1][qi].x > 0.0f)) continue;
        accepted |= 1u << i;
        k++;
    }
    if (!accepted) return centre;
    RiReservoir r = centre;
    RiPairwise pw = ri_pairwise_begin(centre.M, k);
    for (uint32_t i = 0; i < p.spatial_samples; i++) {
        const float rnd = rng_float(rng);
        if (!(accepted & (1u << i))) continue;
        uint32_t qx, qy;
        (void)ri_neighbour(b, p.radius, px, py, (start + i) & (kRiNeighbourTable - 1u), rot, qx, qy);
        const uint32_t qi = qy * b.w + qx;
        const RiSurface ns = ri_surface(ri_load_record(b.rec, b.rec_t, qi), p.cam_pos);
        const RiReservoir nr = ri_load_reservoir(b.res, qi);
        const RiShade e = ri_shade(sc, s, nr.light, nr.u1, nr.u2);
        if (ri_stream(pw.w_sum, ri_pairwise_neighbour(pw, nr.M, nr.W, nr.p_hat, e.p_hat), rnd)) {
            r.light = nr.light; r.u1 = nr.u1; r.u2 = nr.u2; r.p_hat = e.p_hat; r.age = nr.age;
            r.vis = ri_vis_moved(nr.vis, (int)px - (int)qx, (int)py - (int)qy);
        }
        pw.m_c += ri_pairwise_canonical_term(pw, nr.M, centre.p_hat, ri_shade(sc, ns, centre.light, centre.u1, centre.u2).p_hat);
        r.M += nr.M;
    }
    ri_pairwise_end(pw, centre, rng_float(rng), r);
    return r;
}

// ---- final shading (DIFinalShading.hlsl:23-103, IsLastRenderPass false): false = the pixel is not written
template <typename TraceFn, typename EmitFn>
PT_HD bool ri_final(const RiScene& sc, const RiSurface& s, const RiReservoir& r, TraceFn&& trace, EmitFn&& emit, float4& diffuse, float4& specular)
{
    if (!(r.W > 0.0f) || !is_finite(r.W)) return false;
    const RiShade e = ri_shade(sc, s, r.light, r.u1, r.u2);
    if (!(e.p_hat > 0.0f)) return false;
    f3 so;
    float t2;
    if (!ri_visible(s, e, trace, so, t2)) return false;
    const f3 le = emit(e.sphere, so, e.L, t2);  // at the point reached: an emissive map modulates it, as in di_estimate
    const float k = e.inv_pdf * r.W;
    const f3 d = (le * e.f_d) * k, sp = (le * e.f_s) * k, sum = d + sp;
    if (sum.x == 0.0f && sum.y == 0.0f && sum.z == 0.0f) return false;
    if (!is_finite(sum.x) || !is_finite(sum.y) || !is_finite(sum.z)) return false;
    diffuse = ri_float4(d.x, d.y, d.z, t2);
    specular = ri_float4(sp.x, sp.y, sp.z, t2);
    return true;
}

// ri_final with reuseFinalVisibility (DIFinalShading.hlsl:32-56; spec S26, part 1): a sample whose word says it was seen, young and
// near enough, on an emitter whose every crossing counts, casts no ray -- the light distance is intersect_sphere's from the spawn
// origin, the leaf function every tree walk calls, so the pixel holds the bits a traced one would.  Where that intersection fails (a
// limb sample) the ray is cast.  The reservoir is never changed.
template <typename TraceFn, typename EmitFn>
PT_HD bool ri_final_reuse(const RiScene& sc, const RiShading& sh, const RiSurface& s, const RiReservoir& r, TraceFn&& trace, EmitFn&& emit, float4& diffuse,
                          float4& specular)
{
    const uint32_t sphere = sc.lights[r.light < sc.n_lights ? r.light : sc.n_lights - 1u];
    const bool known = ri_vis_usable(sh, r) && !(sc.alpha_class && sc.alpha_class[sphere] != 0u);
    auto query = [&](f3 o, f3 d, float& t, uint32_t& id) {
        if (known) {
            const float4 ls = sc.sph[sphere];
            if (intersect_sphere(o, d, 0.0f, kInf, make_f3(ls.x, ls.y, ls.z), ls.w, t)) { id = sphere; return; }
        }
        trace(o, d, t, id);
    };
    return ri_final(sc, s, r, query, emit, diffuse, specular);
}

// ---- what one lane of each launch does
// launch 1: the pixel's surface record from the G-buffer, initial sampling, temporal resampling -> this call's slot
template <uint32_t kMode = kLrUniform, typename TraceFn>
PT_HD void ri_pass1_px(const RiBuffers& b, const RiScene& sc, const RiParams& p, uint32_t px, uint32_t py, TraceFn&& trace)
{
    const uint32_t i = py * b.w + px;
    const RiRecord rec = ri_record_from_gbuffer(b, i);
    if (!is_finite(rec.r3.z)) {
        // no surface: the plane that says so is all any reader looks at (ri_load_record; a reservoir is only read behind a valid
        // record), 16 B written instead of 100 -- most pixels of a frame with sky or mirror-like ground
        b.rec[3][i] = rec.r3;
        return;
    }
    ri_store_record(b.rec, b.rec_t, i, rec);
    const RiSurface s = ri_surface(rec, p.cam_pos);
    RiReservoir r = ri_initial<kMode>(sc, p, s, px, py, trace);
    const f3 mv = make_f3(b.motion_vector[3u * i], b.motion_vector[3u * i + 1u], b.motion_vector[3u * i + 2u]);
    r = ri_temporal(b, sc, p, s, r, px, py, mv, trace);
    ri_store_reservoir(b.res, i, r);
}

// launch 1 of pt_restir_di_ex (row N17): as ri_pass1_px up to the store of the reservoir, which the caller does behind the boiling
// filter; false: no surface (nothing but the record's validity plane is written, r is empty).  kBrdf: initial sampling is ri_initial_mis.
template <uint32_t kMode, bool kBrdf, typename TraceFn>
PT_HD bool ri_pass1_reservoir(const RiBuffers& b, const RiScene& sc, const RiParamsEx& p, uint32_t px, uint32_t py, TraceFn&& trace, RiReservoir& r)
{
    const uint32_t i = py * b.w + px;
    r = ri_empty_reservoir();
    const RiRecord rec = ri_record_from_gbuffer(b, i);
    if (!is_finite(rec.r3.z)) {
        b.rec[3][i] = rec.r3;
        return false;
    }
    ri_store_record(b.rec, b.rec_t, i, rec);
    const RiSurface s = ri_surface(rec, p.cam_pos);
    if (kBrdf) r = ri_initial_mis<kMode>(sc, p, s, px, py, trace);
    else r = ri_initial<kMode>(sc, p, s, px, py, trace);
    const f3 mv = make_f3(b.motion_vector[3u * i], b.motion_vector[3u * i + 1u], b.motion_vector[3u * i + 2u]);
    r = ri_temporal(b, sc, p, s, r, px, py, mv, trace);
    return true;
}

// ... and the host form of one 8x8 block of it, (bx, by) in blocks: the 64 lanes in row-major order, the filter, the stores
template <uint32_t kMode, bool kBrdf, typename TraceFn>
inline void ri_pass1_block(const RiBuffers& b, const RiScene& sc, const RiParamsEx& p, uint32_t bx, uint32_t by, TraceFn&& trace)
{
    RiReservoir res[64];
    bool has[64];
    float w[64];
    for (uint32_t l = 0; l < 64u; l++) {
        const uint32_t px = bx * 8u + (l & 7u), py = by * 8u + (l >> 3);
        has[l] = px < b.w && py < b.h && ri_pass1_reservoir<kMode, kBrdf>(b, sc, p, px, py, trace, res[l]);
        w[l] = has[l] ? res[l].W : 0.0f;
    }
    uint32_t n = 0u;
    const float sum = p.boiling_filter ? ri_boiling_sum64(w, n) : 0.0f;
    const float mult = ri_boiling_multiplier(p.boiling_strength);
    for (uint32_t l = 0; l < 64u; l++) {
        if (!has[l]) continue;
        if (p.boiling_filter && ri_boiled(w[l], sum, n, mult)) res[l] = ri_empty_reservoir();
        ri_store_reservoir(b.res, (by * 8u + (l >> 3)) * b.w + bx * 8u + (l & 7u), res[l]);
    }
}

// launch 2: spatial resampling over launch 1's results, final shading
template <typename TraceFn, typename EmitFn>
PT_HD void ri_pass2_px(const RiBuffers& b, const RiScene& sc, const RiParams& p, uint32_t px, uint32_t py, TraceFn&& trace, EmitFn&& emit)
{
    const uint32_t i = py * b.w + px;
    const RiRecord rec = ri_load_record(b.rec, b.rec_t, i);
    if (!is_finite(rec.r3.z)) return;
    const RiSurface s = ri_surface(rec, p.cam_pos);
    const RiReservoir r = ri_spatial(b, sc, p, s, ri_load_reservoir(b.res, i), px, py, trace);
    float4 d, sp;
    if (ri_final(sc, s, r, trace, emit, d, sp)) { b.out_diffuse[i] = d; b.out_specular[i] = sp; }
}

// ---- the launches of pt_restir_di_full (row N22)
// launch 1: as ri_pass1_reservoir, and a sample whose initial visibility ray reached its emitter says so in its word (W > 0 behind
// ri_initial / ri_initial_mis means exactly that); kPairwise: temporal resampling under bias mode 2
template <uint32_t kMode, bool kBrdf, bool kPairwise, typename TraceFn>
PT_HD bool ri_pass1_full_reservoir(const RiBuffers& b, const RiScene& sc, const RiParamsFull& p, uint32_t px, uint32_t py, TraceFn&& trace, RiReservoir& r)
{
    const uint32_t i = py * b.w + px;
    r = ri_empty_reservoir();
    const RiRecord rec = ri_record_from_gbuffer(b, i);
    if (!is_finite(rec.r3.z)) {
        b.rec[3][i] = rec.r3;
        return false;
    }
    ri_store_record(b.rec, b.rec_t, i, rec);
    const RiSurface s = ri_surface(rec, p.cam_pos);
    if (kBrdf) r = ri_initial_mis<kMode>(sc, p, s, px, py, trace);
    else r = ri_initial<kMode>(sc, p, s, px, py, trace);
    if (r.W > 0.0f) r.vis = kRiVisFresh;
    const f3 mv = make_f3(b.motion_vector[3u * i], b.motion_vector[3u * i + 1u], b.motion_vector[3u * i + 2u]);
    if (kPairwise) r = ri_temporal_pairwise(b, sc, p, s, r, px, py, mv);
    else r = ri_temporal<true>(b, sc, p, s, r, px, py, mv, trace);
    return true;
}

// ... and the host form of one 8x8 block of it, as ri_pass1_block
template <uint32_t kMode, bool kBrdf, bool kPairwise, typename TraceFn>
inline void ri_pass1_full_block(const RiBuffers& b, const RiScene& sc, const RiParamsFull& p, uint32_t bx, uint32_t by, TraceFn&& trace)
{
    RiReservoir res[64];
    bool has[64];
    float w[64];
    for (uint32_t l = 0; l < 64u; l++) {
        const uint32_t px = bx * 8u + (l & 7u), py = by * 8u + (l >> 3);
        has[l] = px < b.w && py < b.h && ri_pass1_full_reservoir<kMode, kBrdf, kPairwise>(b, sc, p, px, py, trace, res[l]);
        w[l] = has[l] ? res[l].W : 0.0f;
    }
    uint32_t n = 0u;
    const float sum = p.boiling_filter ? ri_boiling_sum64(w, n) : 0.0f;
    const float mult = ri_boiling_multiplier(p.boiling_strength);
    for (uint32_t l = 0; l < 64u; l++) {
        if (!has[l]) continue;
        if (p.boiling_filter && ri_boiled(w[l], sum, n, mult)) res[l] = ri_empty_reservoir();
        ri_store_reservoir(b.res, (by * 8u + (l >> 3)) * b.w + bx * 8u + (l & 7u), res[l]);
    }
}

// launch 2: kPairwise -- spatial resampling under bias mode 2; kReuse -- final shading through ri_final_reuse (the spatial pass then
// carries the word).  Read-only on the slot, like ri_pass2_px.
template <bool kPairwise, bool kReuse, typename TraceFn, typename EmitFn>
PT_HD void ri_pass2_full_px(const RiBuffers& b, const RiScene& sc, const RiParamsFull& p, uint32_t px, uint32_t py, TraceFn&& trace, EmitFn&& emit)
{
    const uint32_t i = py * b.w + px;
    const RiRecord rec = ri_load_record(b.rec, b.rec_t, i);
    if (!is_finite(rec.r3.z)) return;
    const RiSurface s = ri_surface(rec, p.cam_pos);
    const RiReservoir centre = ri_load_reservoir(b.res, i);
    const RiReservoir r = kPairwise ? ri_spatial_pairwise(b, sc, p, s, centre, px, py) : ri_spatial<kReuse>(b, sc, p, s, centre, px, py, trace);
    float4 d, sp;
    if (kReuse ? ri_final_reuse(sc, p.sh, s, r, trace, emit, d, sp) : ri_final(sc, s, r, trace, emit, d, sp)) { b.out_diffuse[i] = d; b.out_specular[i] = sp; }
}

#if defined(__HIPCC__)
struct SceneView;
struct PixelMap;
// pass 0: launch 1 (initial + temporal), pass 1: launch 2 (spatial + final), over the pixels of pm (mode 0, the whole RenderSize);
// mode, lr: the source of launch 1's candidates (kLrUniform: lr is not read)
hipError_t launch_restir_pass(int pass, const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParams& p, uint32_t mode, const LrView& lr,
                              uint32_t grid, hipStream_t stream);
// what launch 1 of pt_restir_di_ex reads besides (row N17): the emitter index of every sphere, S22's pyramid (null in Uniform mode)
struct RiExtra {
    const uint32_t* light_of;
    const float* pyramid;
    uint32_t pyramid_levels;
};
// launch 1 with p.brdf_samples > 0 and / or p.boiling_filter (both off: launch_restir_pass)
hipError_t launch_restir_pass1_ex(const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsEx& p, uint32_t mode, const LrView& lr,
                                  const RiExtra& x, uint32_t grid, hipStream_t stream);
// the launches of pt_restir_di_full (row N22, pt_restir_full.hip).  pass 0: launch 1 writing the visibility word, temporal resampling
// pairwise where p.temporal_bias is 2; pass 1: launch 2 with the spatial pass pairwise where p.spatial_bias is 2 and final shading
// through the word where p.sh.reuse.  The caller sends a call that needs neither to the launches above.
hipError_t launch_restir_full(int pass, const SceneView& sv, const PixelMap& pm, const RiBuffers& b, const RiParamsFull& p, uint32_t mode, const LrView& lr,
                              const RiExtra& x, uint32_t grid, hipStream_t stream);
#endif

}  // namespace pt
