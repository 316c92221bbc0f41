// gbframe_host.h -- TEST SHIM: what gbframe_host.cpp (the library the tests load), gbframe_sanitize.cpp (the stand-alone sanitizer program)
// and gbframe_leaf_gpu.hip (the leaf functions compiled for gfx950) run csrc/pt_pixfmt.h and csrc/pt_gbframe.h with (row N27, spec S30),
// over sharc_host.h's scene (brute-force closest hit, which the device walkers equal bit for bit).  Not part of the product.
#pragma once

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_gbframe.h"

namespace gbfhost {

// The leaf functions over 32-bit words: encoders take a float's bits and return the code, decoders take the code and return the float's bits
enum : uint32_t { kLeafHalfEncode = 0, kLeafHalfDecode, kLeafUnorm8Encode, kLeafUnorm8Decode, kLeafSnorm16Encode, kLeafSnorm16Decode, kLeafCount };

PT_HD uint32_t leaf(uint32_t op, uint32_t x)
{
    switch (op) {
    case kLeafHalfEncode: return pt::half_encode(pt::as_float(x));
    case kLeafHalfDecode: return pt::as_uint(pt::half_decode(x & 0xFFFFu));
    case kLeafUnorm8Encode: return pt::unorm8_encode(pt::as_float(x));
    case kLeafUnorm8Decode: return pt::as_uint(pt::unorm8_decode(x & 0xFFu));
    case kLeafSnorm16Encode: return pt::snorm16_encode(pt::as_float(x));
    default: return pt::as_uint(pt::snorm16_decode(x & 0xFFFFu));
    }
}

}  // namespace gbfhost

#if !defined(__HIPCC__)
#include "sharc_host.h"

namespace gbfhost {

using namespace pt;

constexpr uint32_t kFloatsPerPixel = 32;  // one float per channel component, in PtGBuffer's order (gbuffer_host.cpp)

// SceneData's environment map as the kernels' environment functor reads it (lens_host.h)
struct HostEnvMap {
    uint32_t tex = kNoTexture, cube = 0;
    float xf[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
};

inline void pixel_floats(const GBufferPixel& g, float* o)
{
    const float v[kFloatsPerPixel] = { g.Position.x, g.Position.y, g.Position.z, g.Position.w, g.FlatNormal.x, g.FlatNormal.y,
                                       g.GeometricNormal.x, g.GeometricNormal.y, g.LinearDepth, g.NormalizedDepth,
                                       g.MotionVector.x, g.MotionVector.y, g.MotionVector.z,
                                       g.BaseColorMetalness.x, g.BaseColorMetalness.y, g.BaseColorMetalness.z, g.BaseColorMetalness.w,
                                       g.DiffuseAlbedo.x, g.DiffuseAlbedo.y, g.DiffuseAlbedo.z, g.SpecularAlbedo.x, g.SpecularAlbedo.y, g.SpecularAlbedo.z,
                                       g.NormalRoughness.x, g.NormalRoughness.y, g.NormalRoughness.z, g.NormalRoughness.w, g.IOR, g.Transmission,
                                       g.Radiance.x, g.Radiance.y, g.Radiance.z };
    std::memcpy(o, v, sizeof v);
}

inline GBufferPixel pixel_of_floats(const float* v, uint32_t mask)
{
    GBufferPixel g{};
    g.Position = gb_float4(v[0], v[1], v[2], v[3]);
    g.FlatNormal.x = v[4]; g.FlatNormal.y = v[5]; g.GeometricNormal.x = v[6]; g.GeometricNormal.y = v[7];
    g.LinearDepth = v[8]; g.NormalizedDepth = v[9];
    g.MotionVector = make_f3(v[10], v[11], v[12]);
    g.BaseColorMetalness = gb_float4(v[13], v[14], v[15], v[16]);
    g.DiffuseAlbedo = make_f3(v[17], v[18], v[19]); g.SpecularAlbedo = make_f3(v[20], v[21], v[22]);
    g.NormalRoughness = gb_float4(v[23], v[24], v[25], v[26]);
    g.IOR = v[27]; g.Transmission = v[28];
    g.Radiance = make_f3(v[29], v[30], v[31]);
    g.mask = mask;
    return g;
}

// pt_gbuffer_packed.hip's stores for texel i: a channel is written where its pointer is given and the pixel's mask has its bit
inline void store_packed(const GBufferPixel& g, void* const out[13], size_t i)
{
    auto on = [&](uint32_t k) { return out[k] && (g.mask & (1u << k)); };
    if (on(0)) static_cast<float4*>(out[0])[i] = g.Position;
    if (on(1)) static_cast<uint32_t*>(out[1])[i] = gbp_pack_normal(g.FlatNormal);
    if (on(2)) static_cast<uint32_t*>(out[2])[i] = gbp_pack_normal(g.GeometricNormal);
    if (on(3)) static_cast<float*>(out[3])[i] = g.LinearDepth;
    if (on(4)) static_cast<float*>(out[4])[i] = g.NormalizedDepth;
    if (on(5)) static_cast<uint64_t*>(out[5])[i] = gbp_pack_motion(g.MotionVector);
    if (on(6)) static_cast<uint32_t*>(out[6])[i] = gbp_pack_base_color_metalness(g.BaseColorMetalness);
    if (on(7)) static_cast<uint64_t*>(out[7])[i] = gbp_pack_albedo(g.DiffuseAlbedo);
    if (on(8)) static_cast<uint64_t*>(out[8])[i] = gbp_pack_albedo(g.SpecularAlbedo);
    if (on(9)) static_cast<uint64_t*>(out[9])[i] = gbp_pack_normal_roughness(g.NormalRoughness);
    if (on(10)) static_cast<uint16_t*>(out[10])[i] = gbp_pack_ior(g.IOR);
    if (on(11)) static_cast<uint8_t*>(out[11])[i] = gbp_pack_transmission(g.Transmission);
    if (on(12)) static_cast<uint64_t*>(out[12])[i] = gbp_pack_radiance(g.Radiance);
}

// pt_render_gbuffer*'s GBufferFrame / GBufferScene over a HostScene (gbuffer_pass in pt_api_side.hip)
inline GBufferFrame gbuffer_frame_of(const PtCamera* cam, uint32_t w, uint32_t h)
{
    GBufferFrame fr{};
    fr.cam = camera_params(*cam, w, h);
    fr.width = (float)w;
    fr.height = (float)h;
    fr.reversed = cam->IsNormalizedDepthReversed ? 1u : 0u;
    std::memcpy(fr.world_to_projection, cam->Matrices[5], sizeof fr.world_to_projection);
    std::memcpy(fr.prev_world_to_projection, cam->Matrices[2], sizeof fr.prev_world_to_projection);
    std::memcpy(fr.prev_world_to_view, cam->Matrices[0], sizeof fr.prev_world_to_view);
    return fr;
}

// One G-buffer call over rect = {x, y, w, h}: per pixel of the rect the 32 floats and the mask of gbuffer_pixel (f32 / mask, may be null),
// the hit (t / id, may be null) and the packed stores (packed: 13 pointers, null = not requested; may itself be null).
// prev_sph / prev_rot: n float4 each, null = not given.
inline void run_gbuffer(const shhost::HostScene& hs, const HostEnvMap& em, bool is_static, const PtCamera* cam, uint32_t w, uint32_t h, const uint32_t* rect, const float4* prev_sph,
                        const float4* prev_rot, bool has_rot, uint32_t want, float* f32, uint32_t* mask, float* t_out, uint32_t* id_out, void* const* packed)
{
    const GBufferFrame fr = gbuffer_frame_of(cam, w, h);
    GBufferScene sc{};
    sc.sph = hs.sph.data(); sc.mats = hs.mats.data();
    sc.tex = hs.tex ? hs.views.data() : nullptr;
    sc.tex_maps = hs.tex ? hs.tex_maps.data() : nullptr;
    sc.rot = has_rot ? hs.rots.data() : nullptr;
    sc.is_static = is_static ? 1u : 0u;
    sc.prev_sph = is_static ? nullptr : prev_sph;
    sc.prev_rot = is_static ? nullptr : prev_rot;
    sc.env_tex = em.tex; sc.env_cube = em.cube;
    for (int k = 0; k < 4; k++) sc.env[k] = hs.env[k];
    for (int k = 0; k < 9; k++) sc.env_xf[k] = em.xf[k];
    for (uint32_t y = 0; y < rect[3]; y++)
        for (uint32_t x = 0; x < rect[2]; x++) {
            const uint32_t px = rect[0] + x, py = rect[1] + y;
            f3 o, d;
            float tmin, tmax, t;
            uint32_t id;
            primary_ray(fr.cam, px, py, o, d, tmin, tmax);
            hs.trace(o, d, tmin, tmax, t, id);
            const GBufferPixel g = hs.tex ? gbuffer_pixel<true>(fr, sc, px, py, t, id, want) : gbuffer_pixel<false>(fr, sc, px, py, t, id, want);
            const size_t i = (size_t)y * rect[2] + x;
            if (f32) pixel_floats(g, f32 + kFloatsPerPixel * i);
            if (mask) mask[i] = g.mask;
            if (t_out) t_out[i] = t;
            if (id_out) id_out[i] = id;
            if (packed) store_packed(g, packed, i);
        }
}

// prm = {RenderSize w, h, FrameIndex, Bounces, SamplesPerPixel, IsRussianRouletteEnabled, rect x, y, w, h}
inline GbFrame frame_of(const PtCamera* cam, const uint32_t* prm, float throughput_threshold)
{
    return gb_frame(*cam, prm[0], prm[1], prm[2], prm[3], prm[4], prm[5] != 0u, throughput_threshold);
}

// One pt_render_from_gbuffer call: out = rect.w * rect.h float4; returns the rays traced.  pixel_rays (may be null): the rays of each pixel.
inline uint64_t run_frame(const shhost::HostScene& hs, const HostEnvMap& em, const GbFrame& fr, const GbInput& in, const uint32_t* rect, float* out, uint32_t* pixel_rays)
{
    auto trace = [&](f3 o, f3 d, float tmin, float tmax, float& t, uint32_t& id) { hs.trace(o, d, tmin, tmax, t, id); };
    auto material = [&](uint32_t id, f3 o, f3 d, float t, bool primary) { return hs.material(id, o, d, t, primary); };
    auto env = [&](f3 d) {  // gbframe_kernel's functor: the map only in a textured scene
        if (hs.tex && em.tex != kNoTexture) return em.cube ? environment_cube(hs.views.data() + em.tex, em.xf, d) : environment_texture(hs.views[em.tex], em.xf, d);
        return hs.environment(d);
    };
    uint64_t total = 0;
    for (uint32_t y = 0; y < rect[3]; y++)
        for (uint32_t x = 0; x < rect[2]; x++) {
            uint32_t rays = 0;
            const size_t k = (size_t)y * rect[2] + x;
            const f3 c = gbframe_pixel(fr, in, rect[0] + x, rect[1] + y, k, trace, material, env, rays);
            out[4u * k] = c.x; out[4u * k + 1u] = c.y; out[4u * k + 2u] = c.z; out[4u * k + 3u] = 1.0f;
            if (pixel_rays) pixel_rays[k] = rays;
            total += rays;
        }
    return total;
}

}  // namespace gbfhost
#endif
