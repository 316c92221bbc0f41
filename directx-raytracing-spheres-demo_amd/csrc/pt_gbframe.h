// pt_gbframe.h -- the frame whose primary surface is a G-buffer texel and not a traced ray (row N27, pt_render_from_gbuffer, DESIGN.md spec
// S30): the reference's DEFAULT permutation with Denoiser::None as Shaders/Raytracing.hlsl:103-386 runs it -- the raygen shader loads the
// textures GBufferGeneration wrote (:118-148) as the first vertex of EVERY sample and only traces from the first bounce on.
// Everything compiles on the device (pt_gbframe.hip) and as host C++ (the bit-parity tests):
//   gbf_primary_vertex  the first vertex from the eight channels the shader loads, float32 (Format 0) or packed (Format 1, pt_pixfmt.h)
//   gbframe_pixel       one pixel of the frame: pt_lens.h's lens_pixel without a camera ray, its draw order, breaks, Russian roulette and
//                       throughput cut-off kept; the optional DI of pt_render_with_di added after the mean (:302, :382)
// The functors are those of pt_lens.h: trace(o, d, tmin, tmax, t, id), material(id, o, d, t, primary) -> HitMaterial, env(d).
#pragma once

#include "pt_pixfmt.h"
#include "pt_restir.h"  // decode_unit_vector, the inverse of pt_gbuffer.h's encode_unit_vector

namespace pt {

enum : uint32_t { kGbFormatFloat32 = 0u, kGbFormatPacked = 1u };

struct GbFrame {
    CameraParams cam;
    uint32_t frame_index, bounces, spp, rr_enabled;
    float throughput_threshold, inv_spp;
};

PT_HD GbFrame gb_frame(const PtCamera& c, uint32_t w, uint32_t h, uint32_t frame_index, uint32_t bounces, uint32_t spp, bool rr_enabled, float throughput_threshold)
{
    GbFrame fr;
    fr.cam = camera_params(c, w, h);
    fr.frame_index = frame_index; fr.bounces = bounces; fr.spp = spp; fr.rr_enabled = rr_enabled ? 1u : 0u;
    fr.throughput_threshold = throughput_threshold;
    fr.inv_spp = 1.0f / (float)spp;
    return fr;
}

// The channels Raytracing.hlsl:118-148 loads, one texel per pixel of the rect, row-major; the layouts are PtGBuffer's (format 0) or
// PtGBufferPacked's (format 1).  Position is a float4 in both.  di_diffuse null: no DI.
struct GbInput {
    uint32_t format;
    const float4* Position;
    const void *FlatNormal, *GeometricNormal, *BaseColorMetalness, *NormalRoughness, *IOR, *Transmission, *Radiance;
    const float4 *di_diffuse, *di_specular;
};

// A vertex of the path as the loop below needs it: N the flat normal (spawn side and offset, GetSafeWorldRayOrigin), Ng the geometric one
struct GbVertex {
    f3 P, N, Ng, Ns, emission;
    float offset;
    bool front;
    Bsdf bsdf;
};

PT_HD f3 gbf_load_radiance(const GbInput& in, size_t i)
{
    if (in.format == kGbFormatPacked) return gbp_unpack_radiance(static_cast<const uint64_t*>(in.Radiance)[i]);
    return static_cast<const f3*>(in.Radiance)[i];
}

PT_HD f3 gbf_load_normal(uint32_t format, const void* p, size_t i)
{
    f2 e;
    if (format == kGbFormatPacked) e = gbp_unpack_normal(static_cast<const uint32_t*>(p)[i]);
    else { const float* q = static_cast<const float*>(p) + 2u * i; e.x = q[0]; e.y = q[1]; }
    return decode_unit_vector(e.x, e.y);
}

// DI = Diffuse.rgb + Specular.rgb of one texel and the reference's isDIValid = any(DI > 0): the arithmetic of pt_sharc.h's sh_load_di
PT_HD bool gbf_load_di(const GbInput& in, size_t i, f3& DI)
{
    const float4 a = in.di_diffuse[i], b = in.di_specular[i];
    DI = load3(a) + load3(b);
    return DI.x > 0.0f || DI.y > 0.0f || DI.z > 0.0f;
}

// The first vertex of a hit pixel (pos = its Position texel, d = the primary ray's direction).  Ns is taken as stored: not flipped to
// the ray's side again and not renormalised.  Transmission is read only where the stored Metalness is below 1: the G-buffer pass writes
// it only where Metallic < 1, and a stored Metalness below 1 implies that (unorm8_encode gives 255 from 1 up).
PT_HD GbVertex gbf_primary_vertex(const GbInput& in, size_t i, float4 pos, f3 d)
{
    GbVertex v;
    v.P = load3(pos);
    v.offset = pos.w;
    v.N = gbf_load_normal(in.format, in.FlatNormal, i);
    v.Ng = gbf_load_normal(in.format, in.GeometricNormal, i);
    v.front = dot(v.Ng, d) < 0.0f;
    float4 bcm, nr;
    float ior, transmission = 0.0f;
    if (in.format == kGbFormatPacked) {
        bcm = gbp_unpack_base_color_metalness(static_cast<const uint32_t*>(in.BaseColorMetalness)[i]);
        nr = gbp_unpack_normal_roughness(static_cast<const uint64_t*>(in.NormalRoughness)[i]);
        ior = gbp_unpack_ior(static_cast<const uint16_t*>(in.IOR)[i]);
        if (bcm.w < 1.0f) transmission = gbp_unpack_transmission(static_cast<const uint8_t*>(in.Transmission)[i]);
    } else {
        bcm = static_cast<const float4*>(in.BaseColorMetalness)[i];
        nr = static_cast<const float4*>(in.NormalRoughness)[i];
        ior = static_cast<const float*>(in.IOR)[i];
        if (bcm.w < 1.0f) transmission = static_cast<const float*>(in.Transmission)[i];
    }
    v.Ns = load3(nr);
    v.bsdf = bsdf_init(load3(bcm), bcm.w, nr.w, ior, transmission, v.front);
    v.emission = gbf_load_radiance(in, i);
    return v;
}

PT_HD GbVertex gbf_vertex(const HitMaterial& hm)
{
    GbVertex v;
    v.P = hm.hf.P; v.N = hm.hf.N; v.Ng = hm.hf.N; v.Ns = hm.Ns; v.emission = hm.emission;
    v.offset = hm.hf.offset; v.front = hm.hf.front; v.bsdf = hm.bsdf;
    return v;
}

// One pixel of pt_render_from_gbuffer; index = the pixel's texel.  The generator (rng_init, running on across the samples) and its draw
// order are pt_render's.  A miss (Position.w not finite) is its Radiance texel: nothing else is read and no ray is traced.  The texels of
// the first vertex are loaded again for every sample, and the DI again at the end, instead of being carried through the bounce loop (they
// stay in cache; carrying them costs registers in every instance).  rays counts the rays of the loop: there is no primary ray.
template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD f3 gbframe_pixel(const GbFrame& fr, const GbInput& in, uint32_t px, uint32_t py, size_t index, TraceFn&& trace, MaterialFn&& material, EnvFn&& env, uint32_t& rays)
{
    uint32_t rng = rng_init(px, py, fr.frame_index);
    if (!is_finite(in.Position[index].w)) return gbf_load_radiance(in, index);
    bool di_valid = false;
    if (in.di_diffuse) { f3 DI; di_valid = gbf_load_di(in, index, DI); }
    f3 acc = make_f3(0.0f, 0.0f, 0.0f);
    for (uint32_t sample = 0;;) {
        f3 o, d, T = make_f3(1.0f, 1.0f, 1.0f), srad = make_f3(0.0f, 0.0f, 0.0f);
        { float tmin, tmax; primary_ray(fr.cam, px, py, o, d, tmin, tmax); }  // the direction only: V and the front face of the first vertex
        bool drop_emission = false;  // the DI covers the second vertex's emission (:302)
        size_t texel = index;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(texel));  // (an index the compiler cannot see through: the loads below stay inside the sample loop)
#endif
        GbVertex v = gbf_primary_vertex(in, texel, in.Position[texel], d);
        for (uint32_t bounce = 0;; bounce++) {  // v: vertex `bounce`, d: the direction of the ray that arrived there
            const bool t_finite = is_finite(T.x) && is_finite(T.y) && is_finite(T.z);
            f3 emission = v.emission;
            if (bounce == 1u && drop_emission) emission = make_f3(0.0f, 0.0f, 0.0f);
            if (emission.x != 0.0f || emission.y != 0.0f || emission.z != 0.0f || !t_finite) srad = srad + T * emission;
            const bool last = bounce == fr.bounces;
            if (last && sample + 1u == fr.spp) break;  // the sample drawn on the final iteration is never used
            const Surf surf = surf_init(v.front, v.Ng, v.Ns);
            const f3 V = -d;
            float w[3];
            lobe_weights(v.bsdf, surf, V, w);
            float rnd[4];
            rnd[0] = rng_float(rng); rnd[1] = rng_float(rng); rnd[2] = rng_float(rng); rnd[3] = rng_float(rng);
            f3 L;
            int lobe;
            if (!bsdf_sample(v.bsdf, surf, V, w, rnd, L, lobe)) break;
            if (bounce == 0u) drop_emission = di_valid && lobe != kLobeTransmission;
            float pdf;
            f3 f;
            if (!bsdf_pdf_eval(v.bsdf, surf, L, V, w, lobe, pdf, f)) break;
            if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) break;
            { const float inv_pdf = pt_rcp(pdf); T = T * (f * inv_pdf); }
            if (fr.rr_enabled && bounce > 3u) {
                const float p = pt_max(T.x, pt_max(T.y, T.z));
                if (rng_float(rng) >= p) break;
                T = T * pt_rcp(p);
            }
            if (luminance(T) <= fr.throughput_threshold) break;
            if (last) break;
            o = spawn_origin(v.P, v.N, v.offset, L);
            d = L;
            float t;
            uint32_t id;
            trace(o, d, 0.0f, kInf, t, id);
            rays++;
            if (id == 0xFFFFFFFFu) {
                srad = srad + T * env(d);
                break;
            }
            v = gbf_vertex(material(id, o, d, t, false));
        }
        const f3 total = acc + srad;
        if (++sample == fr.spp) {
            f3 res = make_f3(0.0f, 0.0f, 0.0f);
            if (is_finite(total.x) && is_finite(total.y) && is_finite(total.z)) res = total * fr.inv_spp;
            if (di_valid) { f3 DI; gbf_load_di(in, index, DI); res = res + DI; }  // out.rgb += DI after the mean (:382)
            return res;
        }
        acc = total;
    }
}

#if defined(__HIPCC__)
// one lane per pixel of pm: out[out_index] from the texels at out_index; counter: the rays traced
hipError_t launch_gbframe(const SceneView& sv, const PixelMap& pm, const GbFrame& fr, const GbInput& in, float4* out, unsigned long long* counter, uint32_t grid,
                          hipStream_t stream);
#endif

}  // namespace pt
