// pt_lens.h -- the thin-lens camera of row N26 (pt_render_lens, DESIGN.md spec S29): Camera::GenerateThinLensRay (Shaders/Camera.hlsli:43-54),
// which the reference declares and never calls (its raygen loads the primary hit from the pinhole G-buffer), in front of pt_render's
// bounce loop.  ImportanceSampling::Uniform::GetRay is MathLib's: its body here is frozen from recollection and is this project's own.
// Everything compiles on the device (pt_lens.hip) and as host C++ (the bit-parity tests):
//   lens_get_ray   ImportanceSampling::Uniform::GetRay(u).xy
//   lens_ray       the lens ray of a pixel and a lens sample
//   lens_pixel     one pixel of the frame: every sample traces its own primary ray from its own lens point, then pt_render's DEFAULT loop
// The functors are those of pt_sharc.h: trace(o, d, tmin, tmax, t, id), material(id, o, d, t, primary) -> HitMaterial, env(d).
// PtCamera::ApertureRadius is read here and nowhere else: it travels in LensFrame, not in CameraParams.
#pragma once

#include "pt_surface.h"

namespace pt {

constexpr uint32_t kLensSeed = 0x4C454E53u;  // "LENS": the lens stream is hash_combine(rng_init(px, py, FrameIndex), kLensSeed)

struct LensFrame {
    CameraParams cam;
    f3 RightN, UpN;  // normalize(Right), normalize(Up) of GenerateThinLensRay, hoisted on the host with the same arithmetic
    float aperture;  // ApertureRadius; 0 = the pinhole camera (primary_ray itself)
    uint32_t frame_index, bounces, spp, rr_enabled;
    float throughput_threshold, inv_spp;
};

PT_HD LensFrame lens_frame(const PtCamera& c, uint32_t w, uint32_t h, uint32_t frame_index, uint32_t bounces, uint32_t spp, bool rr_enabled, float throughput_threshold)
{
    LensFrame fr;
    fr.cam = camera_params(c, w, h);
    fr.RightN = normalize(fr.cam.Right);
    fr.UpN = normalize(fr.cam.Up);
    fr.aperture = c.ApertureRadius;
    fr.frame_index = frame_index; fr.bounces = bounces; fr.spp = spp; fr.rr_enabled = rr_enabled ? 1u : 0u;
    fr.throughput_threshold = throughput_threshold;
    fr.inv_spp = 1.0f / (float)spp;
    return fr;
}

// GetRay(u) = (r cos phi, r sin phi, z), phi = 2 pi u.x, z = u.y, r = Sqrt01(1 - z^2); the lens takes .xy.  Not uniform on the disc:
// r = sqrt(1 - u^2) crowds the rim, E[r^2] = 2/3.  No pdf weight is applied, as in the shader text.
PT_HD void lens_get_ray(float u1, float u2, float& x, float& y)
{
    float s, c;
    sincos_2pi(u1, s, c);
    const float r = sqrt01(1.0f - u2 * u2);
    x = r * c;
    y = r * s;
}

// Camera.hlsli:43-54 for pixel (px, py) and lens sample (u1, u2); NDC and the unnormalised direction as primary_ray forms them
PT_HD void lens_ray(const LensFrame& fr, uint32_t px, uint32_t py, float u1, float u2, f3& o, f3& d, float& tmin, float& tmax)
{
    const CameraParams& cam = fr.cam;
    float u = ((float)px + 0.5f + cam.JitterX) * cam.InvW;
    float v = ((float)py + 0.5f + cam.JitterY) * cam.InvH;
    float nx = pt_fma(u, 2.0f, -1.0f);
    float ny = pt_fma(v, -2.0f, 1.0f);
    const f3 D = mad(ny, cam.Up, cam.Right * nx) + cam.Forward;
    float vx, vy;
    lens_get_ray(u1, u2, vx, vy);
    const f3 offset = (fr.RightN * vx + fr.UpN * vy) * fr.aperture;
    o = cam.Position + offset;
    d = normalize(D - offset);
    float inv_cos = pt_rcp(dot(cam.ForwardN, d));
    tmin = cam.Near * inv_cos;
    tmax = cam.Far * inv_cos;
}

// One pixel of pt_render_lens.  The bounce generator (rng_init, running on across the samples) and its draw order are pt_render's; the lens
// draws two numbers per sample from a stream of its own.  The lens ray is the ray of "bounce -1": the loop's one trace call serves it and
// the bounce rays alike (a second inlined copy of the walker costs registers: pt_sharc.h, sh_query_pixel_t).  aperture == 0: every sample's
// ray is primary_ray's, and a pixel whose ray misses is the environment itself, as pt_render returns it (not the mean of spp copies of it).
template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD f3 lens_pixel(const LensFrame& fr, uint32_t px, uint32_t py, TraceFn&& trace, MaterialFn&& material, EnvFn&& env, uint32_t& rays)
{
    uint32_t rng = rng_init(px, py, fr.frame_index);
    uint32_t lens = hash_combine(rng, kLensSeed);
    const bool pinhole = fr.aperture == 0.0f;
    f3 acc = make_f3(0.0f, 0.0f, 0.0f);
    for (uint32_t sample = 0;;) {
        f3 o, d, T = make_f3(1.0f, 1.0f, 1.0f), srad = make_f3(0.0f, 0.0f, 0.0f);
        float tmin, tmax;
        if (pinhole) {
            primary_ray(fr.cam, px, py, o, d, tmin, tmax);
        } else {
            const float u1 = rng_float(lens), u2 = rng_float(lens);
            lens_ray(fr, px, py, u1, u2, o, d, tmin, tmax);
        }
        for (uint32_t bounce = 0;; bounce++) {  // (o, d, tmin, tmax): the ray that arrives at vertex `bounce`
            float t;
            uint32_t id;
            trace(o, d, tmin, tmax, t, id);
            rays++;
            if (id == 0xFFFFFFFFu) {
                if (pinhole && bounce == 0u) return env(d);
                srad = srad + T * env(d);
                break;
            }
            const HitMaterial hm = material(id, o, d, t, bounce == 0u);
            const bool t_finite = is_finite(T.x) && is_finite(T.y) && is_finite(T.z);
            const f3 emission = hm.emission;
            if (emission.x != 0.0f || emission.y != 0.0f || emission.z != 0.0f || !t_finite) srad = srad + T * emission;
            const bool last = bounce == fr.bounces;
            if (last && sample + 1u == fr.spp) break;  // the sample drawn on the final iteration is never used
            const Surf surf = surf_init(hm.hf.front, hm.hf.N, hm.Ns);
            const f3 V = -d;
            float w[3];
            lobe_weights(hm.bsdf, surf, V, w);
            float rnd[4];
            rnd[0] = rng_float(rng); rnd[1] = rng_float(rng); rnd[2] = rng_float(rng); rnd[3] = rng_float(rng);
            f3 L;
            int lobe;
            if (!bsdf_sample(hm.bsdf, surf, V, w, rnd, L, lobe)) break;
            float pdf;
            f3 f;
            if (!bsdf_pdf_eval(hm.bsdf, surf, L, V, w, lobe, pdf, f)) break;
            if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) break;
            { const float inv_pdf = pt_rcp(pdf); T = T * (f * inv_pdf); }
            if (fr.rr_enabled && bounce > 3u) {
                const float p = pt_max(T.x, pt_max(T.y, T.z));
                if (rng_float(rng) >= p) break;
                T = T * pt_rcp(p);
            }
            if (luminance(T) <= fr.throughput_threshold) break;
            if (last) break;
            o = spawn_origin(hm.hf.P, hm.hf.N, hm.hf.offset, L);
            d = L;
            tmin = 0.0f; tmax = kInf;
        }
        const f3 total = acc + srad;
        if (++sample == fr.spp) {
            if (is_finite(total.x) && is_finite(total.y) && is_finite(total.z)) return total * fr.inv_spp;
            return make_f3(0.0f, 0.0f, 0.0f);
        }
        acc = total;
    }
}

#if defined(__HIPCC__)
struct SceneView;
struct PixelMap;
// one lane per pixel of pm into out[out_index]; counter: the rays traced
hipError_t launch_lens(const SceneView& sv, const PixelMap& pm, const LensFrame& fr, float4* out, unsigned long long* counter, uint32_t grid, hipStream_t stream);
#endif

}  // namespace pt
