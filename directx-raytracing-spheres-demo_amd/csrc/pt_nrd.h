// pt_nrd.h -- the NRD composition pass (row N8): PostProcessing::NRDComposition, Shaders/NRDComposition.hlsl, driven by
// App::ProcessNRD (Source/App.cpp:1549-1642).  Pack (before NRD) divides the albedo out of the noisy Diffuse / Specular in place
// and applies the NRD front-end of the mode; compose (after NRD) applies the back-end to the denoised buffers, multiplies the
// albedo back in and adds both lobes to the radiance.  The NRD front-end / back-end functions (NRD.hlsli, NRDEncoding.hlsli of the
// NRD 4.x submodule, which the reference does not vendor) are a recollection frozen for the build: DESIGN.md spec S14.
// Per-pixel functions for the kernels of pt_nrd.hip; they also compile as host C++ (tests/hostshim/nrd_host.cpp).
#pragma once

#include "pt_texture.h"

namespace pt {

constexpr uint32_t kNrdReblur = 2, kNrdRelax = 3;  // Denoiser::NRDReBLUR, NRDReLAX (Shaders/Denoiser.hlsli)
constexpr float kNrdFp16Max = 65504.0f;            // NRD_FP16_MAX
constexpr float kNrdEps = 1e-6f;                   // NRD_EPS

// nrd::ReblurSettings::hitDistanceParameters {A, B, C, D}: hit distance normalisation (A + |viewZ| B) lerp(1, C, saturate(exp2(D r^2)))
struct NrdHitDistParams { float x, y, z, w; };

// REBLUR_FrontEnd_GetNormHitDist: saturate(h / ((P.x + |z| P.y) (1 + (P.z - 1) saturate(exp2((P.w r) r)))))
PT_HD float nrd_norm_hit_dist(float h, float z, NrdHitDistParams P, float r)
{
    const float f = (P.x + pt_abs(z) * P.y) * (1.0f + (P.z - 1.0f) * saturate(exp2_spec((P.w * r) * r)));
    return saturate(h / f);
}

// the sanitising of the NRD front-ends (sanitize = true): a lobe with any non-finite channel becomes black, else [0, 65504]
PT_HD f3 nrd_sanitize_rgb(f3 c)
{
    if (!is_finite(c.x) || !is_finite(c.y) || !is_finite(c.z)) return make_f3(0.0f, 0.0f, 0.0f);
    return make_f3(pt_min(pt_max(c.x, 0.0f), kNrdFp16Max), pt_min(pt_max(c.y, 0.0f), kNrdFp16Max), pt_min(pt_max(c.z, 0.0f), kNrdFp16Max));
}

// "0" marks a sample without data: any other hit distance is at least NRD_EPS
PT_HD float nrd_keep_nonzero(float a) { return a != 0.0f ? pt_max(a, kNrdEps) : a; }

// _NRD_LinearToYCoCg: three dot products, each summed left to right (no contraction: -ffp-contract=off)
PT_HD f3 nrd_linear_to_ycocg(f3 c)
{
    return make_f3(c.x * 0.25f + c.y * 0.5f + c.z * 0.25f, c.x * 0.5f + c.y * 0.0f + c.z * -0.5f, c.x * -0.25f + c.y * 0.5f + c.z * -0.25f);
}

// _NRD_YCoCgToLinear: max(., 0) as HLSL max (NaN -> 0)
PT_HD f3 nrd_ycocg_to_linear(f3 c)
{
    const float t = c.x - c.z;
    return make_f3(pt_max(t + c.y, 0.0f), pt_max(c.x + c.z, 0.0f), pt_max(t - c.y, 0.0f));
}

// REBLUR_FrontEnd_PackRadianceAndNormHitDist(rgb, a, true)
PT_HD float4 nrd_reblur_pack(f3 rgb, float a)
{
    const f3 c = nrd_linear_to_ycocg(nrd_sanitize_rgb(rgb));
    a = nrd_keep_nonzero(is_finite(a) ? saturate(a) : 0.0f);
    float4 r; r.x = c.x; r.y = c.y; r.z = c.z; r.w = a;
    return r;
}

// RELAX_FrontEnd_PackRadianceAndHitDist(rgb, a, true)
PT_HD float4 nrd_relax_pack(f3 rgb, float a)
{
    const f3 c = nrd_sanitize_rgb(rgb);
    a = nrd_keep_nonzero(is_finite(a) ? pt_min(pt_max(a, 0.0f), kNrdFp16Max) : 0.0f);
    float4 r; r.x = c.x; r.y = c.y; r.z = c.z; r.w = a;
    return r;
}

// the radiance of a denoised lobe: REBLUR_BackEnd_UnpackRadianceAndNormHitDist / RELAX_BackEnd_UnpackRadiance (identity)
template <uint32_t kMode>
PT_HD f3 nrd_unpack_rgb(float4 v)
{
    const f3 c = make_f3(v.x, v.y, v.z);
    return kMode == kNrdReblur ? nrd_ycocg_to_linear(c) : c;
}

// Pack of one hit pixel (finite LinearDepth z), in place on the noisy lobes d and s.  The quotients are IEEE divisions: an albedo
// channel of 0 makes its quotient inf or NaN, and the sanitising then zeroes all three channels of that lobe.  roughness
// (NormalRoughness.w) is read by ReBLUR only.
template <uint32_t kMode>
PT_HD void nrd_pack_px(float z, f3 diffuse_albedo, f3 specular_albedo, float roughness, NrdHitDistParams P, float4& d, float4& s)
{
    const f3 dr = make_f3(d.x / diffuse_albedo.x, d.y / diffuse_albedo.y, d.z / diffuse_albedo.z);
    const f3 sr = make_f3(s.x / specular_albedo.x, s.y / specular_albedo.y, s.z / specular_albedo.z);
    if (kMode == kNrdReblur) {
        d = nrd_reblur_pack(dr, nrd_norm_hit_dist(d.w, z, P, 1.0f));
        s = nrd_reblur_pack(sr, nrd_norm_hit_dist(s.w, z, P, roughness));
    } else {
        d = nrd_relax_pack(dr, d.w);
        s = nrd_relax_pack(sr, s.w);
    }
}

// Compose of one hit pixel: radiance.rgb + (d.rgb * DiffuseAlbedo + s.rgb * SpecularAlbedo), alpha unchanged
template <uint32_t kMode>
PT_HD float4 nrd_compose_px(float4 radiance, f3 diffuse_albedo, f3 specular_albedo, float4 d, float4 s)
{
    const f3 l = nrd_unpack_rgb<kMode>(d) * diffuse_albedo + nrd_unpack_rgb<kMode>(s) * specular_albedo;
    radiance.x = radiance.x + l.x;
    radiance.y = radiance.y + l.y;
    radiance.z = radiance.z + l.z;
    return radiance;
}

// the buffers of one call (NRDComposition::Textures), all n_pixels long; what a direction does not use may be null
struct NrdBuffers {
    const float* linear_depth;
    const float* diffuse_albedo;   // float3
    const float* specular_albedo;  // float3
    const float4* normal_roughness;
    float4* noisy_diffuse;
    float4* noisy_specular;
    const float4* denoised_diffuse;
    const float4* denoised_specular;
    float4* radiance;
};

#if defined(__HIPCC__)
// pt_nrd.hip: pack (in place on the noisy buffers) or compose (into the radiance) of mode kNrdReblur / kNrdRelax, one launch on `stream`
hipError_t launch_nrd_composition(const NrdBuffers& b, uint32_t n_pixels, bool pack, uint32_t mode, NrdHitDistParams P, hipStream_t stream);
#endif

}  // namespace pt
