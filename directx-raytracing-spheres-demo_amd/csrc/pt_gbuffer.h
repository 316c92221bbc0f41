// pt_gbuffer.h -- the G-buffer pass (row N6; Shaders/GBufferGeneration.hlsl::main restated for analytic spheres, DESIGN.md
// spec S12): what one pixel's primary hit writes into the 13 surface buffers.  gbuffer_pixel is the whole per-pixel pass after
// the trace; the kernel (pt_gbuffer.hip) and the host build of the tests (tests/hostshim/gbuffer_host.cpp) both call it, so the
// GPU output is checked bit for bit against this header compiled for the host.
//
// Recollections of the un-vendored MathLib / NRD functions the pass calls (External/NVIDIA/MathLib and NRD are empty), frozen here:
//   Packing::EncodeUnitVector(v, true)   octahedral, signed: v /= |v.x| + |v.y| + |v.z|; z < 0 folds xy to (1 - |v.yx|) * sgn(v.xy)
//                                         with sgn = step(0, x) * 2 - 1 (0 counts as positive)
//   Geometry::ProjectiveTransform(M, p)  [p, 1] . M with M's 16 floats as DirectXMath rows (the column_major float4x4 of
//                                         Camera.hlsli read by mul(M, v) is that product)
//   Geometry::GetScreenUv(M, p)          clip.xy / clip.w * (0.5, -0.5) + 0.5
//   NRD_MaterialFactors(N, V, Albedo, F0, Roughness)
//                                         Fenv = EnvironmentTerm_Rtg(F0, |N.V|, Roughness); diffuse = Albedo * (1 - Fenv),
//                                         specular = Fenv (the combination EstimateDiffuseProbability uses, BxDF.hlsli:21-34)
#pragma once

#include "pt_surface.h"

namespace pt {

// channel bits, in the order of PtGBuffer's fields
enum : uint32_t {
    kGbPosition = 1u << 0, kGbFlatNormal = 1u << 1, kGbGeometricNormal = 1u << 2, kGbLinearDepth = 1u << 3, kGbNormalizedDepth = 1u << 4,
    kGbMotionVector = 1u << 5, kGbBaseColorMetalness = 1u << 6, kGbDiffuseAlbedo = 1u << 7, kGbSpecularAlbedo = 1u << 8,
    kGbNormalRoughness = 1u << 9, kGbIOR = 1u << 10, kGbTransmission = 1u << 11, kGbRadiance = 1u << 12, kGbAll = (1u << 13) - 1u
};
constexpr uint32_t kGbProjected = kGbLinearDepth | kGbNormalizedDepth | kGbMotionVector;  // need clip = [P, 1] . WorldToProjection
constexpr uint32_t kGbMaterial = kGbBaseColorMetalness | kGbDiffuseAlbedo | kGbSpecularAlbedo | kGbNormalRoughness | kGbIOR | kGbTransmission;
constexpr uint32_t kGbMissChannels = kGbPosition | kGbLinearDepth | kGbNormalizedDepth | kGbMotionVector | kGbRadiance;
constexpr uint32_t kGbNoHit = 0xFFFFFFFFu;
constexpr float kGbMissDistance = 1e8f;  // a miss's HitInfo::Position = o + 1e8 d (RaytracingHelpers.hlsli:64)

// What the pass reads of the camera: the lens of primary_ray and three of PtCamera::Matrices
struct GBufferFrame {
    CameraParams cam;
    float width, height;            // RenderSize (UVs are relative to the whole image, whatever the rect)
    uint32_t reversed;              // Camera::IsNormalizedDepthReversed
    float world_to_projection[16];  // Matrices[5]
    float prev_world_to_projection[16];  // Matrices[2]
    float prev_world_to_view[16];   // Matrices[0]
};

// What it reads of the scene.  sph / mats / tex / tex_maps / rot as hit_material_at; prev_sph / prev_rot: the caller's previous
// pose of every sphere (PreviousObjectToWorld), null = the current one; is_static = SceneData.IsStatic (no previous pose at all)
struct GBufferScene {
    const float4* sph;
    const float4* mats;
    const TexView* tex;
    const uint32_t* tex_maps;
    const float4* rot;
    const float4* prev_sph;
    const float4* prev_rot;
    uint32_t is_static;
    uint32_t env_tex, env_cube;  // environment map (kNoTexture = EnvironmentLightColor / sky), as SceneView
    float env[4];
    float env_xf[9];
};

struct GBufferPixel {
    float4 Position;
    f2 FlatNormal, GeometricNormal;
    float LinearDepth, NormalizedDepth;
    f3 MotionVector;
    float4 BaseColorMetalness;
    f3 DiffuseAlbedo, SpecularAlbedo;
    float4 NormalRoughness;
    float IOR, Transmission;
    f3 Radiance;
    uint32_t mask;  // the channels the reference writes for this pixel (and the caller asked for); the others hold no value
};

PT_HD float4 gb_float4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

// Packing::EncodeUnitVector(v, true)
PT_HD f2 encode_unit_vector(f3 v)
{
    const float s = pt_abs(v.x) + pt_abs(v.y) + pt_abs(v.z);
    const float x = v.x / s, y = v.y / s, z = v.z / s;
    f2 e;
    if (z >= 0.0f) { e.x = x; e.y = y; return e; }
    e.x = (1.0f - pt_abs(y)) * (x >= 0.0f ? 1.0f : -1.0f);
    e.y = (1.0f - pt_abs(x)) * (y >= 0.0f ? 1.0f : -1.0f);
    return e;
}

// Geometry::ProjectiveTransform: [p, 1] . M
PT_HD float4 project_point(const float* m, f3 p)
{
    return gb_float4(pt_fma(p.z, m[8], pt_fma(p.y, m[4], pt_fma(p.x, m[0], m[12]))), pt_fma(p.z, m[9], pt_fma(p.y, m[5], pt_fma(p.x, m[1], m[13]))),
                     pt_fma(p.z, m[10], pt_fma(p.y, m[6], pt_fma(p.x, m[2], m[14]))), pt_fma(p.z, m[11], pt_fma(p.y, m[7], pt_fma(p.x, m[3], m[15]))));
}

// Geometry::GetScreenUv
PT_HD f2 screen_uv(const float* m, f3 p)
{
    const float4 c = project_point(m, p);
    f2 uv;
    uv.x = pt_fma(c.x / c.w, 0.5f, 0.5f);
    uv.y = pt_fma(c.y / c.w, -0.5f, 0.5f);
    return uv;
}

// CalculateMotionVector (GBufferGeneration.hlsl:63-95): P = this frame's position, Pprev = where the same surface point was
PT_HD f3 motion_vector(const GBufferFrame& fr, f2 uv, float linear_depth, f3 Pprev)
{
    const f2 uvp = screen_uv(fr.prev_world_to_projection, Pprev);
    return make_f3((uvp.x - uv.x) * fr.width, (uvp.y - uv.y) * fr.height, project_point(fr.prev_world_to_view, Pprev).z - linear_depth);
}

// The previous position of the point of sphere `id` with outward normal N (spec S12): c' + r' rot(q', rot(conj q, N)) -- object
// space as hit_uv_rot forms it, so the point keeps its texture coordinates; the rotations only where the caller gave previous ones
PT_HD f3 previous_position(const GBufferScene& sc, uint32_t id, f3 P, f3 N)
{
    if (sc.is_static || (!sc.prev_sph && !sc.prev_rot)) return P;
    const float4 ps = sc.prev_sph ? sc.prev_sph[id] : sc.sph[id];
    f3 n = N;
    if (sc.prev_rot) {
        const float4 q = sc.rot ? sc.rot[id] : gb_float4(0.0f, 0.0f, 0.0f, 1.0f);
        const float4 qp = sc.prev_rot[id];
        n = quat_rotate(qp.x, qp.y, qp.z, qp.w, quat_rotate(-q.x, -q.y, -q.z, q.w, N));
    }
    return mad(ps.w, n, load3(ps));
}

// The pass for pixel (px, py) whose primary ray hit sphere `id` at t (id == kGbNoHit: a miss).  want: the requested channels.
template <bool kTex>
PT_HD GBufferPixel gbuffer_pixel(const GBufferFrame& fr, const GBufferScene& sc, uint32_t px, uint32_t py, float t, uint32_t id, uint32_t want)
{
    GBufferPixel g;
    f3 o, d;
    float tmin, tmax;
    primary_ray(fr.cam, px, py, o, d, tmin, tmax);
    f2 uv;  // Math::CalculateUV, the arithmetic of primary_ray
    uv.x = ((float)px + 0.5f + fr.cam.JitterX) * fr.cam.InvW;
    uv.y = ((float)py + 0.5f + fr.cam.JitterY) * fr.cam.InvH;
    if (id == kGbNoHit) {
        g.mask = want & kGbMissChannels;
        g.Position = gb_float4(kInf, kInf, kInf, kInf);
        g.LinearDepth = kInf;
        g.NormalizedDepth = fr.reversed ? 0.0f : 1.0f;
        if (want & kGbMotionVector) {
            const f3 Pm = mad(kGbMissDistance, d, o);
            g.MotionVector = motion_vector(fr, uv, project_point(fr.world_to_projection, Pm).w, Pm);
        }
        if (want & kGbRadiance) {
            if (kTex && sc.env_tex != kNoTexture)
                g.Radiance = sc.env_cube ? environment_cube(sc.tex + sc.env_tex, sc.env_xf, d) : environment_texture(sc.tex[sc.env_tex], sc.env_xf, d);
            else g.Radiance = environment_color(sc.env[0], sc.env[1], sc.env[2], sc.env[3], d);
        }
        return g;
    }
    uint32_t mask = want & (kGbAll & ~kGbTransmission);
    const float4 sp = sc.sph[id];
    const HitFrame hf = hit_frame(o, d, t, load3(sp), sp.w);
    g.Position = gb_float4(hf.P.x, hf.P.y, hf.P.z, hf.offset);
    g.FlatNormal = encode_unit_vector(hf.N);  // a sphere's flat and geometric normals are one vector
    g.GeometricNormal = g.FlatNormal;
    if (want & kGbProjected) {
        const float4 clip = project_point(fr.world_to_projection, hf.P);
        g.LinearDepth = clip.w;
        g.NormalizedDepth = clip.z / clip.w;
        if (want & kGbMotionVector) g.MotionVector = motion_vector(fr, uv, clip.w, previous_position(sc, id, hf.P, hf.N));
    }
    if (want & (kGbMaterial | kGbRadiance)) {
        const HitMaterial hm = hit_material_at<kTex>(sc.sph, sc.mats, sc.tex, sc.tex_maps, sc.rot, id, o, d, t, true);
        const Bsdf& b = hm.bsdf;
        g.BaseColorMetalness = gb_float4(b.BaseColor.x, b.BaseColor.y, b.BaseColor.z, b.Metallic);
        if (want & (kGbDiffuseAlbedo | kGbSpecularAlbedo)) {
            const f3 fe = environment_term_rtg(b.F0, pt_abs(dot(hm.Ns, -d)), b.Roughness);  // NRD_MaterialFactors
            g.DiffuseAlbedo = b.Albedo * make_f3(1.0f - fe.x, 1.0f - fe.y, 1.0f - fe.z);
            g.SpecularAlbedo = fe;
        }
        g.NormalRoughness = gb_float4(hm.Ns.x, hm.Ns.y, hm.Ns.z, b.Roughness);
        g.IOR = sc.mats[id * 4 + 2].z;  // Material::IOR
        g.Transmission = b.Transmission;
        if (b.Metallic < 1.0f) mask |= want & kGbTransmission;  // GBufferGeneration.hlsl:191-195
        g.Radiance = hm.emission;  // Material::GetEmission
    }
    g.mask = mask;
    return g;
}

}  // namespace pt
