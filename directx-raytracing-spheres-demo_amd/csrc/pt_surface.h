// pt_surface.h -- the surface a ray hit: the sphere's texture coordinates and the material after EvaluateMaterial + BSDFSample
// (HitInfo.hlsli, ShadingHelpers.hlsli:161-235, BxDF.hlsli:36-79), over plain pointers so that the same code runs in the
// kernels (pt_trace.h hit_material: SceneView's arrays) and on the host (the G-buffer's bit-parity tests, pt_gbuffer.h).
#pragma once

#include "pt_texture.h"

#if !defined(__HIPCC__)
struct uint4 { uint32_t x, y, z, w; };  // host build of the tests (as float4 in pt_texture.h)
#endif

namespace pt {

constexpr uint32_t kMaterialHasMaps = 0x80000000u;  // device copy of PtMaterial::AlphaMode, bit 31: the sphere has texture maps (pt_set_textures)

PT_HD f3 load3(const float4& v) { return make_f3(v.x, v.y, v.z); }

// texture coordinates of the point of sphere `id` whose outward world-space normal is N (spec S6): q = the object's rotation,
// n_mesh = the mesh-space normal the coordinates (and the tangent) derive from
PT_HD f2 hit_uv_rot(const float4* __restrict__ rot, uint32_t id, f3 N, float4& q, f3& n_mesh)
{
    q = rot[id];
    const f3 n_obj = quat_rotate(-q.x, -q.y, -q.z, q.w, N);  // world -> object: the conjugate rotation
    // ObjectToWorld = diag(1, 1, -1) * pose (Scene.ixx:197-199): the mesh-space normal is the z mirror of the object-space
    // one (settled against the reference's screenshot with its own Earth map: without it the continents are mirrored)
    n_mesh = make_f3(n_obj.x, n_obj.y, -n_obj.z);
    return sphere_uv(n_mesh);
}

// What a hit needs for shading: geometry frame, the material after EvaluateMaterial (textures when kTex), BSDFSample.
struct HitMaterial {
    HitFrame hf;
    f3 emission, Ns;
    Bsdf bsdf;
};

// sph / mats: the scene's spheres and device materials (4 float4 per PtMaterial, padding words as pt_set_scene fills them);
// tex / tex_maps / rot: the texture table, 8 map words per sphere and the rotations (read only when kTex)
template <bool kTex>
PT_HD HitMaterial hit_material_at(const float4* sph, const float4* mats, const TexView* tex, const uint32_t* tex_maps, const float4* rot, uint32_t id, f3 o, f3 d, float t, bool primary)
{
    HitMaterial r;
    const float4 sp = sph[id];
    const float4 m0 = mats[id * 4 + 0], m1 = mats[id * 4 + 1], m2 = mats[id * 4 + 2], m3 = mats[id * 4 + 3];
    r.hf = hit_frame(o, d, t, load3(sp), sp.w);
    f3 base = load3(m0), emissive_color = make_f3(m1.y, m1.z, m1.w);
    float metallic = m2.x, roughness = m2.y, transmission_m = m2.w;
    f3 Ns = r.hf.front ? r.hf.N : -r.hf.N;  // HitInfo.hlsli:60-64
    // (bit 31 of the device copy's AlphaMode word = "this sphere has texture maps", set by pt_set_textures: an untextured sphere in a textured
    // scene -- almost every hit of the demo -- costs no look-up of its map table, which would sit on the dependent chain of every bounce)
    if (kTex && (as_uint(m3.x) & kMaterialHasMaps) != 0u) {
        const uint4* mp = reinterpret_cast<const uint4*>(tex_maps + (size_t)id * 8u);
        const uint4 ma = mp[0], mb = mp[1];
        {
            const uint32_t maps[kMapCount] = { ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z };
            float4 q;
            f3 n_mesh;
            const f2 uv = hit_uv_rot(rot, id, r.hf.N, q, n_mesh);
            const f3 t_mesh = sphere_tangent(n_mesh);
            f3 T = quat_rotate(q.x, q.y, q.z, q.w, make_f3(t_mesh.x, t_mesh.y, -t_mesh.z));
            if (!r.hf.front) T = -T;  // HitInfo::GetFrontTangent
            const MaterialEval me = evaluate_material(tex, maps, uv, base, m1.x, emissive_color, metallic, roughness, transmission_m, Ns, T);
            base = me.BaseColor; emissive_color = me.EmissiveColor; metallic = me.Metallic; roughness = me.Roughness;
            transmission_m = me.Transmission; Ns = me.Ns;
        }
    }
    r.emission = emissive_color * m1.x;  // Material::GetEmission
    r.Ns = Ns;
    // the primary hit mirrors the G-buffer round trip: Transmission = Metallic < 1 ? Transmission : 0 (Raytracing.hlsl:148)
    const float transmission = (primary && !(metallic < 1.0f)) ? 0.0f : transmission_m;
    // m3.z / m3.w: dielectric F0 and 1/IOR, precomputed per material by pt_set_scene (padding words of PtMaterial)
    r.bsdf = bsdf_init_pre(base, metallic, roughness, m2.z, m3.w, m3.z, transmission, r.hf.front);
    return r;
}

}  // namespace pt
