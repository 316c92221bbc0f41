// restir_host.cpp -- TEST SHIM: compiles the product's reservoir-pass header (csrc/pt_restir.h, with pt_surface.h's hit material) as
// plain host C++ (the flags of gbuffer_host.cpp) so the tests can check it pass by pass against the float64 restatement without a
// GPU, and the GPU kernels against it bit for bit.  The scene arrives as the C-ABI receives it and is converted the way pt_set_scene
// / pt_set_textures convert it for the device; the visibility query is a brute-force closest hit (nearest t, ties -> lowest id, the
// alpha test of spec S10 per crossing), which the device walkers equal bit for bit.  Not part of the product; never loaded by it.
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_surface.h"
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_restir.h"
#include <cstring>
#include <vector>

using namespace pt;

namespace {

struct HostScene {
    std::vector<float4> sph, mats, rots;
    std::vector<uint32_t> tex_maps, lights, cls;  // cls: 0 visible, 1 tested per crossing, 2 invisible (pt_device.h's alpha classes)
    std::vector<TexView> views;
    bool tex = false;

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

    void trace(f3 o, f3 d, float& t_out, uint32_t& id_out) const
    {
        float best = kInf;
        uint32_t best_id = kRiNoHit;
        for (uint32_t i = 0; i < (uint32_t)sph.size(); i++) {
            if (cls[i] == 2u) continue;
            const f3 C = make_f3(sph[i].x, sph[i].y, sph[i].z);
            float t;
            if (!intersect_sphere(o, d, 0.0f, kInf, C, sph[i].w, t)) continue;
            bool ok = true;
            while (cls[i] == 1u && !crossing_is_opaque(i, C, o, d, t)) {
                float t2;
                if (!intersect_sphere(o, d, t, kInf, C, sph[i].w, t2)) { ok = false; break; }
                t = t2;
            }
            if (ok && t < best) { best = t; best_id = i; }
        }
        t_out = best; id_out = best_id;
    }
};

}  // namespace

extern "C" {

// One pt_restir_di call (or one of its two launches) over caller-owned history arrays.
// spheres, materials[n]: pt_set_scene's arguments; texels / tex_info / n_tex / maps / rot: as gb_pixels (gbuffer_host.cpp).
// prm = {w, h, FrameIndex, initial_samples, temporal, temporal_bias, max_history, spatial, spatial_bias, spatial_samples, history_valid,
//        launches (bit 0: launch 1, bit 1: launch 2, bit 2: the spatial pass alone, see below)} with the defaults already applied; fprm = {radius, cam_pos[3], prev_cam_pos[3]}.
// ptrs = Position, GeometricNormal, LinearDepth, MotionVector, BaseColorMetalness, NormalRoughness, IOR, Transmission,
//        this call's slot {rec0, rec1, rec2, rec3, rec_t, res0, res1}, the previous call's slot (same seven), Diffuse, Specular.
void ri_host_call(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                  const uint32_t* maps, const float* rot, const uint32_t* prm, const float* fprm, void* const* ptrs)
{
    HostScene hs;
    hs.tex = n_tex != 0;
    hs.sph.resize(n);
    hs.mats.resize(4 * (size_t)n);
    std::memcpy(hs.sph.data(), spheres, (size_t)n * sizeof(float4));
    if (n_tex) {
        hs.tex_maps.assign((size_t)n * 8u, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < n; i++) hs.tex_maps[(size_t)i * 8u + 7u] = 0u;
        if (maps) std::memcpy(hs.tex_maps.data(), maps, hs.tex_maps.size() * sizeof(uint32_t));
    }
    hs.cls.assign(n, 0u);
    for (uint32_t i = 0; i < n; i++) {
        PtMaterial m = materials[i];
        const float f0d = dielectric_f0(m.IOR), inv_ior = 1.0f / m.IOR;
        std::memcpy(&m._pad[0], &f0d, 4);
        std::memcpy(&m._pad[1], &inv_ior, 4);
        m.AlphaMode &= ~kMaterialHasMaps;
        if (n_tex && hs.tex_maps[(size_t)i * 8u + 7u]) m.AlphaMode |= kMaterialHasMaps;
        std::memcpy(&hs.mats[4 * (size_t)i], &m, sizeof m);
        // pt_set_scene's emitter list and alpha classes
        if (m.EmissiveStrength * m.EmissiveColor[0] > 0.0f || m.EmissiveStrength * m.EmissiveColor[1] > 0.0f || m.EmissiveStrength * m.EmissiveColor[2] > 0.0f)
            hs.lights.push_back(i);
        if (materials[i].AlphaMode != PT_ALPHA_OPAQUE) {
            const float* bc = materials[i].BaseColor;
            const bool sampled = n_tex && hs.tex_maps[(size_t)i * 8u + kMapBaseColor] != kNoTexture && (bc[0] > 0.0f || bc[1] > 0.0f || bc[2] > 0.0f || bc[3] > 0.0f);
            hs.cls[i] = sampled ? 1u : (bc[3] >= materials[i].AlphaCutoff ? 0u : 2u);
        }
    }
    hs.views.resize(n_tex);
    for (uint32_t k = 0; k < n_tex; k++)
        hs.views[k] = TexView{ reinterpret_cast<const float4*>(texels) + tex_info[3 * k], tex_info[3 * k + 1], tex_info[3 * k + 2] };
    hs.rots.resize(n);
    for (uint32_t i = 0; i < n; i++) { hs.rots[i].x = hs.rots[i].y = hs.rots[i].z = 0.0f; hs.rots[i].w = 1.0f; }
    if (rot) std::memcpy(hs.rots.data(), rot, (size_t)n * sizeof(float4));
    if (hs.lights.empty()) return;  // pt_restir_di: no emitters, nothing is written

    RiBuffers b{};
    b.w = prm[0]; b.h = prm[1];
    b.position = static_cast<const float4*>(ptrs[0]);
    b.geometric_normal = static_cast<const float*>(ptrs[1]);
    b.linear_depth = static_cast<const float*>(ptrs[2]);
    b.motion_vector = static_cast<const float*>(ptrs[3]);
    b.base_color_metalness = static_cast<const float4*>(ptrs[4]);
    b.normal_roughness = static_cast<const float4*>(ptrs[5]);
    b.ior = static_cast<const float*>(ptrs[6]);
    b.transmission = static_cast<const float*>(ptrs[7]);
    for (int k = 0; k < 4; k++) { b.rec[k] = static_cast<float4*>(ptrs[8 + k]); b.prev_rec[k] = static_cast<const float4*>(ptrs[15 + k]); }
    b.rec_t = static_cast<float*>(ptrs[12]);
    b.prev_rec_t = static_cast<const float*>(ptrs[19]);
    for (int k = 0; k < 2; k++) { b.res[k] = static_cast<float4*>(ptrs[13 + k]); b.prev_res[k] = static_cast<const float4*>(ptrs[20 + k]); }
    b.out_diffuse = static_cast<float4*>(ptrs[22]);
    b.out_specular = static_cast<float4*>(ptrs[23]);
    RiParams P{};
    P.frame_index = prm[2]; P.initial_samples = prm[3]; P.temporal = prm[4]; P.temporal_bias = prm[5]; P.max_history = prm[6];
    P.spatial = prm[7]; P.spatial_bias = prm[8]; P.spatial_samples = prm[9]; P.history_valid = prm[10];
    P.radius = fprm[0];
    P.cam_pos = make_f3(fprm[1], fprm[2], fprm[3]);
    P.prev_cam_pos = make_f3(fprm[4], fprm[5], fprm[6]);
    RiScene sc{};
    sc.sph = hs.sph.data(); sc.mats = hs.mats.data(); sc.lights = hs.lights.data(); sc.n_lights = (uint32_t)hs.lights.size();
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { hs.trace(o, d, t, id); };
    auto emit = [&](uint32_t id, f3 o, f3 d, float t) {
        return hs.tex ? hit_material_at<true>(hs.sph.data(), hs.mats.data(), hs.views.data(), hs.tex_maps.data(), hs.rots.data(), id, o, d, t, false).emission
                      : hit_material_at<false>(hs.sph.data(), hs.mats.data(), nullptr, nullptr, nullptr, id, o, d, t, false).emission;
    };
    // what each lane of pt_restir.hip does, one launch after the other
    if (prm[11] & 1u)
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) ri_pass1_px(b, sc, P, x, y, trace);
    if (prm[11] & 2u)
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) ri_pass2_px(b, sc, P, x, y, trace, emit);
    // bit 2: launch 2's spatial pass alone; the reservoir it hands to final shading is written in the layout of a slot's reservoir planes
    // to Diffuse / Specular (pixels without a surface are left as they are)
    if (prm[11] & 4u) {
        float4* const planes[2] = { b.out_diffuse, b.out_specular };
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) {
                const uint32_t i = y * b.w + x;
                const RiRecord rec = ri_load_record(b.rec, b.rec_t, i);
                if (!is_finite(rec.r3.z)) continue;
                ri_store_reservoir(planes, i, ri_spatial(b, sc, P, ri_surface(rec, P.cam_pos), ri_load_reservoir(b.res, i), x, y, trace));
            }
    }
}

void ri_host_decode_unit_vector(const float e[2], float out[3])
{
    const f3 v = decode_unit_vector(e[0], e[1]);
    out[0] = v.x; out[1] = v.y; out[2] = v.z;
}

}  // extern "C"
