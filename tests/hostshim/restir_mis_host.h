// restir_mis_host.h -- TEST SHIM: the host side of spec S23 (pt_restir_di_ex, row N17) over the product's headers, shared by
// restir_mis_host.cpp (the tests' library) and tests/cpp/restir_mis_sanitize.cpp (the same code under ASan + UBSan).  The scene arrives
// as the C-ABI receives it and is converted the way pt_set_scene / pt_set_textures convert it (the emitter list, its inverse, the alpha
// classes); the visibility query is a brute-force closest hit (nearest t, ties -> lowest id, the alpha test of spec S10 per crossing),
// which the device walkers equal bit for bit; the presampled structures of spec S22 are lightris_host.h's.  Not part of the product.
#pragma once

#include "lightris_host.h"

struct RmHostScene {
    LrHostScene lr;  // sph, mats, lights (and the untextured alpha classes, which `cls` below replaces)
    std::vector<float4> rots;
    std::vector<uint32_t> tex_maps, cls, light_of;
    std::vector<TexView> views;
    bool tex = false;

    void set(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* texels, const uint32_t* tex_info, uint32_t n_tex, const uint32_t* maps,
             const float* rot)
    {
        lr.set(spheres, materials, n);
        tex = n_tex != 0;
        tex_maps.clear();
        if (n_tex) {
            tex_maps.assign((size_t)n * 8u, 0xFFFFFFFFu);
            for (uint32_t i = 0; i < n; i++) tex_maps[(size_t)i * 8u + 7u] = 0u;
            if (maps) std::memcpy(tex_maps.data(), maps, tex_maps.size() * sizeof(uint32_t));
        }
        cls.assign(n, 0u);
        for (uint32_t i = 0; i < n; i++) {
            if (n_tex && tex_maps[(size_t)i * 8u + 7u]) {  // pt_set_textures' "has texture maps" flag in the device copy of the material
                uint32_t mode;
                std::memcpy(&mode, reinterpret_cast<const char*>(&lr.mats[4 * (size_t)i]) + offsetof(PtMaterial, AlphaMode), 4);
                mode |= kMaterialHasMaps;
                std::memcpy(reinterpret_cast<char*>(&lr.mats[4 * (size_t)i]) + offsetof(PtMaterial, AlphaMode), &mode, 4);
            }
            if (materials[i].AlphaMode != PT_ALPHA_OPAQUE) {
                const float* bc = materials[i].BaseColor;
                const bool sampled = n_tex && tex_maps[(size_t)i * 8u + kMapBaseColor] != kNoTexture && (bc[0] > 0.0f || bc[1] > 0.0f || bc[2] > 0.0f || bc[3] > 0.0f);
                cls[i] = sampled ? 1u : (bc[3] >= materials[i].AlphaCutoff ? 0u : 2u);
            }
        }
        views.resize(n_tex);
        for (uint32_t k = 0; k < n_tex; k++)
            views[k] = TexView{ reinterpret_cast<const float4*>(texels) + tex_info[3 * k], tex_info[3 * k + 1], tex_info[3 * k + 2] };
        rots.resize(n);
        for (uint32_t i = 0; i < n; i++) { rots[i].x = rots[i].y = rots[i].z = 0.0f; rots[i].w = 1.0f; }
        if (rot) std::memcpy(rots.data(), rot, (size_t)n * sizeof(float4));
        light_of.assign(n, kRiNoHit);
        for (uint32_t j = 0; j < (uint32_t)lr.lights.size(); j++) light_of[lr.lights[j]] = j;
    }

    bool crossing_is_opaque(uint32_t id, f3 C, f3 o, f3 d, float t) const
    {
        const float base_alpha = lr.mats[id * 4 + 0].w, cutoff = lr.mats[id * 4 + 3].y;
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
        for (uint32_t i = 0; i < (uint32_t)lr.sph.size(); i++) {
            if (cls[i] == 2u) continue;
            const f3 C = make_f3(lr.sph[i].x, lr.sph[i].y, lr.sph[i].z);
            float t;
            if (!intersect_sphere(o, d, 0.0f, kInf, C, lr.sph[i].w, t)) continue;
            bool ok = true;
            while (cls[i] == 1u && !crossing_is_opaque(i, C, o, d, t)) {
                float t2;
                if (!intersect_sphere(o, d, t, kInf, C, lr.sph[i].w, t2)) { ok = false; break; }
                t = t2;
            }
            if (ok && t < best) { best = t; best_id = i; }
        }
        t_out = best; id_out = best_id;
    }
};

template <uint32_t kMode, typename TraceFn>
inline void rm_launch1(const RiBuffers& b, const RiScene& sc, const RiParamsEx& P, TraceFn&& trace)
{
    for (uint32_t by = 0; by < (b.h + 7u) / 8u; by++)
        for (uint32_t bx = 0; bx < (b.w + 7u) / 8u; bx++) {
            if (P.brdf_samples) ri_pass1_block<kMode, true>(b, sc, P, bx, by, trace);
            else ri_pass1_block<kMode, false>(b, sc, P, bx, by, trace);
        }
}

// One pt_restir_di_ex call over caller-owned history arrays.  prm, fprm, ptrs: as ri_host_call (restir_host.cpp); sprm, cell_size: as
// lr_host_call (lightris_host.cpp); cprm = {BrdfSamples, EnableBoilingFilter}, strength = BoilingFilterStrength.
inline void rm_call(const RmHostScene& hs, const uint32_t* prm, const float* fprm, void* const* ptrs, const uint32_t* sprm, float cell_size, const uint32_t* cprm,
                    float strength)
{
    if (hs.lr.lights.empty()) return;  // no emitters, nothing is written
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
    RiParamsEx P{};
    P.frame_index = prm[2]; P.initial_samples = prm[3]; P.temporal = prm[4]; P.temporal_bias = prm[5]; P.max_history = prm[6];
    P.spatial = prm[7]; P.spatial_bias = prm[8]; P.spatial_samples = prm[9]; P.history_valid = prm[10];
    P.radius = fprm[0];
    P.cam_pos = make_f3(fprm[1], fprm[2], fprm[3]);
    P.prev_cam_pos = make_f3(fprm[4], fprm[5], fprm[6]);
    P.brdf_samples = cprm[0]; P.boiling_filter = cprm[1]; P.boiling_strength = cprm[1] ? strength : 0.0f;
    RiScene sc{};
    sc.sph = hs.lr.sph.data(); sc.mats = hs.lr.mats.data(); sc.lights = hs.lr.lights.data(); sc.n_lights = (uint32_t)hs.lr.lights.size();
    sc.light_of = hs.light_of.data();

    const uint32_t mode = sprm[0];
    std::vector<float> pyr;
    std::vector<LrEntry> entries;
    if (mode != kLrUniform) {
        LrGrid g{};
        g.tile_size = sprm[1]; g.tile_count = sprm[2]; g.grid = sprm[3]; g.lights_per_cell = sprm[4]; g.build_samples = sprm[5];
        g.cell_size = cell_size;
        g.cam = P.cam_pos;
        std::vector<float> powers(sc.n_lights);
        for (uint32_t j = 0; j < sc.n_lights; j++) powers[j] = lr_light_power(sc.sph, sc.mats, sc.lights, j);
        pyr.resize(lr_pyramid_floats(lr_levels(sc.n_lights)));
        lr_host_build_pyramid(powers.data(), sc.n_lights, pyr.data());
        const size_t n_power = (size_t)g.tile_size * g.tile_count;
        entries.resize(n_power + (mode == kLrRegirRis ? (size_t)g.grid * g.grid * g.grid * g.lights_per_cell : 0u));
        lr_host_build_power(pyr.data(), sc.n_lights, g.tile_size, g.tile_count, P.frame_index, entries.data());
        if (mode == kLrRegirRis) lr_host_build_regir(hs.lr, g, entries.data(), P.frame_index, entries.data() + n_power);
        sc.lr.ris = entries.data();
        sc.lr.tile_size = g.tile_size; sc.lr.tile_count = g.tile_count; sc.lr.grid = g.grid; sc.lr.lights_per_cell = g.lights_per_cell; sc.lr.cell_size = g.cell_size;
        sc.pyramid = pyr.data();
        sc.pyramid_levels = lr_levels(sc.n_lights);
    }
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { hs.trace(o, d, t, id); };
    auto emit = [&](uint32_t id, f3 o, f3 d, float t) {
        return hs.tex ? hit_material_at<true>(hs.lr.sph.data(), hs.lr.mats.data(), hs.views.data(), hs.tex_maps.data(), hs.rots.data(), id, o, d, t, false).emission
                      : hit_material_at<false>(hs.lr.sph.data(), hs.lr.mats.data(), nullptr, nullptr, nullptr, id, o, d, t, false).emission;
    };
    if (prm[11] & 1u) {
        if (!P.brdf_samples && !P.boiling_filter) {  // both off: the launch of rows N10 / N16, lane by lane
            for (uint32_t y = 0; y < b.h; y++)
                for (uint32_t x = 0; x < b.w; x++) {
                    if (mode == kLrPowerRis) ri_pass1_px<kLrPowerRis>(b, sc, P, x, y, trace);
                    else if (mode == kLrRegirRis) ri_pass1_px<kLrRegirRis>(b, sc, P, x, y, trace);
                    else ri_pass1_px(b, sc, P, x, y, trace);
                }
        } else if (mode == kLrPowerRis) rm_launch1<kLrPowerRis>(b, sc, P, trace);
        else if (mode == kLrRegirRis) rm_launch1<kLrRegirRis>(b, sc, P, trace);
        else rm_launch1<kLrUniform>(b, sc, P, trace);
    }
    if (prm[11] & 2u)
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) ri_pass2_px(b, sc, P, x, y, trace, emit);
}
