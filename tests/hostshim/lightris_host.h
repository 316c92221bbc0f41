// lightris_host.h -- TEST SHIM: the host side of spec S22 over the product's headers, shared by lightris_host.cpp (the tests' library)
// and tests/cpp/lightris_sanitize.cpp (the same code under ASan + UBSan): the scene as pt_set_scene converts it, a brute-force closest
// hit, and the three structures built element by element with the header's functions, in the order the kernels of pt_lightris.hip
// fill them.  Not part of the product.
#pragma once

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_surface.h"
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_lightris.h"
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_restir.h"
#include "../../include/pt_types.h"
#include <cstring>
#include <vector>

using namespace pt;

struct LrHostScene {
    std::vector<float4> sph, mats;
    std::vector<uint32_t> lights, cls;  // cls: 0 visible, 2 invisible (an untextured scene has no per-crossing test)

    void set(const PtSphere* spheres, const PtMaterial* materials, uint32_t n)
    {
        sph.resize(n);
        mats.resize(4 * (size_t)n);
        if (spheres) std::memcpy(sph.data(), spheres, (size_t)n * sizeof(float4));
        cls.assign(n, 0u);
        lights.clear();
        for (uint32_t i = 0; i < n; i++) {
            PtMaterial m = materials[i];
            const float f0d = dielectric_f0(m.IOR), inv_ior = 1.0f / m.IOR;
            std::memcpy(&m._pad[0], &f0d, 4);
            std::memcpy(&m._pad[1], &inv_ior, 4);
            m.AlphaMode &= ~kMaterialHasMaps;
            std::memcpy(&mats[4 * (size_t)i], &m, sizeof m);
            if (m.EmissiveStrength * m.EmissiveColor[0] > 0.0f || m.EmissiveStrength * m.EmissiveColor[1] > 0.0f || m.EmissiveStrength * m.EmissiveColor[2] > 0.0f)
                lights.push_back(i);
            if (materials[i].AlphaMode != PT_ALPHA_OPAQUE) cls[i] = materials[i].BaseColor[3] >= materials[i].AlphaCutoff ? 0u : 2u;
        }
    }

    void trace(f3 o, f3 d, float& t_out, uint32_t& id_out) const
    {
        float best = kInf;
        uint32_t best_id = kRiNoHit;
        for (uint32_t i = 0; i < (uint32_t)sph.size(); i++) {
            if (cls[i] == 2u) continue;
            float t;
            if (!intersect_sphere(o, d, 0.0f, kInf, make_f3(sph[i].x, sph[i].y, sph[i].z), sph[i].w, t)) continue;
            if (t < best) { best = t; best_id = i; }
        }
        t_out = best; id_out = best_id;
    }
};

// every level from the leaves up (leaf j = powers[j], padding 0)
inline void lr_host_build_pyramid(const float* powers, uint32_t n_lights, float* pyramid)
{
    const uint32_t lv = lr_levels(n_lights);
    for (uint32_t j = 0; j < lr_level_size(lv, 0); j++) pyramid[j] = j < n_lights ? powers[j] : 0.0f;
    for (uint32_t k = 0; k < lv; k++) {
        const float* q = pyramid + lr_level_offset(lv, k);
        float* up = pyramid + lr_level_offset(lv, k + 1u);
        for (uint32_t i = 0; i < lr_level_size(lv, k + 1u); i++) up[i] = lr_parent(q[4u * i], q[4u * i + 1u], q[4u * i + 2u], q[4u * i + 3u]);
    }
}

inline void lr_host_build_power(const float* pyramid, uint32_t n_lights, uint32_t tile_size, uint32_t tile_count, uint32_t frame_index, LrEntry* out)
{
    const uint32_t lv = lr_levels(n_lights);
    for (uint32_t t = 0; t < tile_count; t++)
        for (uint32_t s = 0; s < tile_size; s++)
            out[(size_t)t * tile_size + s] = lr_power_entry(lv, t, s, frame_index, [&](uint32_t level, uint32_t node) {
                const float* q = pyramid + lr_level_offset(lv, level) + 4u * node;
                float4 v;
                v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
                return v;
            });
}

inline void lr_host_build_regir(const LrHostScene& hs, const LrGrid& g, const LrEntry* power, uint32_t frame_index, LrEntry* out)
{
    const uint32_t n = g.grid * g.grid * g.grid * g.lights_per_cell;
    for (uint32_t s = 0; s < n; s++) {
        const LrEntry* tile = power + (size_t)lr_regir_tile(s, frame_index, g.tile_count) * g.tile_size;
        out[s] = lr_regir_entry(g, hs.sph.data(), hs.mats.data(), hs.lights.data(), s, frame_index, [&](uint32_t i) { return tile[i]; });
    }
}
