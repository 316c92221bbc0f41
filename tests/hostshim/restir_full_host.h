// restir_full_host.h -- TEST SHIM: the host side of spec S26 (pt_restir_di_full, row N22) over the product's headers, shared by
// restir_full_host.cpp (the tests' library) and restir_full_sanitize.cpp (the same code under ASan + UBSan).  The scene, the
// brute-force visibility query and the presampled structures are restir_mis_host.h's; the choice of launches is the entry point's
// (csrc/pt_api_side.hip): the new launch 1 where the word is read or temporal resampling is pairwise, the new launch 2 where the spatial
// pass is pairwise or final shading reuses the word, otherwise the launches of rows N10 / N16 / N17.  Not part of the product.
#pragma once

#include "restir_mis_host.h"

// what a call counted: rays[0] launch 1's, rays[1] the spatial pass's, rays[2] final shading's; rays[3]: final-shading pixels that cast none
struct RfCounters {
    uint64_t rays[4];
};

template <uint32_t kMode, typename TraceFn>
inline void rf_launch1(const RiBuffers& b, const RiScene& sc, const RiParamsFull& P, TraceFn&& trace)
{
    const bool pairwise = P.temporal_bias == kRiBiasPairwise;
    for (uint32_t by = 0; by < (b.h + 7u) / 8u; by++)
        for (uint32_t bx = 0; bx < (b.w + 7u) / 8u; bx++) {
            if (P.brdf_samples && pairwise) ri_pass1_full_block<kMode, true, true>(b, sc, P, bx, by, trace);
            else if (P.brdf_samples) ri_pass1_full_block<kMode, true, false>(b, sc, P, bx, by, trace);
            else if (pairwise) ri_pass1_full_block<kMode, false, true>(b, sc, P, bx, by, trace);
            else ri_pass1_full_block<kMode, false, false>(b, sc, P, bx, by, trace);
        }
}

// One pt_restir_di_full call over caller-owned history arrays.  prm, fprm, ptrs, sprm, cell_size, cprm, strength: as rm_call; shprm =
// {ReuseFinalVisibility, FinalVisibilityMaxAge}, max_distance = FinalVisibilityMaxDistance; prm[11] bit 2: the spatial pass alone, as
// ri_host_call (restir_host.cpp) writes it.  counters may be null.
inline void rf_call(const RmHostScene& hs, const uint32_t* prm, const float* fprm, void* const* ptrs, const uint32_t* sprm, float cell_size, const uint32_t* cprm,
                    float strength, const uint32_t* shprm, float max_distance, RfCounters* counters)
{
    if (counters) *counters = RfCounters{};
    if (hs.lr.lights.empty()) return;
    const bool reuse = shprm[0] != 0;
    const bool full1 = reuse || (prm[4] && prm[5] == kRiBiasPairwise), full2 = reuse || (prm[7] && prm[8] == kRiBiasPairwise);
    uint32_t step[12];
    std::memcpy(step, prm, sizeof step);
    if (!full1 && (prm[11] & 1u)) {  // the launch 1 of rows N10 / N16 / N17
        step[11] = 1u;
        rm_call(hs, step, fprm, ptrs, sprm, cell_size, cprm, strength);
    }
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
    RiParamsFull P{};
    P.frame_index = prm[2]; P.initial_samples = prm[3]; P.temporal = prm[4]; P.temporal_bias = prm[5]; P.max_history = prm[6];
    P.spatial = prm[7]; P.spatial_bias = prm[8]; P.spatial_samples = prm[9]; P.history_valid = prm[10];
    P.radius = fprm[0];
    P.cam_pos = make_f3(fprm[1], fprm[2], fprm[3]);
    P.prev_cam_pos = make_f3(fprm[4], fprm[5], fprm[6]);
    P.brdf_samples = cprm[0]; P.boiling_filter = cprm[1]; P.boiling_strength = cprm[1] ? strength : 0.0f;
    if (reuse) { P.sh.reuse = 1u; P.sh.max_age = shprm[1]; P.sh.max_dist2 = max_distance * max_distance; }
    RiScene sc{};
    sc.sph = hs.lr.sph.data(); sc.mats = hs.lr.mats.data(); sc.lights = hs.lr.lights.data(); sc.n_lights = (uint32_t)hs.lr.lights.size();
    sc.light_of = hs.light_of.data();
    sc.alpha_class = hs.cls.data();

    const uint32_t mode = sprm[0];
    std::vector<float> pyr;
    std::vector<LrEntry> entries;
    if (mode != kLrUniform && full1 && (prm[11] & 1u)) {
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
    uint64_t* count = nullptr;
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) {
        if (count) ++*count;
        hs.trace(o, d, t, id);
    };
    auto emit = [&](uint32_t id, f3 o, f3 d, float t) {
        return hs.tex ? hit_material_at<true>(hs.lr.sph.data(), hs.lr.mats.data(), hs.views.data(), hs.tex_maps.data(), hs.rots.data(), id, o, d, t, false).emission
                      : hit_material_at<false>(hs.lr.sph.data(), hs.lr.mats.data(), nullptr, nullptr, nullptr, id, o, d, t, false).emission;
    };
    if (full1 && (prm[11] & 1u)) {
        count = counters ? &counters->rays[0] : nullptr;
        if (mode == kLrPowerRis) rf_launch1<kLrPowerRis>(b, sc, P, trace);
        else if (mode == kLrRegirRis) rf_launch1<kLrRegirRis>(b, sc, P, trace);
        else rf_launch1<kLrUniform>(b, sc, P, trace);
    }
    // launch 2, and the spatial pass alone: the spatial and the final step of ri_pass2_full_px / ri_pass2_px with a counter each
    const bool pairwise = P.spatial_bias == kRiBiasPairwise;
    float4* const planes[2] = { b.out_diffuse, b.out_specular };
    if (prm[11] & 6u)
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) {
                const uint32_t i = y * b.w + x;
                const RiRecord rec = ri_load_record(b.rec, b.rec_t, i);
                if (!is_finite(rec.r3.z)) continue;
                const RiSurface s = ri_surface(rec, P.cam_pos);
                const RiReservoir centre = ri_load_reservoir(b.res, i);
                count = counters ? &counters->rays[1] : nullptr;
                const RiReservoir r = !full2 ? ri_spatial(b, sc, P, s, centre, x, y, trace)
                                             : (pairwise ? ri_spatial_pairwise(b, sc, P, s, centre, x, y) : ri_spatial<true>(b, sc, P, s, centre, x, y, trace));
                if (prm[11] & 4u) { ri_store_reservoir(planes, i, r); continue; }
                count = counters ? &counters->rays[2] : nullptr;
                const uint64_t before = counters ? counters->rays[2] : 0u;
                float4 d, sp;
                const bool lit = reuse ? ri_final_reuse(sc, P.sh, s, r, trace, emit, d, sp) : ri_final(sc, s, r, trace, emit, d, sp);
                if (lit) { b.out_diffuse[i] = d; b.out_specular[i] = sp; }
                if (counters && lit && counters->rays[2] == before) counters->rays[3]++;
            }
}
