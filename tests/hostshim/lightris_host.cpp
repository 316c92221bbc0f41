// lightris_host.cpp -- TEST SHIM: compiles the product's presampling header (csrc/pt_lightris.h) and the reservoir-pass header that
// consumes it (csrc/pt_restir.h) as plain host C++ (the flags of restir_host.cpp), so the tests can check spec S22 against its float64
// restatement without a GPU, and the GPU kernels against it bit for bit.  Untextured scenes only; the scene arrives as the C-ABI
// receives it and is converted the way pt_set_scene converts it; the visibility query is a brute-force closest hit (nearest t, ties ->
// lowest id), which the device walkers equal bit for bit.  Not part of the product; never loaded by it.
#include "lightris_host.h"

extern "C" {

// the emitter list of pt_set_scene -> its length; lights may be null
uint32_t lr_host_lights(const PtMaterial* materials, uint32_t n, uint32_t* lights)
{
    LrHostScene hs;
    hs.set(nullptr, materials, n);
    if (lights) std::memcpy(lights, hs.lights.data(), hs.lights.size() * sizeof(uint32_t));
    return (uint32_t)hs.lights.size();
}

uint32_t lr_host_levels(uint32_t n_lights) { return lr_levels(n_lights); }
uint32_t lr_host_pyramid_floats(uint32_t n_lights) { return lr_pyramid_floats(lr_levels(n_lights)); }
uint32_t lr_host_level_offset(uint32_t lv, uint32_t k) { return lr_level_offset(lv, k); }

// powers[n_lights] (any floats: the tests feed synthetic powers as well as a scene's) -> the pyramid, every level
void lr_host_pyramid_from_powers(const float* powers, uint32_t n_lights, float* pyramid) { lr_host_build_pyramid(powers, n_lights, pyramid); }

// the emitters' powers of a scene
void lr_host_powers(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, float* powers)
{
    LrHostScene hs;
    hs.set(spheres, materials, n);
    for (uint32_t j = 0; j < (uint32_t)hs.lights.size(); j++) powers[j] = lr_light_power(hs.sph.data(), hs.mats.data(), hs.lights.data(), j);
}

// the Power segment: tile_count * tile_size entries
void lr_host_power_segment(const float* pyramid, uint32_t n_lights, uint32_t tile_size, uint32_t tile_count, uint32_t frame_index, LrEntry* out)
{
    lr_host_build_power(pyramid, n_lights, tile_size, tile_count, frame_index, out);
}

// the ReGIR segment over a Power segment: grid^3 * lights_per_cell entries.  iprm = {grid, lights_per_cell, build_samples, tile_size,
// tile_count, frame_index}; fprm = {cell_size, cam[3]}
void lr_host_regir_segment(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const LrEntry* power, const uint32_t* iprm, const float* fprm, LrEntry* out)
{
    LrHostScene hs;
    hs.set(spheres, materials, n);
    LrGrid g{};
    g.grid = iprm[0]; g.lights_per_cell = iprm[1]; g.build_samples = iprm[2]; g.tile_size = iprm[3]; g.tile_count = iprm[4];
    g.cell_size = fprm[0];
    g.cam = make_f3(fprm[1], fprm[2], fprm[3]);
    lr_host_build_regir(hs, g, power, iprm[5], out);
}

float lr_host_volume_target(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, uint32_t j, const float centre[3], float cell_size)
{
    LrHostScene hs;
    hs.set(spheres, materials, n);
    return lr_volume_target(hs.sph.data(), hs.mats.data(), hs.lights.data(), j, make_f3(centre[0], centre[1], centre[2]), cell_size);
}

void lr_host_cell_centre(const float cam[3], uint32_t grid, float cell_size, uint32_t cell, float out[3])
{
    LrGrid g{};
    g.cam = make_f3(cam[0], cam[1], cam[2]); g.grid = grid; g.cell_size = cell_size;
    const f3 c = lr_cell_centre(g, cell);
    out[0] = c.x; out[1] = c.y; out[2] = c.z;
}

// -> the cell, or 0xFFFFFFFF outside the grid
uint32_t lr_host_cell_of(const float P[3], const float xi[3], const float cam[3], uint32_t grid, float cell_size)
{
    uint32_t cell = 0;
    return lr_cell_of(make_f3(P[0], P[1], P[2]), make_f3(xi[0], xi[1], xi[2]), make_f3(cam[0], cam[1], cam[2]), grid, cell_size, cell) ? cell : 0xFFFFFFFFu;
}

// One pt_restir_di_sampled call over caller-owned history arrays: prm, fprm, ptrs as ri_host_call (restir_host.cpp); sprm = {Mode,
// tile_size, tile_count, grid, lights_per_cell, build_samples} with the defaults already applied, cell_size likewise.  pyramid / ris: null,
// or arrays that receive what the call built (lr_host_pyramid_floats floats; the Power segment then, in mode 2, the ReGIR segment).
void lr_host_call(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const uint32_t* prm, const float* fprm, void* const* ptrs, const uint32_t* sprm,
                  float cell_size, float* pyramid, LrEntry* ris)
{
    LrHostScene hs;
    hs.set(spheres, materials, n);
    if (hs.lights.empty()) return;  // no emitters, nothing is written
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

    // the host side of the call: pyramid -> Power segment -> ReGIR segment (mode 2)
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
        if (mode == kLrRegirRis) lr_host_build_regir(hs, g, entries.data(), P.frame_index, entries.data() + n_power);
        if (pyramid) std::memcpy(pyramid, pyr.data(), pyr.size() * sizeof(float));
        if (ris) std::memcpy(ris, entries.data(), entries.size() * sizeof(LrEntry));
        sc.lr.ris = entries.data();
        sc.lr.tile_size = g.tile_size; sc.lr.tile_count = g.tile_count; sc.lr.grid = g.grid; sc.lr.lights_per_cell = g.lights_per_cell; sc.lr.cell_size = g.cell_size;
    }
    auto trace = [&](f3 o, f3 d, float& t, uint32_t& id) { hs.trace(o, d, t, id); };
    auto emit = [&](uint32_t id, f3 o, f3 d, float t) { return hit_material_at<false>(hs.sph.data(), hs.mats.data(), nullptr, nullptr, nullptr, id, o, d, t, false).emission; };
    // what each lane of pt_restir.hip does, one launch after the other
    if (prm[11] & 1u)
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) {
                if (mode == kLrPowerRis) ri_pass1_px<kLrPowerRis>(b, sc, P, x, y, trace);
                else if (mode == kLrRegirRis) ri_pass1_px<kLrRegirRis>(b, sc, P, x, y, trace);
                else ri_pass1_px(b, sc, P, x, y, trace);
            }
    if (prm[11] & 2u)
        for (uint32_t y = 0; y < b.h; y++)
            for (uint32_t x = 0; x < b.w; x++) ri_pass2_px(b, sc, P, x, y, trace, emit);
}

}  // extern "C"
