// pt_lightris.h -- the local-light presampling of row N16 (pt_restir_di_sampled, DESIGN.md spec S22): a stand-in for what the reference
// runs in front of RTXDI's DI passes (LightPreparation.hlsl and MipmapGeneration.hlsl every frame, LocalLightPresampling.hlsl and
// ReGIRPresampling.hlsl in RTXDI::Render).  Three structures, rebuilt by every call from the lane's own spheres:
//   the power pyramid   every level in Z-curve (Morton) linear order, so a 2x2 texel quad is one aligned float4; leaf j = power of
//                       emitter j, a parent = (((q0 + q1) + q2) + q3) * 0.25 -- the reference's PDF texture and its mip chain up to
//                       addressing (RTXDI_LinearIndexToZCurve disappears)
//   the Power_RIS tiles TileCount x TileSize entries {emitter, 1 / pdf}, each a walk down the pyramid
//   the ReGIR grid      G^3 cells x LightsPerCell entries, each a RIS over BuildSamples entries of one Power_RIS tile against the
//                       cell's volume target (CalculateWeightForVolume's sphere form, Light.hlsli:85-95)
// Per-element functions that compile on the device (pt_lightris.hip; the candidate source of pt_restir.h's ri_initial) and as host
// C++ (the bit-parity tests).  fp32, no contraction.  The RTXDI SDK is a submodule the reference tree does not contain: where only
// the SDK had the code the arithmetic is written from recollection and frozen here.
//
// Out of scope: the onion mode of ReGIR, the cell visualisation, BRDF and environment candidates, the compact-light-info path (the
// reference's bridge returns false from it, RTXDIAppBridge.hlsli:213-221).
#pragma once

#include "pt_light.h"

namespace pt {

constexpr uint32_t kLrPowerRngSalt = 0x4C525031u;      // Power_RIS entry (tile t, slot s): rng_init(s, t, FrameIndex ^ salt)
constexpr uint32_t kLrRegirRngSalt = 0x4C525231u;      // ReGIR slot g: rng_init(g & 0xfff, g >> 12, FrameIndex ^ salt)
constexpr uint32_t kLrRegirTileRngSalt = 0x4C525431u;  // ... and the tile of 256 consecutive slots: rng_init(g >> 8, 0, FrameIndex ^ salt)
constexpr uint32_t kLrPixelTileRngSalt = 0x4C525831u;  // initial sampling, the tile of a 16x16 pixel block: rng_init(px >> 4, py >> 4, ...)
constexpr uint32_t kLrInvalid = 0xFFFFFFFFu;
enum : uint32_t { kLrUniform = 0, kLrPowerRis = 1, kLrRegirRis = 2 };
constexpr uint32_t kLrDefaultTileSize = 1024, kLrMaxTileSize = 8192, kLrDefaultTileCount = 128, kLrMaxTileCount = 1024, kLrDefaultGrid = 16,
                   kLrMaxGrid = 32, kLrDefaultLightsPerCell = 512, kLrMaxLightsPerCell = 1024, kLrDefaultBuildSamples = 8, kLrMaxBuildSamples = 32,
                   kLrMaxEntries = 1u << 24;
constexpr float kLrDefaultCellSize = 1.0f, kLrMinCellSize = 0.1f, kLrMaxCellSize = 10.0f;
constexpr uint32_t kLrGroupLeaves = 1024, kLrGroupLevels = 5;  // what one workgroup of the pyramid kernel reduces

struct alignas(8) LrEntry {
    uint32_t light;  // index into the emitter list; kLrInvalid: the entry carries nothing
    float inv_pdf;   // 1 / (source pdf of `light`)
};

// what ri_initial reads; all zero = Uniform
struct LrView {
    const LrEntry* ris;  // the Power segment (tile_count * tile_size entries), then the ReGIR segment (grid^3 * lights_per_cell)
    uint32_t tile_size, tile_count, grid, lights_per_cell;
    float cell_size;
};

// ---- the pyramid
PT_HD uint32_t lr_levels(uint32_t n_lights)  // smallest Lv with 4^Lv >= n_lights
{
    uint32_t lv = 0;
    while (lv < 16u && (1ull << (2u * lv)) < (unsigned long long)n_lights) lv++;
    return lv;
}
PT_HD uint32_t lr_level_size(uint32_t lv, uint32_t k) { return 1u << (2u * (lv - k)); }
PT_HD uint32_t lr_level_offset(uint32_t lv, uint32_t k)  // floats in front of level k (level 0 = the leaves)
{
    uint32_t off = 0;
    for (uint32_t i = 0; i < k; i++) off += lr_level_size(lv, i);
    return off;
}
PT_HD uint32_t lr_pyramid_floats(uint32_t lv) { return lr_level_offset(lv, lv) + 1u; }

// TriangleLight::CalculatePower without its constant factor pi area / r^2 (only ratios are used): r^2 luminance(Le), Le the untextured
// radiance ri_shade uses
PT_HD float lr_light_power(const float4* sph, const float4* mats, const uint32_t* lights, uint32_t j)
{
    const uint32_t id = lights[j];
    const float r = sph[id].w;
    const float4 lm = mats[id * 4u + 1u];  // {EmissiveStrength, EmissiveColor}
    const float p = (r * r) * luminance(make_f3(lm.y, lm.z, lm.w) * lm.x);
    return p > 0.0f && is_finite(p) ? p : 0.0f;
}

PT_HD float lr_quad_sum(float q0, float q1, float q2, float q3) { return ((q0 + q1) + q2) + q3; }
PT_HD float lr_parent(float q0, float q1, float q2, float q3) { return lr_quad_sum(q0, q1, q2, q3) * 0.25f; }

// ---- Power_RIS entry (tile t, slot s): quad(level, node) = the four children of `node`, entries 4 node .. 4 node + 3 of `level`
template <typename QuadFn>
PT_HD LrEntry lr_power_entry(uint32_t lv, uint32_t t, uint32_t s, uint32_t frame_index, QuadFn&& quad)
{
    uint32_t rng = rng_init(s, t, frame_index ^ kLrPowerRngSalt);
    uint32_t node = 0u;
    float pdf = 1.0f;
    LrEntry e;
    for (uint32_t level = lv; level-- > 0u;) {
        const float4 q = quad(level, node);
        const float sum = lr_quad_sum(q.x, q.y, q.z, q.w);
        if (!(sum > 0.0f)) { e.light = kLrInvalid; e.inv_pdf = 0.0f; return e; }
        const float u = rng_float(rng) * sum;
        const float p0 = q.x, p1 = q.x + q.y, p2 = p1 + q.z;  // (the fourth prefix is bitwise `sum`: a zero-weight child is never chosen)
        const uint32_t k = p0 >= u ? 0u : (p1 >= u ? 1u : (p2 >= u ? 2u : 3u));
        const float qk = k == 0u ? q.x : (k == 1u ? q.y : (k == 2u ? q.z : q.w));
        pdf *= qk / sum;
        node = 4u * node + k;
    }
    e.light = node;
    e.inv_pdf = 1.0f / pdf;
    return e;
}

// ---- ReGIR
struct LrGrid {
    f3 cam;             // PtCamera.Position: the grid's centre (App.cpp:1081)
    uint32_t grid;      // cells per axis
    float cell_size;
    uint32_t lights_per_cell, build_samples, tile_size, tile_count;
};

PT_HD f3 lr_cell_centre(const LrGrid& g, uint32_t cell)
{
    const uint32_t ix = cell % g.grid, iy = (cell / g.grid) % g.grid, iz = cell / (g.grid * g.grid);
    const float half = 0.5f * (float)g.grid;
    return make_f3(g.cam.x + (((float)ix + 0.5f) - half) * g.cell_size, g.cam.y + (((float)iy + 0.5f) - half) * g.cell_size,
                   g.cam.z + (((float)iz + 0.5f) - half) * g.cell_size);
}

// CalculateWeightForVolume, sphere form (Light.hlsli:85-95, the distance of Light.hlsli:16-23), without the normal cull: the volume's
// radius is the half diagonal of a cell widened by the lookup jitter
PT_HD float lr_volume_target(const float4* sph, const float4* mats, const uint32_t* lights, uint32_t j, f3 centre, float cell_size)
{
    const uint32_t id = lights[j];
    const float4 ls = sph[id];
    const float4 lm = mats[id * 4u + 1u];
    const float R = 1.7320508f * cell_size;
    const f3 v = make_f3(ls.x, ls.y, ls.z) - centre;
    const float d = pt_sqrt(dot(v, v));
    const float den = d + 1.1547f * R;
    const float dist = d + ((R * R) * R) / (den * den);
    const float solid = pt_min((kPi * (ls.w * ls.w)) / (dist * dist), 2.0f * kPi);
    const float t = solid * luminance(make_f3(lm.y, lm.z, lm.w) * lm.x);
    return t > 0.0f && is_finite(t) ? t : 0.0f;
}

// the Power_RIS tile that the 256 consecutive slots around g draw from (ReGIRPresampling.hlsl:8-10)
PT_HD uint32_t lr_regir_tile(uint32_t g, uint32_t frame_index, uint32_t tile_count)
{
    uint32_t rng = rng_init(g >> 8, 0u, frame_index ^ kLrRegirTileRngSalt);
    return pick_light(rng_float(rng), tile_count);
}

// slot g of the ReGIR segment: tile(i) = entry i of the slot's Power_RIS tile
template <typename TileFn>
PT_HD LrEntry lr_regir_entry(const LrGrid& gr, const float4* sph, const float4* mats, const uint32_t* lights, uint32_t g, uint32_t frame_index, TileFn&& tile)
{
    const f3 centre = lr_cell_centre(gr, g / gr.lights_per_cell);
    uint32_t rng = rng_init(g & 0xfffu, g >> 12, frame_index ^ kLrRegirRngSalt);
    float w_sum = 0.0f, sel_target = 0.0f;
    uint32_t sel = kLrInvalid;
    for (uint32_t i = 0; i < gr.build_samples; i++) {
        const float u = rng_float(rng), rnd = rng_float(rng);
        const LrEntry c = tile(pick_light(u, gr.tile_size));
        float target = 0.0f, w = 0.0f;
        if (c.light != kLrInvalid) {
            target = lr_volume_target(sph, mats, lights, c.light, centre, gr.cell_size);
            w = target * c.inv_pdf;
        }
        w_sum += w;
        if (w > 0.0f && rnd * w_sum <= w) { sel = c.light; sel_target = target; }
    }
    LrEntry e;
    e.light = kLrInvalid; e.inv_pdf = 0.0f;
    if (sel != kLrInvalid) {
        const float inv = w_sum / ((float)gr.build_samples * sel_target);
        if (inv > 0.0f && is_finite(inv)) { e.light = sel; e.inv_pdf = inv; }
    }
    return e;
}

// ---- initial sampling's lookups
// the tile of the 16x16 pixel block of (px, py)
PT_HD uint32_t lr_pixel_tile(uint32_t px, uint32_t py, uint32_t frame_index, uint32_t tile_count)
{
    uint32_t rng = rng_init(px >> 4, py >> 4, frame_index ^ kLrPixelTileRngSalt);
    return pick_light(rng_float(rng), tile_count);
}

// the cell of the jittered point P' = P + (xi - 0.5) cell_size; false: outside the grid (the pixel uses the Power_RIS path)
PT_HD bool lr_cell_of(f3 P, f3 xi, f3 cam, uint32_t grid, float cell_size, uint32_t& cell)
{
    const float half = 0.5f * (float)grid, G = (float)grid;
    const float cx = pt_floor(((P.x + (xi.x - 0.5f) * cell_size) - cam.x) / cell_size + half);
    const float cy = pt_floor(((P.y + (xi.y - 0.5f) * cell_size) - cam.y) / cell_size + half);
    const float cz = pt_floor(((P.z + (xi.z - 0.5f) * cell_size) - cam.z) / cell_size + half);
    if (!(cx >= 0.0f && cx < G && cy >= 0.0f && cy < G && cz >= 0.0f && cz < G)) return false;
    cell = ((uint32_t)cz * grid + (uint32_t)cy) * grid + (uint32_t)cx;
    return true;
}

#if defined(__HIPCC__)
// what a call builds, on `stream`: the pyramid (every level), the Power segment, and in ReGIR mode the ReGIR segment behind it
struct LrBuild {
    const float4* sph;       // the lane's spheres, original order
    const float4* mats;
    const uint32_t* lights;
    uint32_t n_lights, frame_index;
    float* pyramid;          // lr_pyramid_floats(lr_levels(n_lights)) floats
    LrEntry* ris;
    LrGrid grid;             // grid.grid = 0: no ReGIR segment
};
hipError_t launch_lr_pyramid(const LrBuild& b, hipStream_t stream);
hipError_t launch_lr_power(const LrBuild& b, hipStream_t stream);
hipError_t launch_lr_regir(const LrBuild& b, hipStream_t stream);
#endif

}  // namespace pt
