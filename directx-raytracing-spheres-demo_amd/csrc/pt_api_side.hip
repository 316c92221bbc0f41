// pt_api_side.hip -- the entry points of the C-ABI (include/pt_api.h) that are side passes of a frame: work for the frame the NEXT render call renders,
// queued on the lane that frame will take and ordered against the caller's stream like the frame itself (pt_lane_order.h, side_pass_begin): the G-buffer pass,
// the reservoir pass, the frame through the radiance cache, the frame through the thin-lens camera and the frame from G-buffer texels, with their downloads.  The frames and the shared helpers (end of pt_context.h) are in pt_api.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_context.h"
#include "pt_restir.h"
#include "pt_lightris.h"
#include "pt_sharc.h"
#include "pt_lens.h"
#include "pt_gbframe.h"

// Row N6 -- the G-buffer pass of the frame the next pt_render renders, on the lane that frame will use (DESIGN.md spec S12).
// published (pt_render_gbuffer_published, spec S28): the previous pose is the generation published before the newest one, copied on the
// device by the lane's take (lane_catch_up); the two pointers are null.
static PtStatus gbuffer_pass(PtContext* c, const PtRect* rect, void* const* gb13, const PtSphere* previous_spheres, const float* previous_rotations, bool published,
                             bool packed = false)
{
    if (!c) return PT_ERR_INVALID_ARG;
    // packed (pt_render_gbuffer_packed, row N27, spec S30): the same pass stored in the reference's texel formats
    const std::string who = packed ? "pt_render_gbuffer_packed" : "pt_render_gbuffer";
    if (!gb13) return fail(c, PT_ERR_INVALID_ARG, who + (packed ? ": null PtGBufferPacked" : ": null PtGBuffer"));
    // the requested channels; every buffer must be aligned to its channel's vector width (float4: 16 B, float2: 8 B, else 4 B), a packed one to its texel
    void* const* ptrs = gb13;
    const uint32_t align_f32[13] = { 16, 8, 8, 4, 4, 4, 16, 4, 4, 16, 4, 4, 4 };
    const uint32_t* align = packed ? kGbPackedTexelBytes : align_f32;
    uint32_t want = 0;
    for (uint32_t k = 0; k < 13; k++) {
        if (!ptrs[k]) continue;
        if (reinterpret_cast<uintptr_t>(ptrs[k]) % align[k]) return fail(c, PT_ERR_INVALID_ARG, who + ": a buffer is not aligned to its channel's width");
        want |= 1u << k;
    }
    if (!want) return fail(c, PT_ERR_INVALID_ARG, who + ": no output requested (all 13 pointers are NULL)");
    PtStatus st = validate_frame(c);
    if (st != PT_OK) return st;
    PtRect r;
    PixelMap pm{};
    if ((st = rect_pixel_map(c, rect, who.c_str(), r, pm)) != PT_OK) return st;
    if ((st = check_environment(c)) != PT_OK) return st;
    if ((st = check_tree_lds(c)) != PT_OK) return st;
    // previous poses (PreviousObjectToWorld): only while the scene is not static; the empty scene has none
    const uint32_t n = c->empty_scene ? 0u : c->n;
    const bool use_prev_sph = previous_spheres && !c->sd.IsStatic && n > 0, use_prev_rot = previous_rotations && !c->sd.IsStatic && n > 0;
    for (uint32_t i = 0; use_prev_sph && i < n; i++) {
        const PtSphere& p = previous_spheres[i];
        if (!std::isfinite(p.cx) || !std::isfinite(p.cy) || !std::isfinite(p.cz) || !std::isfinite(p.r) || !(p.r > 0.0f))
            return fail(c, PT_ERR_INVALID_ARG, who + ": previous sphere " + std::to_string(i) + " is not finite or has radius <= 0");
    }
    for (uint32_t i = 0; use_prev_rot && i < 4u * n; i++)
        if (!std::isfinite(previous_rotations[i])) return fail(c, PT_ERR_INVALID_ARG, who + ": previous rotation " + std::to_string(i / 4) + " is not finite");
    if (published && n > 0 && !c->pub.order.sph_live)
        return fail(c, PT_ERR_STATE, "pt_render_gbuffer_published: the scene's newest spheres are not a published pose (pt_physics_publish first)");
    PT_HIP(c, hipSetDevice(c->device));

    Lane& L = c->lanes[c->next_lane];  // the lane of the next frame
    // (shared: a buffer is one that another lane's G-buffer call or frame holds within the window, or no frame has been rendered yet)
    c->pub.want_prev = published && !c->sd.IsStatic && n > 0;
    st = side_pass_begin(c, L, ledger_gbuffer({ c->ledgers, c->n_lanes, c->next_lane }, c->calls == 0, ptrs));
    c->pub.want_prev = false;
    if (st != PT_OK) return st;
    const SceneView sv = make_scene_view(c, &L);
    GBufferScene sc{};
    sc.sph = sv.sph; sc.mats = sv.mats; sc.tex = sv.tex; sc.tex_maps = sv.tex_maps; sc.rot = sv.rot;
    sc.is_static = c->sd.IsStatic ? 1u : 0u;
    sc.env_tex = sv.env_tex; sc.env_cube = sv.env_cube;
    for (int k = 0; k < 4; k++) sc.env[k] = sv.env[k];
    for (int k = 0; k < 9; k++) sc.env_xf[k] = sv.env_xf[k];
    if (published) {
        // (the lane's take has put generation g - 1 into d_prev_pose; a first generation has no predecessor: previous = current)
        const bool have = !c->sd.IsStatic && n > 0 && L.pub_prev_gen == c->pub.order.gen && L.pub_prev_valid;
        sc.prev_sph = have ? L.d_prev_pose : nullptr;
        sc.prev_rot = have && c->has_textures ? L.d_prev_pose + n : nullptr;
    } else if (use_prev_sph || use_prev_rot) {
        const bool fresh = L.prev_cap < n;
        if ((st = lane_prev_pose_reserve(c, L, n)) != PT_OK) return st;
        if (!fresh) PT_HIP(c, hipEventSynchronize(L.ev_prev));  // the previous upload from the staging buffer has been consumed
        L.pub_prev_gen = 0;  // (d_prev_pose no longer holds a published generation's predecessor)
        if (use_prev_sph) std::memcpy(L.h_prev_stage, previous_spheres, (size_t)n * sizeof(float4));
        if (use_prev_rot) std::memcpy(L.h_prev_stage + n, previous_rotations, (size_t)n * sizeof(float4));
        PT_HIP(c, hipMemcpyAsync(L.d_prev_pose, L.h_prev_stage, 2u * (size_t)n * sizeof(float4), hipMemcpyHostToDevice, L.stream));
        PT_HIP(c, hipEventRecord(L.ev_prev, L.stream));
        sc.prev_sph = use_prev_sph ? L.d_prev_pose : nullptr;
        sc.prev_rot = use_prev_rot ? L.d_prev_pose + n : nullptr;
    }
    GBufferFrame fr{};
    fr.cam = camera_params(c->cam, c->gs.RenderSize[0], c->gs.RenderSize[1]);
    fr.width = (float)c->gs.RenderSize[0];
    fr.height = (float)c->gs.RenderSize[1];
    fr.reversed = c->cam.IsNormalizedDepthReversed ? 1u : 0u;
    std::memcpy(fr.world_to_projection, c->cam.Matrices[5], sizeof fr.world_to_projection);
    std::memcpy(fr.prev_world_to_projection, c->cam.Matrices[2], sizeof fr.prev_world_to_projection);
    std::memcpy(fr.prev_world_to_view, c->cam.Matrices[0], sizeof fr.prev_world_to_view);
    st = PT_OK;
    hipError_t e;
    if (packed) {
        const GBufferPackedOut out{ static_cast<float4*>(ptrs[0]), static_cast<uint32_t*>(ptrs[1]), static_cast<uint32_t*>(ptrs[2]), static_cast<float*>(ptrs[3]),
                                    static_cast<float*>(ptrs[4]), static_cast<uint64_t*>(ptrs[5]), static_cast<uint32_t*>(ptrs[6]), static_cast<uint64_t*>(ptrs[7]),
                                    static_cast<uint64_t*>(ptrs[8]), static_cast<uint64_t*>(ptrs[9]), static_cast<uint16_t*>(ptrs[10]), static_cast<uint8_t*>(ptrs[11]),
                                    static_cast<uint64_t*>(ptrs[12]) };  // (GBufferPackedOut's members in the order of ptrs)
        e = launch_gbuffer_packed(sv, pm, fr, sc, out, want, side_pass_grid(c, pm.n_slots), L.stream);
    } else {
        const GBufferOut out{ static_cast<float4*>(ptrs[0]), static_cast<float2*>(ptrs[1]), static_cast<float2*>(ptrs[2]), static_cast<float*>(ptrs[3]), static_cast<float*>(ptrs[4]),
                              static_cast<f3*>(ptrs[5]), static_cast<float4*>(ptrs[6]), static_cast<f3*>(ptrs[7]), static_cast<f3*>(ptrs[8]), static_cast<float4*>(ptrs[9]),
                              static_cast<float*>(ptrs[10]), static_cast<float*>(ptrs[11]), static_cast<f3*>(ptrs[12]) };  // (GBufferOut's members in the order of ptrs)
        e = launch_gbuffer(sv, pm, fr, sc, out, want, side_pass_grid(c, pm.n_slots), L.stream);
    }
    if (e != hipSuccess) st = fail(c, PT_ERR_HIP, who + ": launch: " + hipGetErrorString(e));
    return publish_lane_to_caller(c, L, who.c_str(), st);
}

// the 13 pointers of a PtGBuffer / PtGBufferPacked in field order
template <typename G>
static void gbuffer_pointers(const G* gb, void* out[13])
{
    void* const p[13] = { gb->Position, gb->FlatNormal, gb->GeometricNormal, gb->LinearDepth, gb->NormalizedDepth, gb->MotionVector,
                          gb->BaseColorMetalness, gb->DiffuseAlbedo, gb->SpecularAlbedo, gb->NormalRoughness, gb->IOR, gb->Transmission, gb->Radiance };
    std::copy(p, p + 13, out);
}

extern "C" {

PtStatus pt_render_gbuffer(PtContext* c, const PtRect* rect, const PtGBuffer* gb, const PtSphere* previous_spheres, const float* previous_rotations)
{
    void* p[13];
    if (gb) gbuffer_pointers(gb, p);
    return gbuffer_pass(c, rect, gb ? p : nullptr, previous_spheres, previous_rotations, false);
}

// Row N27 -- pt_render_gbuffer into the reference's texel formats (DESIGN.md spec S30)
PtStatus pt_render_gbuffer_packed(PtContext* c, const PtRect* rect, const PtGBufferPacked* gb, const PtSphere* previous_spheres, const float* previous_rotations)
{
    void* p[13];
    if (gb) gbuffer_pointers(gb, p);
    return gbuffer_pass(c, rect, gb ? p : nullptr, previous_spheres, previous_rotations, false, true);
}

// Row N24 -- pt_render_gbuffer with the previous pose taken from the published ring (DESIGN.md spec S28)
PtStatus pt_render_gbuffer_published(PtContext* c, const PtRect* rect, const PtGBuffer* gb)
{
    void* p[13];
    if (gb) gbuffer_pointers(gb, p);
    return gbuffer_pass(c, rect, gb ? p : nullptr, nullptr, nullptr, true);
}

// Row N10 -- the reservoir pass (DESIGN.md spec S16): two launches on the lane of the next render call, ordered like pt_render_gbuffer;
// the history (per pixel and slot: a surface record of four float4 and a float, a reservoir of two float4) lives in the context.
constexpr uint64_t kRiSlotBytesPerPixel = 6 * sizeof(float4) + sizeof(float);

// The body of pt_restir_di, pt_restir_di_sampled (row N16, spec S22), pt_restir_di_ex (row N17, spec S23) and pt_restir_di_full (row N22,
// spec S26); ls null or Mode 0 = Uniform: nothing is presampled; cd null, or no BRDF candidates and the filter off: launch 1 is the one of
// rows N10 / N16.  full: the entry point accepts pairwise bias correction (2) and reads sh; sh null or ReuseFinalVisibility 0 and no mode
// equal to 2: the launches are pt_restir_di_ex's.
static PtStatus restir_di_common(PtContext* c, const char* who, const PtRestirDiSettings* s, const PtLightSamplingSettings* ls, const PtRestirDiCandidates* cd,
                                 const PtRestirDiShading* sh, bool full, const PtRestirDiTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": null pointer");
    const uint32_t w = s->RenderSize[0], h = s->RenderSize[1];
    if (w == 0 || h == 0 || w > 16384u || h > 16384u) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": RenderSize must be in [1, 16384]");
    if (s->InitialSamples > kRiMaxInitialSamples) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": InitialSamples must be at most 32");
    if (s->SpatialSamples > kRiMaxSpatialSamples) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": SpatialSamples must be at most 32");
    if (s->EnableTemporal > 1 || s->EnableSpatial > 1) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": EnableTemporal and EnableSpatial must be 0 or 1");
    for (const uint32_t mode : { s->TemporalBiasCorrection, s->SpatialBiasCorrection }) {
        if (mode == kRiBiasPairwise && !full) return fail(c, PT_ERR_UNSUPPORTED, std::string(who) + ": pairwise bias correction (2) runs through pt_restir_di_full");
        if (mode > kRiBiasRaytraced) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": a bias correction mode must be 0 (Off), 1 (Basic), 2 (Pairwise: pt_restir_di_full) or 3 (Raytraced)");
    }
    if (sh) {
        if (sh->ReuseFinalVisibility > 1) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": ReuseFinalVisibility must be 0 or 1");
        if (sh->FinalVisibilityMaxAge > 255u) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": FinalVisibilityMaxAge must be at most 255");
        if (!std::isfinite(sh->FinalVisibilityMaxDistance) || !(sh->FinalVisibilityMaxDistance >= 0.0f))
            return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": FinalVisibilityMaxDistance must be finite and >= 0");
        if (sh->_pad != 0) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": PtRestirDiShading._pad must be 0");
    }
    if (!std::isfinite(s->SpatialRadius) || !(s->SpatialRadius >= 0.0f)) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": SpatialRadius must be finite and >= 0");
    if (cd) {
        if (cd->BrdfSamples > kRiMaxBrdfSamples) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": BrdfSamples must be at most 8");
        if (cd->EnableBoilingFilter > 1) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": EnableBoilingFilter must be 0 or 1");
        if (cd->EnableBoilingFilter && (!std::isfinite(cd->BoilingFilterStrength) || !(cd->BoilingFilterStrength >= 0.0f && cd->BoilingFilterStrength <= 1.0f)))
            return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": BoilingFilterStrength must be finite and in [0, 1]");
        if (cd->_pad != 0) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": PtRestirDiCandidates._pad must be 0");
    }
    // the candidates' source (spec S22): defaults applied, ranges checked
    const uint32_t mode = ls ? ls->Mode : kLrUniform;
    LrGrid lg{};
    if (mode != kLrUniform) {
        if (mode > kLrRegirRis) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": Mode must be 0 (Uniform), 1 (Power_RIS) or 2 (ReGIR_RIS)");
        if (ls->_pad != 0) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": PtLightSamplingSettings._pad must be 0");
        if (ls->TileSize > kLrMaxTileSize) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": TileSize must be at most 8192");
        if (ls->TileCount > kLrMaxTileCount) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": TileCount must be at most 1024");
        if (ls->ReGIRGridSize > kLrMaxGrid) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": ReGIRGridSize must be at most 32");
        if (ls->ReGIRLightsPerCell > kLrMaxLightsPerCell) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": ReGIRLightsPerCell must be at most 1024");
        if (ls->ReGIRBuildSamples > kLrMaxBuildSamples) return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": ReGIRBuildSamples must be at most 32");
        if (ls->ReGIRCellSize != 0.0f && !(std::isfinite(ls->ReGIRCellSize) && ls->ReGIRCellSize >= kLrMinCellSize && ls->ReGIRCellSize <= kLrMaxCellSize))
            return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": ReGIRCellSize must be 0 or finite and in [0.1, 10]");
        lg.tile_size = ls->TileSize ? ls->TileSize : kLrDefaultTileSize;
        lg.tile_count = ls->TileCount ? ls->TileCount : kLrDefaultTileCount;
        lg.grid = ls->ReGIRGridSize ? ls->ReGIRGridSize : kLrDefaultGrid;
        lg.lights_per_cell = ls->ReGIRLightsPerCell ? ls->ReGIRLightsPerCell : kLrDefaultLightsPerCell;
        lg.build_samples = ls->ReGIRBuildSamples ? ls->ReGIRBuildSamples : kLrDefaultBuildSamples;
        lg.cell_size = ls->ReGIRCellSize != 0.0f ? ls->ReGIRCellSize : kLrDefaultCellSize;
        if ((uint64_t)lg.tile_size * lg.tile_count + (uint64_t)lg.grid * lg.grid * lg.grid * lg.lights_per_cell > kLrMaxEntries)
            return fail(c, PT_ERR_INVALID_ARG, std::string(who) + ": the Power_RIS and ReGIR segments together hold more than 2^24 entries");
    }
    const uint64_t n = (uint64_t)w * h;
    // the eight inputs, then the two outputs
    const BufferUse use[10] = {
        {t->Position, n * 16, 16, false, true, "Position"}, {t->GeometricNormal, n * 8, 8, false, true, "GeometricNormal"},
        {t->LinearDepth, n * 4, 4, false, true, "LinearDepth"}, {t->MotionVector, n * 12, 4, false, true, "MotionVector"},
        {t->BaseColorMetalness, n * 16, 16, false, true, "BaseColorMetalness"}, {t->NormalRoughness, n * 16, 16, false, true, "NormalRoughness"},
        {t->IOR, n * 4, 4, false, true, "IOR"}, {t->Transmission, n * 4, 4, false, true, "Transmission"},
        {t->Diffuse, n * 16, 16, true, true, "Diffuse"}, {t->Specular, n * 16, 16, true, true, "Specular"},
    };
    PtStatus st = buffers_ok(c, who, use, 10);
    if (st != PT_OK) return st;
    if ((st = validate_frame(c)) != PT_OK) return st;
    if ((st = check_environment(c)) != PT_OK) return st;
    if ((st = check_tree_lds(c)) != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    if (c->n_lights == 0 || c->empty_scene) {  // no emitters: nothing is written, and there is no history to keep
        c->ri_valid = false;
        return PT_OK;
    }

    Lane& L = c->lanes[c->next_lane];  // the lane of the next frame
    // (pt_lane_order.h: pt_render_gbuffer's rule, and shared also when an input is not one of this lane's own G-buffer call, or a buffer is another lane's DI output)
    const bool shared = ledger_reservoir({ c->ledgers, c->n_lanes, c->next_lane }, c->calls == 0, [&](int k) { return use[k].p; });
    if ((st = side_pass_begin(c, L, shared)) != PT_OK) return st;
    // the history: the previous call (on whichever lane it ran) wrote the slot this one reads and read the slot this one writes
    bool restart = s->ResetHistory != 0 || !c->ri_valid || c->ri_scene != c->set_scene_calls;
    if (!c->ev_ri) PT_HIP(c, hipEventCreateWithFlags(&c->ev_ri, hipEventDisableTiming));
    if (!c->d_ri || c->ri_w != w || c->ri_h != h) {
        if (c->d_ri) PT_HIP(c, hipEventSynchronize(c->ev_ri));  // (the previous call may still use the old buffers)
        free_dev(c->d_ri);
        c->ri_valid = false;
        void* mem = nullptr;
        if (hipMalloc(&mem, 2u * n * kRiSlotBytesPerPixel) != hipSuccess) { (void)hipGetLastError(); return fail(c, PT_ERR_OOM, std::string(who) + ": history allocation failed"); }
        c->d_ri = static_cast<float4*>(mem);
        c->ri_w = w; c->ri_h = h;
        restart = true;
    } else if (L.stream != c->stream || c->n_lanes > 1) {
        PT_HIP(c, hipStreamWaitEvent(L.stream, c->ev_ri, 0));
    }
    const uint32_t cur = c->ri_slot ^ 1u, prev = c->ri_slot;
    RiBuffers b{};
    b.w = w; b.h = h;
    b.position = static_cast<const float4*>(t->Position);
    b.geometric_normal = static_cast<const float*>(t->GeometricNormal);
    b.linear_depth = static_cast<const float*>(t->LinearDepth);
    b.motion_vector = static_cast<const float*>(t->MotionVector);
    b.base_color_metalness = static_cast<const float4*>(t->BaseColorMetalness);
    b.normal_roughness = static_cast<const float4*>(t->NormalRoughness);
    b.ior = static_cast<const float*>(t->IOR);
    b.transmission = static_cast<const float*>(t->Transmission);
    float4* planes = c->d_ri;                                              // [slot][6 planes][n] float4, then [slot][n] float
    float* tplanes = reinterpret_cast<float*>(c->d_ri + 12u * n);
    for (uint32_t k = 0; k < 4; k++) { b.rec[k] = planes + ((uint64_t)cur * 6u + k) * n; b.prev_rec[k] = planes + ((uint64_t)prev * 6u + k) * n; }
    for (uint32_t k = 0; k < 2; k++) { b.res[k] = planes + ((uint64_t)cur * 6u + 4u + k) * n; b.prev_res[k] = planes + ((uint64_t)prev * 6u + 4u + k) * n; }
    b.rec_t = tplanes + (uint64_t)cur * n;
    b.prev_rec_t = tplanes + (uint64_t)prev * n;
    b.out_diffuse = static_cast<float4*>(t->Diffuse);
    b.out_specular = static_cast<float4*>(t->Specular);
    RiParamsFull P{};
    P.frame_index = s->FrameIndex;
    P.initial_samples = s->InitialSamples ? s->InitialSamples : kRiDefaultInitialSamples;
    P.temporal = s->EnableTemporal; P.temporal_bias = s->TemporalBiasCorrection;
    P.max_history = s->MaxHistoryLength ? s->MaxHistoryLength : kRiDefaultHistory;
    P.spatial = s->EnableSpatial; P.spatial_bias = s->SpatialBiasCorrection;
    P.spatial_samples = s->SpatialSamples ? s->SpatialSamples : kRiDefaultSpatialSamples;
    P.radius = std::min(s->SpatialRadius == 0.0f ? kRiDefaultRadius : s->SpatialRadius, kRiMaxRadius);
    P.history_valid = restart ? 0u : 1u;
    P.cam_pos = make_f3(c->cam.Position[0], c->cam.Position[1], c->cam.Position[2]);
    P.prev_cam_pos = make_f3(c->cam.PreviousPosition[0], c->cam.PreviousPosition[1], c->cam.PreviousPosition[2]);
    if (cd) {
        P.brdf_samples = cd->BrdfSamples;
        P.boiling_filter = cd->EnableBoilingFilter;
        P.boiling_strength = cd->EnableBoilingFilter ? cd->BoilingFilterStrength : 0.0f;
    }
    if (sh && sh->ReuseFinalVisibility) {
        P.sh.reuse = 1u;
        P.sh.max_age = sh->FinalVisibilityMaxAge;
        P.sh.max_dist2 = sh->FinalVisibilityMaxDistance * sh->FinalVisibilityMaxDistance;
    }
    // row N22: launch 1 writes the visibility word where something of this call reads it or temporal resampling is pairwise; launch 2 is
    // the new one where the spatial pass is pairwise or final shading reuses the word.  Neither: the launches of rows N10 / N16 / N17.
    const bool full2 = P.sh.reuse || (P.spatial && P.spatial_bias == kRiBiasPairwise);
    const bool full1 = P.sh.reuse || (P.temporal && P.temporal_bias == kRiBiasPairwise);
    const PixelMap pm = make_pixel_map(w, h, PtRect{ 0, 0, w, h });  // (at most 2048^2 * 64 = 2^28 slots)
    const SceneView sv = make_scene_view(c, &L);
    const uint32_t grid = side_pass_grid(c, pm.n_slots);
    st = PT_OK;
    // Presampling (spec S22): pyramid -> Power_RIS -> ReGIR on the lane's stream, in front of launch 1.  The previous call's launch 1 read
    // the two buffers: this call is ordered after it by what orders the history above -- the stream itself on a one-lane context, the
    // ev_ri wait otherwise, and a host-side wait where the history was reallocated (a first call has no predecessor) -- so the existing
    // condition suffices.  The kernels read the lane's own spheres (sv.sph): an emitter moved by pt_update_spheres is seen.
    LrView lr{};
    if (mode != kLrUniform) {
        const uint32_t lv = lr_levels(c->n_lights), n_pyr = lr_pyramid_floats(lv);
        const uint32_t n_power = lg.tile_size * lg.tile_count;
        const uint32_t n_ris = n_power + (mode == kLrRegirRis ? lg.grid * lg.grid * lg.grid * lg.lights_per_cell : 0u);
        if (n_pyr > c->lr_cap_pyramid || n_ris > c->lr_cap_ris) {
            PT_HIP(c, hipEventSynchronize(c->ev_ri));  // (the previous call, on whichever lane, may still read the old buffers; a no-op before the first record)
            if (n_pyr > c->lr_cap_pyramid) {
                free_dev(c->d_lr_pyramid);
                c->lr_cap_pyramid = 0; c->lr_n_pyramid = 0;
                if (hipMalloc(reinterpret_cast<void**>(&c->d_lr_pyramid), (size_t)n_pyr * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return fail(c, PT_ERR_OOM, std::string(who) + ": pyramid allocation failed"); }
                c->lr_cap_pyramid = n_pyr;
            }
            if (n_ris > c->lr_cap_ris) {
                free_dev(c->d_lr_ris);
                c->lr_cap_ris = 0; c->lr_n_ris = 0;
                if (hipMalloc(&c->d_lr_ris, (size_t)n_ris * sizeof(LrEntry)) != hipSuccess) { (void)hipGetLastError(); return fail(c, PT_ERR_OOM, std::string(who) + ": RIS buffer allocation failed"); }
                c->lr_cap_ris = n_ris;
            }
        }
        lg.cam = P.cam_pos;
        LrBuild lb{};
        lb.sph = sv.sph; lb.mats = sv.mats; lb.lights = sv.lights; lb.n_lights = sv.n_lights; lb.frame_index = s->FrameIndex;
        lb.pyramid = c->d_lr_pyramid;
        lb.ris = static_cast<LrEntry*>(c->d_lr_ris);
        lb.grid = lg;
        const hipError_t e = profiled_launch(c, L.stream, 3, [&] {  // pt_get_profile: the presampling launches, as one interval, under ms_tail
            hipError_t e = launch_lr_pyramid(lb, L.stream);
            if (e == hipSuccess) e = launch_lr_power(lb, L.stream);
            return e == hipSuccess && mode == kLrRegirRis ? launch_lr_regir(lb, L.stream) : e;
        });
        if (e != hipSuccess) st = fail(c, PT_ERR_HIP, std::string(who) + ": presampling launch: " + hipGetErrorString(e));
        c->lr_n_pyramid = e == hipSuccess ? n_pyr : 0u;  // (pt_light_ris_download returns only what was built whole)
        c->lr_n_ris = e == hipSuccess ? n_ris : 0u;
        lr.ris = lb.ris;
        lr.tile_size = lg.tile_size; lr.tile_count = lg.tile_count; lr.grid = lg.grid; lr.lights_per_cell = lg.lights_per_cell; lr.cell_size = lg.cell_size;
    }
    for (int pass = 0; pass < 2 && st == PT_OK; pass++) {
        const RiExtra rx{ c->d_light_of, mode != kLrUniform ? c->d_lr_pyramid : nullptr, lr_levels(c->n_lights) };
        // pt_get_profile: launch 1 under ms_traverse, launch 2 under ms_shade
        const hipError_t e = profiled_launch(c, L.stream, pass == 0 ? 1 : 2, [&] {
            if (pass == 0 ? full1 : full2) return launch_restir_full(pass, sv, pm, b, P, mode, lr, rx, grid, L.stream);
            return pass == 0 ? launch_restir_pass1_ex(sv, pm, b, P, mode, lr, rx, grid, L.stream) : launch_restir_pass(pass, sv, pm, b, P, mode, lr, grid, L.stream);
        });
        if (e != hipSuccess) st = fail(c, PT_ERR_HIP, std::string(who) + ": launch: " + hipGetErrorString(e));
    }
    const hipError_t e0 = hipEventRecord(c->ev_ri, L.stream);
    if (st == PT_OK && e0 != hipSuccess) st = fail(c, PT_ERR_HIP, std::string(who) + ": history event: " + hipGetErrorString(e0));
    st = publish_lane_to_caller(c, L, who, st);
    if (st == PT_OK) {
        c->ri_slot = cur;
        c->ri_scene = c->set_scene_calls;
        c->ri_valid = true;
    } else {
        c->ri_valid = false;
    }
    return st;
}

PtStatus pt_restir_di(PtContext* c, const PtRestirDiSettings* s, const PtRestirDiTextures* t) { return restir_di_common(c, "pt_restir_di", s, nullptr, nullptr, nullptr, false, t); }

PtStatus pt_restir_di_sampled(PtContext* c, const PtRestirDiSettings* s, const PtLightSamplingSettings* ls, const PtRestirDiTextures* t) { return restir_di_common(c, "pt_restir_di_sampled", s, ls, nullptr, nullptr, false, t); }

PtStatus pt_restir_di_ex(PtContext* c, const PtRestirDiSettings* s, const PtLightSamplingSettings* ls, const PtRestirDiCandidates* cd, const PtRestirDiTextures* t) { return restir_di_common(c, "pt_restir_di_ex", s, ls, cd, nullptr, false, t); }

PtStatus pt_restir_di_full(PtContext* c, const PtRestirDiSettings* s, const PtLightSamplingSettings* ls, const PtRestirDiCandidates* cd, const PtRestirDiShading* sh,
                           const PtRestirDiTextures* t)
{
    return restir_di_common(c, "pt_restir_di_full", s, ls, cd, sh, true, t);
}

PtStatus pt_restir_di_history(PtContext* c, uint32_t which, void* planes, void* transmission)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (which > 1u || !planes || !transmission) return fail(c, PT_ERR_INVALID_ARG, "pt_restir_di_history: which must be 0 or 1 and the arrays non-null");
    if (!c->ri_valid || !c->d_ri) return fail(c, PT_ERR_STATE, "pt_restir_di_history: no pt_restir_di call has left a history");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipEventSynchronize(c->ev_ri));
    const uint64_t n = (uint64_t)c->ri_w * c->ri_h;
    const uint32_t slot = c->ri_slot ^ which;
    PT_HIP(c, hipMemcpy(planes, c->d_ri + (uint64_t)slot * 6u * n, 6u * n * sizeof(float4), hipMemcpyDeviceToHost));
    PT_HIP(c, hipMemcpy(transmission, reinterpret_cast<const float*>(c->d_ri + 12u * n) + (uint64_t)slot * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

PtStatus pt_light_ris_download(PtContext* c, float* pyramid, uint32_t* n_pyramid, uint32_t* ris, uint32_t* n_entries)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!n_pyramid || !n_entries) return fail(c, PT_ERR_INVALID_ARG, "pt_light_ris_download: null count");
    if (!c->lr_n_pyramid || !c->d_lr_pyramid || !c->d_lr_ris) return fail(c, PT_ERR_STATE, "pt_light_ris_download: no pt_restir_di_sampled call with a presampling mode has been made");
    const uint32_t cap_p = *n_pyramid, cap_r = *n_entries;
    *n_pyramid = c->lr_n_pyramid;
    *n_entries = c->lr_n_ris;
    if ((pyramid && cap_p < c->lr_n_pyramid) || (ris && cap_r < c->lr_n_ris)) return fail(c, PT_ERR_INVALID_ARG, "pt_light_ris_download: capacity below the count");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipEventSynchronize(c->ev_ri));
    if (pyramid) PT_HIP(c, hipMemcpy(pyramid, c->d_lr_pyramid, (size_t)c->lr_n_pyramid * sizeof(float), hipMemcpyDeviceToHost));
    if (ris) PT_HIP(c, hipMemcpy(ris, c->d_lr_ris, (size_t)c->lr_n_ris * sizeof(LrEntry), hipMemcpyDeviceToHost));
    return PT_OK;
}

// The stats of a frame-like side pass (pt_render_sharc*, pt_render_lens) that recorded PtContext::ev0 on the lane before its launches: the time
// between the two markers and the rays its kernels counted at d_rays.  Waits for the lane.
static PtStatus side_frame_stats(PtContext* c, Lane& L, const unsigned long long* d_rays, PtStats* stats, uint64_t pixels, uint64_t paths)
{
    unsigned long long rays = 0;
    PT_HIP(c, hipEventRecord(c->ev1, L.stream));
    PT_HIP(c, hipMemcpyAsync(&rays, d_rays, sizeof rays, hipMemcpyDeviceToHost, L.stream));
    PT_HIP(c, hipStreamSynchronize(L.stream));
    std::memset(stats, 0, sizeof *stats);
    float ms = 0;
    PT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    stats->ms_total = ms;
    stats->rays = rays;
    stats->pixels = pixels;
    stats->paths = paths;
    return PT_OK;
}

// Row N14 -- the frame through the radiance cache (DESIGN.md spec S20): up to three stages on the lane of the next render call, ordered
// like pt_restir_di; the cache (keys, two voxel arrays that swap at every resolve, two counters) lives in the context.
static PtStatus sharc_allocate(PtContext* c, uint32_t capacity)
{
    if (!c->ev_sh) PT_HIP(c, hipEventCreateWithFlags(&c->ev_sh, hipEventDisableTiming));
    if (c->d_sh && c->sh_capacity == capacity) return PT_OK;
    if (c->d_sh) PT_HIP(c, hipEventSynchronize(c->ev_sh));  // (the previous call may still use the old arrays)
    free_dev(c->d_sh);
    c->sh_valid = false;
    c->sh_capacity = 0;
    const size_t bytes = (size_t)capacity * (sizeof(uint64_t) + 2u * sizeof(uint4)) + 2u * sizeof(unsigned long long);
    if (hipMalloc(&c->d_sh, bytes) != hipSuccess) { (void)hipGetLastError(); c->d_sh = nullptr; return fail(c, PT_ERR_OOM, "pt_render_sharc: cache allocation failed"); }
    char* base = static_cast<char*>(c->d_sh);
    c->sh_accum = reinterpret_cast<uint4*>(base);
    c->sh_resolved = reinterpret_cast<uint4*>(base + (size_t)capacity * sizeof(uint4));
    c->sh_keys = reinterpret_cast<uint64_t*>(base + 2u * (size_t)capacity * sizeof(uint4));
    c->d_sh_counters = reinterpret_cast<unsigned long long*>(base + (size_t)capacity * (sizeof(uint64_t) + 2u * sizeof(uint4)));
    c->sh_capacity = capacity;
    return PT_OK;
}

static bool sharc_capacity_ok(uint32_t capacity) { return capacity >= kShBucket && capacity <= (1u << 28) && (capacity & (capacity - 1u)) == 0u; }

// pt_render_sharc (ex = false: di and outputs null) and pt_render_sharc_ex (row N18, DESIGN.md spec S24): one body.  `who` names the entry
// point in messages.  IsAntiFireflyEnabled (row N19, spec S25) is accepted by the _ex entry point only.
static PtStatus sharc_call(PtContext* c, const PtRect* rect, void* out, int out_is_device, const PtSharcSettings* s, const PtDirectLighting* di,
                           const PtDenoiserOutputs* outputs, PtStats* stats, bool ex, const std::string& who)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s) return fail(c, PT_ERR_INVALID_ARG, who + ": null settings");
    const uint32_t stages = s->Stages ? s->Stages : (uint32_t)(PT_SHARC_UPDATE | PT_SHARC_RESOLVE | PT_SHARC_QUERY);
    if (stages & ~7u) return fail(c, PT_ERR_INVALID_ARG, who + ": Stages must be a mask of PT_SHARC_UPDATE, PT_SHARC_RESOLVE and PT_SHARC_QUERY");
    if ((stages & PT_SHARC_QUERY) && !out) return fail(c, PT_ERR_INVALID_ARG, who + ": null output");
    if (s->_pad[0] || s->_pad[1]) return fail(c, PT_ERR_INVALID_ARG, who + ": the padding words must be 0");
    const uint32_t capacity = s->Capacity ? s->Capacity : kShDefaultCapacity, downscale = s->DownscaleFactor ? s->DownscaleFactor : kShDefaultDownscale;
    const float scene_scale = s->SceneScale == 0.0f ? kShDefaultSceneScale : s->SceneScale;
    const uint32_t acc_frames = s->AccumulationFrames ? s->AccumulationFrames : kShDefaultAccumulationFrames;
    const uint32_t max_stale = s->MaxStaleFrames ? s->MaxStaleFrames : kShDefaultMaxStaleFrames;
    if (!sharc_capacity_ok(capacity)) return fail(c, PT_ERR_INVALID_ARG, who + ": Capacity must be a power of two in [16, 1 << 28]");
    if (downscale > 4u) return fail(c, PT_ERR_INVALID_ARG, who + ": DownscaleFactor must be in [1, 4]");
    if (!(scene_scale >= 5.0f && scene_scale <= 100.0f)) return fail(c, PT_ERR_INVALID_ARG, who + ": SceneScale must be in [5, 100]");
    if (!(s->RoughnessThreshold >= 0.0f && s->RoughnessThreshold <= 1.0f)) return fail(c, PT_ERR_INVALID_ARG, who + ": RoughnessThreshold must be in [0, 1]");
    if (acc_frames > kShMaxFrames) return fail(c, PT_ERR_INVALID_ARG, who + ": AccumulationFrames must be at most 255");
    if (max_stale > kShMaxStale) return fail(c, PT_ERR_INVALID_ARG, who + ": MaxStaleFrames must be at most 254");
    const bool ff = s->IsAntiFireflyEnabled != 0;  // (row N19, spec S25: the _ex update and the resolve; no state of its own)
    if (ff && !ex) return fail(c, PT_ERR_UNSUPPORTED, who + ": IsAntiFireflyEnabled must be 0 (the anti-firefly filter runs through pt_render_sharc_ex)");
    PtStatus st = validate_frame(c);
    if (st != PT_OK) return st;
    if (!ex && (c->gs.IsDIEnabled || c->gs.Denoiser)) return fail(c, PT_ERR_UNSUPPORTED, who + ": IsDIEnabled and Denoiser must be 0 (DI and denoiser outputs through the cache are not built)");
    PtRect r;
    PixelMap pm{};
    if ((st = rect_pixel_map(c, rect, who.c_str(), r, pm)) != PT_OK) return st;
    DenoiseOut dn{};
    if (outputs && (st = denoise_out(c, outputs, who.c_str(), dn)) != PT_OK) return st;
    if (di && (stages & PT_SHARC_UPDATE) && (r.x || r.y || r.w != c->gs.RenderSize[0] || r.h != c->gs.RenderSize[1]))
        return fail(c, PT_ERR_INVALID_ARG, who + ": with di and the UPDATE stage rect must be NULL or the whole frame (the update reads the whole frame's DI)");
    if ((st = check_environment(c)) != PT_OK) return st;
    if ((st = check_tree_lds(c)) != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    const bool query = (stages & PT_SHARC_QUERY) != 0;
    float4* dev_out = nullptr;
    const size_t out_px = (size_t)r.w * r.h;
    if ((st = staged_out_begin(c, out, query && !out_is_device, out_px, dev_out)) != PT_OK) return st;
    if (query && (reinterpret_cast<uintptr_t>(dev_out) & 15u)) return fail(c, PT_ERR_INVALID_ARG, who + ": the output must be 16-byte aligned");
    if (di || outputs) {
        // the buffer rule of pt_args.h: presence and alignment of all, nothing the call writes sharing a byte with another buffer of the
        // call.  One exception: a DI buffer may BE the NRD modes' Diffuse or Specular (the same pointer: the update has read it before the
        // query writes, and that query reads no DI); such a DI buffer leaves the overlap table once its presence and alignment are checked.
        const uint64_t px = out_px;
        const BufferUse in[2] = { { di ? di->Diffuse : nullptr, px * 16u, 16u, false, di != nullptr, "di->Diffuse" },
                                  { di ? di->Specular : nullptr, px * 16u, 16u, false, di != nullptr, "di->Specular" } };
        std::string msg = check_buffers(who.c_str(), in, 2);
        if (msg.empty()) {
            auto is_nrd_output = [&](const void* p) { return p && (p == dn.diffuse || p == dn.specular); };
            const BufferUse all[6] = { { query ? dev_out : nullptr, px * 16u, 16u, true, false, "out" },
                                       { dn.spec_hit_dist, px * 4u, 4u, true, false, "SpecularHitDistance" },
                                       { dn.diffuse, px * 16u, 16u, true, false, "Diffuse" },
                                       { dn.specular, px * 16u, 16u, true, false, "Specular" },
                                       { is_nrd_output(in[0].p) ? nullptr : in[0].p, px * 16u, 16u, false, false, "di->Diffuse" },
                                       { is_nrd_output(in[1].p) ? nullptr : in[1].p, px * 16u, 16u, false, false, "di->Specular" } };
            msg = check_buffers(who.c_str(), all, 6);
        }
        if (!msg.empty()) return fail(c, PT_ERR_INVALID_ARG, msg);
    }

    Lane& L = c->lanes[c->next_lane];  // the lane of the next frame
    // (pt_lane_order.h: a supplied DI forces the wait; the denoiser outputs are held to the rule of `out` and, like the DI, enter the lane's ledger)
    const bool shared = ledger_cache({ c->ledgers, c->n_lanes, c->next_lane }, c->calls == 0, query, dev_out, outputs != nullptr, dn.spec_hit_dist, dn.diffuse, dn.specular,
                                     di != nullptr, di ? di->Diffuse : nullptr, di ? di->Specular : nullptr);
    if ((st = side_pass_begin(c, L, shared)) != PT_OK) return st;
    // the cache: the previous call (on whichever lane it ran) has finished with it before this one touches it
    const bool had = c->d_sh && c->sh_capacity == capacity;
    if ((st = sharc_allocate(c, capacity)) != PT_OK) return st;
    if (had) PT_HIP(c, hipStreamWaitEvent(L.stream, c->ev_sh, 0));
    const bool restart = s->ResetHistory != 0 || !c->sh_valid || c->sh_scene != c->set_scene_calls;
    c->sh_valid = false;  // (until the call has been queued whole)
    const bool timed = stats != nullptr;
    if (timed) PT_HIP(c, hipEventRecord(c->ev0, L.stream));
    if (restart) PT_HIP(c, hipMemsetAsync(c->d_sh, 0, (size_t)capacity * (sizeof(uint64_t) + 2u * sizeof(uint4)), L.stream));
    else if (stages & (PT_SHARC_UPDATE | PT_SHARC_RESOLVE)) PT_HIP(c, hipMemsetAsync(c->sh_accum, 0, (size_t)capacity * sizeof(uint4), L.stream));  // Raytracing.ixx:124
    PT_HIP(c, hipMemsetAsync(c->d_sh_counters, 0, 2u * sizeof(unsigned long long), L.stream));

    const SceneView sv = make_scene_view(c, &L);
    const uint32_t w = c->gs.RenderSize[0], h = c->gs.RenderSize[1];
    ShFrame fr{};
    fr.cam = camera_params(c->cam, w, h);
    fr.frame_index = c->gs.FrameIndex; fr.bounces = c->gs.Bounces; fr.spp = c->gs.SamplesPerPixel;
    fr.rr_enabled = c->gs.IsRussianRouletteEnabled ? 1u : 0u;
    fr.throughput_threshold = c->gs.ThroughputThreshold;
    fr.inv_spp = 1.0f / (float)c->gs.SamplesPerPixel;
    fr.roughness_threshold = s->RoughnessThreshold;
    fr.visualize = s->IsHashGridVisualizationEnabled ? 1u : 0u;
    if (di) {  // (the query reads them indexed like `out`: rect-sized; the update, which demands the whole frame, as RenderSize texels)
        fr.di_diffuse = static_cast<const float4*>(di->Diffuse);
        fr.di_specular = static_cast<const float4*>(di->Specular);
        fr.di_w = w; fr.di_h = h;
    }
    fr.dn_mode = dn.mode;
    fr.spec_hit_dist = dn.spec_hit_dist;
    fr.dn_diffuse = dn.diffuse;
    fr.dn_specular = dn.specular;
    ShGrid g{};
    g.cam_pos = make_f3(c->cam.Position[0], c->cam.Position[1], c->cam.Position[2]);
    g.scene_scale = scene_scale;
    auto map = [&] { ShMap m{}; m.keys = c->sh_keys; m.accum = c->sh_accum; m.resolved = c->sh_resolved; m.capacity = capacity; return m; };
    st = PT_OK;
    const uint32_t gw = w / downscale, gh = h / downscale;
    if ((stages & PT_SHARC_UPDATE) && gw && gh) {
        ShFrame fu = fr;
        fu.cam = camera_params(c->cam, gw, gh);  // (InvW, InvH of the update grid; the jitter is the path's own)
        const PixelMap pu = make_pixel_map(gw, gh, PtRect{ 0, 0, gw, gh });
        // pt_get_profile: the update under ms_traverse
        const hipError_t e = profiled_launch(c, L.stream, 1, [&] { return di || ff ? launch_sharc_update_ex(sv, pu, fu, g, map(), c->d_sh_counters, side_pass_grid(c, pu.n_slots), ff, L.stream)
                                                                              : launch_sharc_update(sv, pu, fu, g, map(), c->d_sh_counters, side_pass_grid(c, pu.n_slots), L.stream); });
        if (e != hipSuccess) st = fail(c, PT_ERR_HIP, who + ": update launch: " + hipGetErrorString(e));
    }
    if (st == PT_OK && (stages & PT_SHARC_RESOLVE)) {
        const hipError_t e = profiled_launch(c, L.stream, 3, [&] { return launch_sharc_resolve(map(), acc_frames, max_stale, ff, L.stream); });  // ... the resolve under ms_tail
        if (e != hipSuccess) st = fail(c, PT_ERR_HIP, who + ": resolve launch: " + hipGetErrorString(e));
        else std::swap(c->sh_accum, c->sh_resolved);  // Raytracing.ixx:147
    }
    if (st == PT_OK && query) {
        // ... the query under ms_shade
        const hipError_t e = profiled_launch(c, L.stream, 2, [&] { return (di || outputs ? launch_sharc_query_ex : launch_sharc_query)(sv, pm, fr, g, map(), dev_out, c->d_sh_counters, side_pass_grid(c, pm.n_slots), L.stream); });
        if (e != hipSuccess) st = fail(c, PT_ERR_HIP, who + ": query launch: " + hipGetErrorString(e));
    }
    const hipError_t e0 = hipEventRecord(c->ev_sh, L.stream);
    if (st == PT_OK && e0 != hipSuccess) st = fail(c, PT_ERR_HIP, who + ": cache event: " + hipGetErrorString(e0));
    if (st == PT_OK && timed)
        if (const PtStatus e = side_frame_stats(c, L, c->d_sh_counters, stats, query ? out_px : 0,
                                                (query ? out_px * c->gs.SamplesPerPixel : 0) + ((stages & PT_SHARC_UPDATE) ? (uint64_t)gw * gh : 0)); e != PT_OK) return e;
    st = publish_lane_to_caller(c, L, who.c_str(), st);
    if (st != PT_OK) return st;
    c->sh_valid = true;
    c->sh_scene = c->set_scene_calls;
    return staged_out_finish(c, out, query && !out_is_device, out_px);
}

PtStatus pt_render_sharc(PtContext* c, const PtRect* rect, void* out, int out_is_device, const PtSharcSettings* s, PtStats* stats) { return sharc_call(c, rect, out, out_is_device, s, nullptr, nullptr, stats, false, "pt_render_sharc"); }

PtStatus pt_render_sharc_ex(PtContext* c, const PtRect* rect, void* out, int out_is_device, const PtSharcSettings* s, const PtDirectLighting* di, const PtDenoiserOutputs* outputs, PtStats* stats) { return sharc_call(c, rect, out, out_is_device, s, di, outputs, stats, true, "pt_render_sharc_ex"); }

// Row N26 -- the pure path-traced frame through the thin-lens camera (DESIGN.md spec S29): one launch on the lane of the next render call,
// ordered like pt_render_sharc's query (the cache family of pt_lane_order.h with QUERY, no DI and no denoiser outputs).  The only entry
// point that reads PtCamera::ApertureRadius.
PtStatus pt_render_lens(PtContext* c, const PtRect* rect, void* out, int out_is_device, PtStats* stats)
{
    const char* who = "pt_render_lens";
    if (!c) return PT_ERR_INVALID_ARG;
    if (!out) return fail(c, PT_ERR_INVALID_ARG, "pt_render_lens: null output");
    PtStatus st = validate_frame(c);
    if (st != PT_OK) return st;
    if (c->gs.IsDIEnabled || c->gs.Denoiser) return fail(c, PT_ERR_UNSUPPORTED, "pt_render_lens: IsDIEnabled and Denoiser must be 0 (DI and denoiser outputs behind the lens are not built)");
    const float aperture = c->cam.ApertureRadius;
    if (!(aperture >= 0.0f) || !std::isfinite(aperture)) return fail(c, PT_ERR_INVALID_ARG, "pt_render_lens: ApertureRadius must be finite and not negative");
    PtRect r;
    PixelMap pm{};
    if ((st = rect_pixel_map(c, rect, who, r, pm)) != PT_OK) return st;
    if ((st = check_environment(c)) != PT_OK) return st;
    if ((st = check_tree_lds(c)) != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    float4* dev_out = nullptr;
    const size_t out_px = (size_t)r.w * r.h;
    if ((st = staged_out_begin(c, out, !out_is_device, out_px, dev_out)) != PT_OK) return st;
    if (reinterpret_cast<uintptr_t>(dev_out) & 15u) return fail(c, PT_ERR_INVALID_ARG, "pt_render_lens: the output must be 16-byte aligned");
    if (!c->d_lens_counters) PT_HIP(c, hipMalloc(&c->d_lens_counters, kMaxLanes * sizeof(unsigned long long)));  // (every call clears its lane's counter on the lane's stream)

    Lane& L = c->lanes[c->next_lane];  // the lane of the next frame
    const bool shared = ledger_cache({ c->ledgers, c->n_lanes, c->next_lane }, c->calls == 0, true, dev_out, false, nullptr, nullptr, nullptr, false, nullptr, nullptr);
    if ((st = side_pass_begin(c, L, shared)) != PT_OK) return st;
    unsigned long long* counter = c->d_lens_counters + c->next_lane;
    const bool timed = stats != nullptr;
    if (timed) PT_HIP(c, hipEventRecord(c->ev0, L.stream));
    PT_HIP(c, hipMemsetAsync(counter, 0, sizeof(unsigned long long), L.stream));
    const SceneView sv = make_scene_view(c, &L);
    const LensFrame fr = lens_frame(c->cam, c->gs.RenderSize[0], c->gs.RenderSize[1], c->gs.FrameIndex, c->gs.Bounces, c->gs.SamplesPerPixel,
                                    c->gs.IsRussianRouletteEnabled != 0, c->gs.ThroughputThreshold);
    // pt_get_profile: the frame under ms_shade, like the cache's query
    const hipError_t e = profiled_launch(c, L.stream, 2, [&] { return launch_lens(sv, pm, fr, dev_out, counter, side_pass_grid(c, pm.n_slots), L.stream); });
    st = e == hipSuccess ? PT_OK : fail(c, PT_ERR_HIP, std::string("pt_render_lens: launch: ") + hipGetErrorString(e));
    if (st == PT_OK && timed)
        if (const PtStatus e2 = side_frame_stats(c, L, counter, stats, out_px, out_px * c->gs.SamplesPerPixel); e2 != PT_OK) return e2;
    st = publish_lane_to_caller(c, L, who, st);
    if (st != PT_OK) return st;
    return staged_out_finish(c, out, !out_is_device, out_px);
}

// Row N27 -- the frame whose first vertex is the G-buffer's texel (DESIGN.md spec S30): one launch on the lane of the next render call, on
// pt_render_lens's lane and ledger (the cache family's query) with the eight input channels and the optional DI as inputs (ledger_gbframe).
PtStatus pt_render_from_gbuffer(PtContext* c, const PtRect* rect, void* out, int out_is_device, const PtGBufferInput* in, const PtDirectLighting* di, PtStats* stats)
{
    const char* who = "pt_render_from_gbuffer";
    if (!c) return PT_ERR_INVALID_ARG;
    if (!out) return fail(c, PT_ERR_INVALID_ARG, "pt_render_from_gbuffer: null output");
    if (!in) return fail(c, PT_ERR_INVALID_ARG, "pt_render_from_gbuffer: null PtGBufferInput");
    if (in->Format > kGbFormatPacked) return fail(c, PT_ERR_INVALID_ARG, "pt_render_from_gbuffer: Format must be 0 (the float32 layouts of PtGBuffer) or 1 (those of PtGBufferPacked)");
    if (in->_pad != 0) return fail(c, PT_ERR_INVALID_ARG, "pt_render_from_gbuffer: PtGBufferInput._pad must be 0");
    PtStatus st = validate_frame(c);
    if (st != PT_OK) return st;
    // the reference's Denoiser::None frame; its IsDIEnabled is `di` (as pt_render_with_di: whatever the constants say once a DI is supplied)
    if (c->gs.Denoiser) return fail(c, PT_ERR_INVALID_ARG, "pt_render_from_gbuffer: Denoiser must be 0 (denoiser outputs through this entry point are not built)");
    if (c->gs.IsDIEnabled && !di) return fail(c, PT_ERR_INVALID_ARG, "pt_render_from_gbuffer: IsDIEnabled is set and no direct lighting is supplied (this frame makes no estimate of its own)");
    PtRect r;
    PixelMap pm{};
    if ((st = rect_pixel_map(c, rect, who, r, pm)) != PT_OK) return st;
    if ((st = check_environment(c)) != PT_OK) return st;
    if ((st = check_tree_lds(c)) != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    float4* dev_out = nullptr;
    const size_t out_px = (size_t)r.w * r.h;
    if ((st = staged_out_begin(c, out, !out_is_device, out_px, dev_out)) != PT_OK) return st;
    {
        // the buffer rule of pt_args.h: every channel present and aligned to its texel, `out` sharing no byte with an input
        const bool packed = in->Format == kGbFormatPacked;
        const uint64_t px = out_px;
        auto texel = [&](uint32_t channel, uint32_t f32_bytes) { return packed ? kGbPackedTexelBytes[channel] : f32_bytes; };
        auto align = [&](uint32_t channel, uint32_t f32_align) { return packed ? kGbPackedTexelBytes[channel] : f32_align; };
        const BufferUse use[11] = { { dev_out, px * 16u, 16u, true, true, "out" },
                                    { in->Position, px * 16u, 16u, false, true, "Position" },
                                    { in->FlatNormal, px * texel(1, 8), align(1, 8), false, true, "FlatNormal" },
                                    { in->GeometricNormal, px * texel(2, 8), align(2, 8), false, true, "GeometricNormal" },
                                    { in->BaseColorMetalness, px * texel(6, 16), align(6, 16), false, true, "BaseColorMetalness" },
                                    { in->NormalRoughness, px * texel(9, 16), align(9, 16), false, true, "NormalRoughness" },
                                    { in->IOR, px * texel(10, 4), align(10, 4), false, true, "IOR" },
                                    { in->Transmission, px * texel(11, 4), align(11, 4), false, true, "Transmission" },
                                    { in->Radiance, px * texel(12, 12), align(12, 4), false, true, "Radiance" },
                                    { di ? di->Diffuse : nullptr, px * 16u, 16u, false, di != nullptr, "di->Diffuse" },
                                    { di ? di->Specular : nullptr, px * 16u, 16u, false, di != nullptr, "di->Specular" } };
        const std::string msg = check_buffers(who, use, 11);
        if (!msg.empty()) return fail(c, PT_ERR_INVALID_ARG, msg);
    }
    if (!c->d_lens_counters) PT_HIP(c, hipMalloc(&c->d_lens_counters, kMaxLanes * sizeof(unsigned long long)));  // (every call clears its lane's counter on the lane's stream)

    Lane& L = c->lanes[c->next_lane];  // the lane of the next frame
    const void* const in13[13] = { in->Position, in->FlatNormal, in->GeometricNormal, nullptr, nullptr, nullptr, in->BaseColorMetalness, nullptr, nullptr,
                                   in->NormalRoughness, in->IOR, in->Transmission, in->Radiance };
    const bool shared = ledger_gbframe({ c->ledgers, c->n_lanes, c->next_lane }, c->calls == 0, dev_out, in13, di != nullptr, di ? di->Diffuse : nullptr, di ? di->Specular : nullptr);
    if ((st = side_pass_begin(c, L, shared)) != PT_OK) return st;
    unsigned long long* counter = c->d_lens_counters + c->next_lane;
    const bool timed = stats != nullptr;
    if (timed) PT_HIP(c, hipEventRecord(c->ev0, L.stream));
    PT_HIP(c, hipMemsetAsync(counter, 0, sizeof(unsigned long long), L.stream));
    const SceneView sv = make_scene_view(c, &L);
    const GbFrame fr = gb_frame(c->cam, c->gs.RenderSize[0], c->gs.RenderSize[1], c->gs.FrameIndex, c->gs.Bounces, c->gs.SamplesPerPixel,
                                c->gs.IsRussianRouletteEnabled != 0, c->gs.ThroughputThreshold);
    const GbInput gi{ in->Format, static_cast<const float4*>(in->Position), in->FlatNormal, in->GeometricNormal, in->BaseColorMetalness, in->NormalRoughness, in->IOR,
                      in->Transmission, in->Radiance, di ? static_cast<const float4*>(di->Diffuse) : nullptr, di ? static_cast<const float4*>(di->Specular) : nullptr };
    // pt_get_profile: the frame under ms_shade, like pt_render_lens
    const hipError_t e = profiled_launch(c, L.stream, 2, [&] { return launch_gbframe(sv, pm, fr, gi, dev_out, counter, side_pass_grid(c, pm.n_slots), L.stream); });
    st = e == hipSuccess ? PT_OK : fail(c, PT_ERR_HIP, std::string("pt_render_from_gbuffer: launch: ") + hipGetErrorString(e));
    if (st == PT_OK && timed)
        if (const PtStatus e2 = side_frame_stats(c, L, counter, stats, out_px, out_px * c->gs.SamplesPerPixel); e2 != PT_OK) return e2;
    st = publish_lane_to_caller(c, L, who, st);
    if (st != PT_OK) return st;
    return staged_out_finish(c, out, !out_is_device, out_px);
}

PtStatus pt_sharc_download(PtContext* c, void* keys, void* voxels, uint32_t capacity)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!keys || !voxels) return fail(c, PT_ERR_INVALID_ARG, "pt_sharc_download: null pointer");
    if (!c->d_sh || !c->sh_valid) return fail(c, PT_ERR_STATE, "pt_sharc_download: there is no cache (no pt_render_sharc call has completed)");
    if (capacity != c->sh_capacity) return fail(c, PT_ERR_INVALID_ARG, "pt_sharc_download: capacity differs from the cache's");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipEventSynchronize(c->ev_sh));
    PT_HIP(c, hipMemcpy(keys, c->sh_keys, (size_t)capacity * sizeof(uint64_t), hipMemcpyDeviceToHost));
    PT_HIP(c, hipMemcpy(voxels, c->sh_resolved, (size_t)capacity * sizeof(uint4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PtStatus pt_sharc_upload(PtContext* c, const void* keys, const void* voxels, uint32_t capacity)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!keys || !voxels) return fail(c, PT_ERR_INVALID_ARG, "pt_sharc_upload: null pointer");
    if (!sharc_capacity_ok(capacity)) return fail(c, PT_ERR_INVALID_ARG, "pt_sharc_upload: capacity must be a power of two in [16, 1 << 28]");
    PT_HIP(c, hipSetDevice(c->device));
    if (const PtStatus st = sharc_allocate(c, capacity); st != PT_OK) return st;
    PT_HIP(c, hipEventSynchronize(c->ev_sh));
    PT_HIP(c, hipMemcpy(c->sh_keys, keys, (size_t)capacity * sizeof(uint64_t), hipMemcpyHostToDevice));
    PT_HIP(c, hipMemcpy(c->sh_resolved, voxels, (size_t)capacity * sizeof(uint4), hipMemcpyHostToDevice));
    PT_HIP(c, hipMemset(c->sh_accum, 0, (size_t)capacity * sizeof(uint4)));
    PT_HIP(c, hipDeviceSynchronize());  // (a memset may return before the device has finished it: the lanes' streams do not wait for the null stream)
    c->sh_valid = true;
    c->sh_scene = c->set_scene_calls;
    return PT_OK;
}

}  // extern "C"
