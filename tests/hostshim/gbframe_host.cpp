// gbframe_host.cpp -- TEST SHIM: compiles the product's texel formats and G-buffer frame (csrc/pt_pixfmt.h, csrc/pt_gbframe.h, row N27) as
// plain host C++ (the flags of lens_host.cpp) so the tests can check them against numpy restatements without a GPU, and the GPU kernels
// against them bit for bit.  Not part of the product; never loaded by it.
#include "gbframe_host.h"
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_lane_order.h"

using namespace gbfhost;

namespace {

HostEnvMap env_map_of(const uint32_t* env_map, const float* env_xf)
{
    HostEnvMap em;
    em.tex = env_map[0]; em.cube = env_map[1] ? 1u : 0u;
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) em.xf[3 * r + k] = env_xf[4 * r + k];
    return em;
}

}  // namespace

extern "C" {

// ---- the leaf functions of pt_pixfmt.h over 32-bit words (gbframe_host.h leaf; the signature of gbframe_leaf_gpu.hip's gbf_gpu_leaf)
int gbf_host_leaf(uint32_t op, uint32_t n, const uint32_t* in, uint32_t* out)
{
    if (op >= kLeafCount) return 1;
    for (uint32_t i = 0; i < n; i++) out[i] = leaf(op, in[i]);
    return 0;
}

// ---- a unit vector through the G-buffer's normal texel and back: decode_unit_vector(unpack(pack(encode_unit_vector(v))))
void gbf_host_normal_round_trip(const float* v, uint32_t n, float* out)
{
    for (uint32_t i = 0; i < n; i++) {
        const f2 e = gbp_unpack_normal(gbp_pack_normal(encode_unit_vector(make_f3(v[3 * i], v[3 * i + 1], v[3 * i + 2]))));
        const f3 r = decode_unit_vector(e.x, e.y);
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}

// ---- the packers applied to float32 pixels (32 floats each, gbuffer_host.cpp's layout) with their masks: the stores of the packed pass
void gbf_host_pack(const float* f32, const uint32_t* mask, uint32_t n, void* const* packed)
{
    for (uint32_t i = 0; i < n; i++) store_packed(pixel_of_floats(f32 + (size_t)kFloatsPerPixel * i, mask[i]), packed, i);
}

// ---- one pt_render_gbuffer / pt_render_gbuffer_packed call (gbframe_host.h run_gbuffer).  Scene arguments as lens_host_frame; is_static =
// SceneData.IsStatic; prm = {RenderSize w, h, rect x, y, w, h}; prev_sph / prev_rot: n float4 each or null.
void gbf_host_gbuffer(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                      const uint32_t* maps, const float* rot, const uint32_t* env_map, const float* env_xf, uint32_t is_static, const PtCamera* cam, const uint32_t* prm,
                      const float* prev_sph, const float* prev_rot, uint32_t want, float* f32, uint32_t* mask, float* t, uint32_t* id, void* const* packed)
{
    shhost::HostScene hs;
    hs.set(spheres, materials, n, env, texels, tex_info, n_tex, maps, rot);
    std::vector<float4> psph, prot;
    if (prev_sph) { psph.resize(n); std::memcpy(psph.data(), prev_sph, (size_t)n * sizeof(float4)); }
    if (prev_rot) { prot.resize(n); std::memcpy(prot.data(), prev_rot, (size_t)n * sizeof(float4)); }
    run_gbuffer(hs, env_map_of(env_map, env_xf), is_static != 0, cam, prm[0], prm[1], prm + 2, prev_sph ? psph.data() : nullptr, prev_rot ? prot.data() : nullptr, rot != nullptr,
                want, f32, mask, t, id, packed);
}

// ---- one pt_render_from_gbuffer call (gbframe_host.h run_frame).  prm = {RenderSize w, h, FrameIndex, Bounces, SamplesPerPixel,
// IsRussianRouletteEnabled, rect x, y, w, h}; in8: Position, FlatNormal, GeometricNormal, BaseColorMetalness, NormalRoughness, IOR,
// Transmission, Radiance in `format`; di_diffuse / di_specular: float4 per pixel or null; pixel_rays may be null.
uint64_t gbf_host_frame(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                        const uint32_t* maps, const float* rot, const uint32_t* env_map, const float* env_xf, const PtCamera* cam, const uint32_t* prm, float throughput_threshold,
                        uint32_t format, const void* const* in8, const float* di_diffuse, const float* di_specular, float* out, uint32_t* pixel_rays)
{
    shhost::HostScene hs;
    hs.set(spheres, materials, n, env, texels, tex_info, n_tex, maps, rot);
    const GbInput in{ format, static_cast<const float4*>(in8[0]), in8[1], in8[2], in8[3], in8[4], in8[5], in8[6], in8[7],
                      reinterpret_cast<const float4*>(di_diffuse), reinterpret_cast<const float4*>(di_specular) };
    return run_frame(hs, env_map_of(env_map, env_xf), frame_of(cam, prm, throughput_threshold), in, prm + 6, out, pixel_rays);
}

// ---- ledger_gbframe (csrc/pt_lane_order.h) over flat arrays, as args_host.cpp exposes the other four families: led = n_lanes ledgers of 21
// addresses each (out, dn[3], di[2], gb[13], ri[2]), updated in place; in13: the 13 channel slots (0 = null); -> shared
uint32_t gbf_host_ledger_gbframe(uint64_t* led, uint32_t n_lanes, uint32_t own, uint32_t first_call, uint64_t out, const uint64_t* in13, uint32_t has_di, const uint64_t* di)
{
    auto ptr = [](uint64_t a) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a)); };
    auto copy = [&](pt::LaneLedger& l, uint64_t* w, bool load) {
        const void** slots[21] = { &l.out, &l.dn[0], &l.dn[1], &l.dn[2], &l.di[0], &l.di[1] };
        for (int k = 0; k < 13; k++) slots[6 + k] = &l.gb[k];
        slots[19] = &l.ri[0]; slots[20] = &l.ri[1];
        for (int k = 0; k < 21; k++) {
            if (load) *slots[k] = ptr(w[k]);
            else w[k] = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(*slots[k]));
        }
    };
    std::vector<pt::LaneLedger> l(n_lanes);
    std::vector<pt::LaneLedger*> of(n_lanes);
    for (uint32_t i = 0; i < n_lanes; i++) { copy(l[i], led + i * 21u, true); of[i] = &l[i]; }
    const void* in[13];
    for (int k = 0; k < 13; k++) in[k] = ptr(in13[k]);
    const bool shared = pt::ledger_gbframe(pt::Ledgers{ of.data(), n_lanes, own }, first_call != 0, ptr(out), in, has_di != 0, ptr(di[0]), ptr(di[1]));
    for (uint32_t i = 0; i < n_lanes; i++) copy(l[i], led + i * 21u, false);
    return shared ? 1u : 0u;
}

}  // extern "C"
