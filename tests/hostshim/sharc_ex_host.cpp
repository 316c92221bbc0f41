// sharc_ex_host.cpp -- TEST SHIM: csrc/pt_sharc.h's _ex functions (row N18, DESIGN.md spec S24) compiled as plain host C++ (the flags of
// sharc_host.cpp), so that the tests can check the DI and denoiser-output rules without a GPU and the GPU kernels against them bit for
// bit.  Not part of the product; never loaded by it.
#include "sharc_ex_host.h"

using namespace shhost;

extern "C" {

// one pt_render_sharc_ex call: the arguments of sh_host_call (sharc_host.cpp), then the extras -- di_diffuse / di_specular (float4 per
// texel, null = no DI), the denoiser mode, SpecularHitDistance (float), Diffuse / Specular (float4); out and the outputs keep what the
// call does not write
void sh_host_call_ex(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                     const uint32_t* maps, const float* rot, const PtCamera* cam, const uint32_t* prm, const float* fprm, uint64_t* keys, uint32_t* accum,
                     uint32_t* resolved, float* out, uint64_t* counters, const float* di_diffuse, const float* di_specular, uint32_t mode, float* spec_hit_dist,
                     float* diffuse, float* specular)
{
    HostScene hs;
    hs.set(spheres, materials, n, env, texels, tex_info, n_tex, maps, rot);
    const Frame f(cam, prm, fprm);
    Extras x;
    x.di_diffuse = reinterpret_cast<const float4*>(di_diffuse);
    x.di_specular = reinterpret_cast<const float4*>(di_specular);
    x.mode = mode;
    x.spec_hit_dist = spec_hit_dist;
    x.diffuse = reinterpret_cast<float4*>(diffuse);
    x.specular = reinterpret_cast<float4*>(specular);
    run_call_ex(hs, cam, f, keys, reinterpret_cast<uint4*>(accum), reinterpret_cast<uint4*>(resolved), out, counters, x);
}

// n_rays rays (origin, unit direction: 3 floats each; tmin 0, tmax inf) through HostScene::trace and through CulledTrace: t and id of both
void sh_host_trace_both(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* origins, const float* directions, uint32_t n_rays, float* t_plain,
                        uint32_t* id_plain, float* t_culled, uint32_t* id_culled)
{
    const float env[4] = { 0.0f, 0.0f, 0.0f, 1.0f };
    HostScene hs;
    hs.set(spheres, materials, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    const CulledTrace culled(hs);
    for (uint32_t i = 0; i < n_rays; i++) {
        const f3 o = make_f3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), d = make_f3(directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]);
        hs.trace(o, d, 0.0f, kInf, t_plain[i], id_plain[i]);
        culled.trace(o, d, 0.0f, kInf, t_culled[i], id_culled[i]);
    }
}

// sh_texel of the update's DI look-up, for its edge values
void sh_host_texel(const float* u, uint32_t n_u, uint32_t n, uint32_t* texel)
{
    for (uint32_t i = 0; i < n_u; i++) texel[i] = sh_texel(u[i], n);
}

}  // extern "C"
