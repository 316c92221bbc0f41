// lens_host.cpp -- TEST SHIM: compiles the product's thin-lens header (csrc/pt_lens.h, row N26) as plain host C++ (the flags of
// sharc_host.cpp) so the tests can check it against the float64 restatement without a GPU, and the GPU kernel against it bit for bit.
// Not part of the product; never loaded by it.
#include "lens_host.h"

using namespace lenshost;

extern "C" {

// ---- ImportanceSampling::Uniform::GetRay(u).xy
void lens_host_get_ray(const float* u1, const float* u2, uint32_t n, float* xy)
{
    for (uint32_t i = 0; i < n; i++) lens_get_ray(u1[i], u2[i], xy[2 * i], xy[2 * i + 1]);
}

// ---- lens_ray for n (pixel, lens sample) pairs of one camera: o, d (3 floats each), tmin / tmax (2 floats)
void lens_host_rays(const PtCamera* cam, uint32_t w, uint32_t h, const uint32_t* px, const uint32_t* py, const float* u1, const float* u2, uint32_t n, float* o, float* d,
                    float* tt)
{
    const LensFrame fr = lens_frame(*cam, w, h, 0, 0, 1, false, 0.0f);
    for (uint32_t i = 0; i < n; i++) {
        f3 oo, dd;
        lens_ray(fr, px[i], py[i], u1[i], u2[i], oo, dd, tt[2 * i], tt[2 * i + 1]);
        o[3 * i] = oo.x; o[3 * i + 1] = oo.y; o[3 * i + 2] = oo.z;
        d[3 * i] = dd.x; d[3 * i + 1] = dd.y; d[3 * i + 2] = dd.z;
    }
}

// ---- the lens stream's numbers of a pixel: 2 * n_samples floats in draw order
void lens_host_stream(uint32_t px, uint32_t py, uint32_t frame_index, uint32_t n_samples, float* u)
{
    uint32_t lens = hash_combine(rng_init(px, py, frame_index), kLensSeed);
    for (uint32_t i = 0; i < 2u * n_samples; i++) u[i] = rng_float(lens);
}

// ---- one pt_render_lens call (lens_host.h run_frame).  Scene arguments as sh_host_call (sharc_host.cpp).  env_map = {EnvironmentLightTextureDescriptor,
// IsEnvironmentLightTextureCubeMap}, env_xf = the 16 floats of EnvironmentLightTransform; pixel_rays may be null.
uint64_t lens_host_frame(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                         const uint32_t* maps, const float* rot, const uint32_t* env_map, const float* env_xf, const PtCamera* cam, const uint32_t* prm, float throughput_threshold, float* out,
                         uint32_t* pixel_rays)
{
    shhost::HostScene hs;
    hs.set(spheres, materials, n, env, texels, tex_info, n_tex, maps, rot);
    HostEnvMap em;
    em.tex = env_map[0]; em.cube = env_map[1] ? 1u : 0u;
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) em.xf[3 * r + k] = env_xf[4 * r + k];
    return run_frame(hs, em, frame_of(cam, prm, throughput_threshold), prm + 6, out, pixel_rays);
}

// ---- the pixels whose pinhole primary ray hits (the aperture-0 test's ray count: such a pixel traces spp primaries, pt_render one)
uint32_t lens_host_primary_hits(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const PtCamera* cam, const uint32_t* prm)
{
    const float env[4] = { 0, 0, 0, 1 };
    shhost::HostScene hs;
    hs.set(spheres, materials, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    const CameraParams cp = camera_params(*cam, prm[0], prm[1]);
    uint32_t hits = 0;
    for (uint32_t y = 0; y < prm[9]; y++)
        for (uint32_t x = 0; x < prm[8]; x++) {
            f3 o, d;
            float tmin, tmax, t;
            uint32_t id;
            primary_ray(cp, prm[6] + x, prm[7] + y, o, d, tmin, tmax);
            hs.trace(o, d, tmin, tmax, t, id);
            hits += id != 0xFFFFFFFFu;
        }
    return hits;
}

}  // extern "C"
