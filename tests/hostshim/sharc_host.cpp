// sharc_host.cpp -- TEST SHIM: compiles the product's radiance-cache header (csrc/pt_sharc.h, row N14) as plain host C++ (the flags of
// restir_host.cpp) so the tests can check it piece by piece against the float64 restatement without a GPU, and the GPU kernels against it
// bit for bit.  Not part of the product; never loaded by it.
#include "sharc_host.h"

using namespace shhost;

extern "C" {

// ---- the hash grid
void sh_host_level(const float* dist2, uint32_t n, float scene_scale, uint32_t* level, float* voxel)
{
    for (uint32_t i = 0; i < n; i++) { level[i] = sh_grid_level(dist2[i]); voxel[i] = sh_voxel_size(level[i], scene_scale); }
}

void sh_host_voxel_size(const uint32_t* level, uint32_t n, float scene_scale, float* voxel)
{
    for (uint32_t i = 0; i < n; i++) voxel[i] = sh_voxel_size(level[i], scene_scale);
}

void sh_host_key(const float* P, const float* N, const uint32_t* level, const float* voxel, uint32_t n, uint64_t* keys)
{
    for (uint32_t i = 0; i < n; i++)
        keys[i] = sh_key(make_f3(P[3 * i], P[3 * i + 1], P[3 * i + 2]), make_f3(N[3 * i], N[3 * i + 1], N[3 * i + 2]), level[i], voxel[i]);
}

void sh_host_key_at(const float* cam, float scene_scale, const float* P, const float* N, uint32_t n, uint64_t* keys, float* voxel)
{
    ShGrid g{};
    g.cam_pos = make_f3(cam[0], cam[1], cam[2]);
    g.scene_scale = scene_scale;
    for (uint32_t i = 0; i < n; i++)
        keys[i] = sh_key_at(g, make_f3(P[3 * i], P[3 * i + 1], P[3 * i + 2]), make_f3(N[3 * i], N[3 * i + 1], N[3 * i + 2]), voxel[i]);
}

void sh_host_bucket(const uint64_t* keys, uint32_t n, uint32_t capacity, uint32_t* base)
{
    for (uint32_t i = 0; i < n; i++) base[i] = sh_bucket_base(keys[i], capacity);
}

// ---- the hash map: op 0 find, 1 insert, 2 erase (what the resolve does to an evicted slot) -> the slot, or kShNoSlot
void sh_host_map_ops(uint64_t* keys, uint32_t capacity, const uint32_t* op, const uint64_t* key, uint32_t n, uint32_t* slot)
{
    for (uint32_t i = 0; i < n; i++) {
        if (op[i] == 1u) slot[i] = sh_insert(keys, capacity, key[i]);
        else slot[i] = sh_find(keys, capacity, key[i]);
        if (op[i] == 2u && slot[i] != kShNoSlot) keys[slot[i]] = 0u;
    }
}

// ---- the voxel
void sh_host_quantise(const float* x, uint32_t n, uint32_t* q)
{
    for (uint32_t i = 0; i < n; i++) q[i] = sh_quantise(x[i]);
}

void sh_host_add(uint32_t* accum, uint32_t slot, const float* rgb, uint32_t samples)
{
    sh_add(reinterpret_cast<uint4*>(accum), slot, make_f3(rgb[0], rgb[1], rgb[2]), samples);
}

void sh_host_resolve(const uint32_t* acc, const uint32_t* prev, uint32_t n, uint32_t accumulation_frames, uint32_t max_stale_frames, uint32_t* out, uint32_t* clear)
{
    for (uint32_t i = 0; i < n; i++) {
        bool c;
        const uint4 r = sh_resolve_slot(reinterpret_cast<const uint4*>(acc)[i], reinterpret_cast<const uint4*>(prev)[i], accumulation_frames, max_stale_frames, c);
        reinterpret_cast<uint4*>(out)[i] = r;
        clear[i] = c ? 1u : 0u;
    }
}

void sh_host_radiance(const uint32_t* voxels, uint32_t n, float* rgb)
{
    for (uint32_t i = 0; i < n; i++) {
        const f3 r = sh_radiance(reinterpret_cast<const uint4*>(voxels)[i]);
        rgb[3 * i] = r.x; rgb[3 * i + 1] = r.y; rgb[3 * i + 2] = r.z;
    }
}

// ---- the query's validity rule: valid[i], and the roughness after its clamp
void sh_host_valid_hit(const float* distance, const float* voxel, float* previous_roughness, uint32_t n, uint32_t* valid)
{
    for (uint32_t i = 0; i < n; i++) valid[i] = sh_valid_hit(distance[i], voxel[i], previous_roughness[i]) ? 1u : 0u;
}

// ---- one pt_render_sharc call (sharc_host.h run_call).  env = SceneData.EnvironmentLightColor; texels / tex_info / n_tex / maps / rot: as
// gb_pixels (gbuffer_host.cpp).  keys = null: the cache is off.
void sh_host_call(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                  const uint32_t* maps, const float* rot, const PtCamera* cam, const uint32_t* prm, const float* fprm, uint64_t* keys, uint32_t* accum,
                  uint32_t* resolved, float* out, uint64_t* counters)
{
    HostScene hs;
    hs.set(spheres, materials, n, env, texels, tex_info, n_tex, maps, rot);
    const Frame f(cam, prm, fprm);
    run_call(hs, cam, f, keys, reinterpret_cast<uint4*>(accum), reinterpret_cast<uint4*>(resolved), out, counters);
}

// ---- what a voxel's radiance estimates, sampled with the cache off: for every path (x, y) of the update grid and every frame index of
// frames[n_frames], the update path's own primary ray, then sh_path_radiance.  Per sample: key (0: the ray left the scene) and rgb.
void sh_host_estimates(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const PtCamera* cam, const uint32_t* prm, const float* fprm,
                       const uint32_t* frames, uint32_t n_frames, uint64_t* keys, float* rgb)
{
    HostScene hs;
    hs.set(spheres, materials, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    const Frame f(cam, prm, fprm);
    auto trace = [&](f3 o, f3 d, float tmin, float tmax, float& t, uint32_t& id) { hs.trace(o, d, tmin, tmax, t, id); };
    auto material = [&](uint32_t id, f3 o, f3 d, float t, bool primary) { return hs.material(id, o, d, t, primary); };
    auto envf = [&](f3 d) { return hs.environment(d); };
    const uint32_t gw = f.w / f.downscale, gh = f.h / f.downscale;
    size_t k = 0;
    for (uint32_t fi = 0; fi < n_frames; fi++)
        for (uint32_t y = 0; y < gh; y++)
            for (uint32_t x = 0; x < gw; x++, k++) {
                uint32_t rng = rng_init(x, y, frames[fi]);
                CameraParams cp = camera_params(*cam, gw, gh);
                cp.JitterX = cp.JitterY = rng_float(rng) - 0.5f;
                f3 o, d, radiance, P, N;
                float tmin, tmax;
                primary_ray(cp, x, y, o, d, tmin, tmax);
                keys[k] = 0u;
                rgb[3 * k] = rgb[3 * k + 1] = rgb[3 * k + 2] = 0.0f;
                if (!sh_path_radiance(f.fr, o, d, tmin, tmax, rng, trace, material, envf, radiance, P, N)) continue;
                float voxel;
                keys[k] = sh_key_at(f.g, P, N, voxel);
                rgb[3 * k] = radiance.x; rgb[3 * k + 1] = radiance.y; rgb[3 * k + 2] = radiance.z;
            }
}

}  // extern "C"
