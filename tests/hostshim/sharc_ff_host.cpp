// sharc_ff_host.cpp -- TEST SHIM: csrc/pt_sharc.h's anti-firefly filter (row N19, DESIGN.md spec S25) compiled as plain host C++ (the flags
// of sharc_ex_host.cpp), so that the tests can check the clamp and the weight threshold without a GPU and the GPU kernels against them
// bit for bit.  Not part of the product; never loaded by it.
#include "sharc_ff_host.h"

using namespace shhost;

extern "C" {

// one pt_render_sharc_ex call: the arguments of sh_host_call_ex (sharc_ex_host.cpp), then IsAntiFireflyEnabled and
// ff_counters = {slots the resolve clamped, walks the weight threshold stopped}
void sh_host_call_ff(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* env, const float* texels, const uint32_t* tex_info, uint32_t n_tex,
                     const uint32_t* maps, const float* rot, const PtCamera* cam, const uint32_t* prm, const float* fprm, uint64_t* keys, uint32_t* accum,
                     uint32_t* resolved, float* out, uint64_t* counters, const float* di_diffuse, const float* di_specular, uint32_t mode, float* spec_hit_dist,
                     float* diffuse, float* specular, uint32_t ff, uint64_t* ff_counters)
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
    run_call_ff(hs, cam, f, keys, reinterpret_cast<uint4*>(accum), reinterpret_cast<uint4*>(resolved), out, counters, x, ff != 0, ff_counters);
}

// n voxels through sh_resolve_slot_ff: out / clear as sh_host_resolve (sharc_host.cpp); clamped_acc = the accumulators behind the clamp
// (what the join sees), clamped[i] = the clamp acted
void sh_host_resolve_ff(const uint32_t* acc, const uint32_t* prev, uint32_t n, uint32_t accumulation_frames, uint32_t max_stale_frames, uint32_t* out, uint32_t* clear,
                        uint32_t* clamped_acc, uint32_t* clamped)
{
    for (uint32_t i = 0; i < n; i++) {
        bool c;
        const uint4 a = reinterpret_cast<const uint4*>(acc)[i], p = reinterpret_cast<const uint4*>(prev)[i];
        reinterpret_cast<uint4*>(out)[i] = sh_resolve_slot_ff(a, p, accumulation_frames, max_stale_frames, c);
        clear[i] = c ? 1u : 0u;
        uint4 b = a;
        clamped[i] = sh_ff_clamp(b, p) ? 1u : 0u;
        reinterpret_cast<uint4*>(clamped_acc)[i] = b;
    }
}

void sh_host_luminance(const float* rgb, uint32_t n, float* y)
{
    for (uint32_t i = 0; i < n; i++) y[i] = sh_luminance(make_f3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
}

// a hand-built ShState (slots, weights: 3 floats per vertex, nearest first; length; skipped), optionally sh_set_throughput(T) first
// (T = null: not called), then `radiance` back through sh_propagate (ff = 0) or sh_propagate_ff into accum (capacity voxels).
// stopped: the state's count afterwards; weight0: st.weight[0] as the walk saw it
void sh_host_propagate(const uint32_t* slots, const float* weights, uint32_t length, uint32_t skipped, const float* T, const float* radiance, uint32_t* accum,
                       uint32_t capacity, uint32_t ff, uint32_t* stopped, float* weight0)
{
    ShMap m{};
    m.accum = reinterpret_cast<uint4*>(accum); m.capacity = capacity;
    ShState st;
    st.length = length; st.skipped = skipped != 0; st.stopped = 0u;
    for (uint32_t i = 0; i < kShPropagationDepth - 1u; i++) { st.slot[i] = slots[i]; st.weight[i] = make_f3(weights[3 * i], weights[3 * i + 1], weights[3 * i + 2]); }
    if (T) sh_set_throughput(st, make_f3(T[0], T[1], T[2]));
    const f3 r = make_f3(radiance[0], radiance[1], radiance[2]);
    if (ff) sh_propagate_ff(m, st, r);
    else sh_propagate(m, st, r);
    *stopped = st.stopped;
    weight0[0] = st.weight[0].x; weight0[1] = st.weight[0].y; weight0[2] = st.weight[0].z;
}

// one vertex through sh_update_hit_t<ff> on a state as above over a caller-owned map: the vertex's own (emission, 1 sample) and the walk
void sh_host_update_hit(uint64_t* keys, uint32_t* accum, uint32_t* resolved, uint32_t capacity, const float* cam_pos, float scene_scale, const uint32_t* slots,
                        const float* weights, uint32_t length, const float* P, const float* N, const float* emission, float rnd, uint32_t ff, uint32_t* slot_out,
                        uint32_t* stopped)
{
    ShMap m{};
    m.keys = keys; m.accum = reinterpret_cast<uint4*>(accum); m.resolved = reinterpret_cast<uint4*>(resolved); m.capacity = capacity;
    ShGrid g{};
    g.cam_pos = make_f3(cam_pos[0], cam_pos[1], cam_pos[2]);
    g.scene_scale = scene_scale;
    ShState st;
    st.length = length; st.skipped = false; st.stopped = 0u;
    for (uint32_t i = 0; i < kShPropagationDepth - 1u; i++) { st.slot[i] = slots[i]; st.weight[i] = make_f3(weights[3 * i], weights[3 * i + 1], weights[3 * i + 2]); }
    uint32_t failed = 0;
    const f3 p = make_f3(P[0], P[1], P[2]), nrm = make_f3(N[0], N[1], N[2]), e = make_f3(emission[0], emission[1], emission[2]);
    if (ff) (void)sh_update_hit_t<true>(g, m, st, p, nrm, e, rnd, failed);
    else (void)sh_update_hit_t<false>(g, m, st, p, nrm, e, rnd, failed);
    *slot_out = failed ? kShNoSlot : st.slot[0];
    *stopped = st.stopped;
}

}  // extern "C"
