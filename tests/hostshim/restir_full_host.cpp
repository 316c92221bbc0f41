// restir_full_host.cpp -- TEST SHIM: compiles spec S26's header paths (csrc/pt_restir.h: the visibility word, ri_final_reuse, pairwise
// MIS) as plain host C++ (the flags of restir_mis_host.cpp), so the tests can check them against the float64 restatement and known
// answers without a GPU, and pt_restir_di_full against them bit for bit.  Not part of the product; never loaded by it.
#include "restir_full_host.h"

extern "C" {

// counters: four uint64 (RfCounters) or null
void rf_host_call(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* texels, const uint32_t* tex_info, uint32_t n_tex, const uint32_t* maps,
                  const float* rot, const uint32_t* prm, const float* fprm, void* const* ptrs, const uint32_t* sprm, float cell_size, const uint32_t* cprm, float strength,
                  const uint32_t* shprm, float max_distance, uint64_t* counters)
{
    RmHostScene hs;
    hs.set(spheres, materials, n, texels, tex_info, n_tex, maps, rot);
    rf_call(hs, prm, fprm, ptrs, sprm, cell_size, cprm, strength, shprm, max_distance, reinterpret_cast<RfCounters*>(counters));
}

uint32_t rf_host_vis_fresh() { return kRiVisFresh; }

uint32_t rf_host_vis_moved(uint32_t vis, int dx, int dy) { return ri_vis_moved(vis, dx, dy); }

// the gate of final shading but for the emitter's alpha class
uint32_t rf_host_vis_usable(uint32_t reuse, uint32_t max_age, float max_distance, uint32_t age, uint32_t vis)
{
    RiShading sh{};
    sh.reuse = reuse; sh.max_age = max_age; sh.max_dist2 = max_distance * max_distance;
    RiReservoir r = ri_empty_reservoir();
    r.age = age; r.vis = vis;
    return ri_vis_usable(sh, r) ? 1u : 0u;
}

// The pairwise weights of one pixel from numbers: the canonical (M_c, W_c, pc_yc = p_c(y_c)) against k neighbours, neighbour i given as
// nb[5 i ..] = {M_i, W_i, p_i(y_i), p_c(y_i), p_i(y_c)} -> out[0 .. k - 1] the neighbours' stream weights, out[k] the canonical's
void rf_host_pairwise(uint32_t k, float M_c, float W_c, float pc_yc, const float* nb, float* out)
{
    RiPairwise pw = ri_pairwise_begin(M_c, k);
    for (uint32_t i = 0; i < k; i++) {
        const float* a = nb + 5u * i;
        out[i] = ri_pairwise_neighbour(pw, a[0], a[1], a[2], a[3]);
        pw.m_c += ri_pairwise_canonical_term(pw, a[0], pc_yc, a[4]);
    }
    out[k] = (pc_yc * W_c) * (pw.m_c / pw.kf);
}

}  // extern "C"
