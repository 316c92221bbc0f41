// restir_mis_host.cpp -- TEST SHIM: compiles spec S23's header paths (csrc/pt_restir.h: ri_initial_mis, invert_sphere_cone, the boiling
// filter; csrc/pt_light.h: bsdf_pdf_all) as plain host C++ (the flags of restir_host.cpp), so the tests can check them against the float64
// restatement without a GPU, and pt_restir_di_ex against them bit for bit.  Not part of the product; never loaded by it.
#include "restir_mis_host.h"

extern "C" {

void rm_host_call(const PtSphere* spheres, const PtMaterial* materials, uint32_t n, const float* texels, const uint32_t* tex_info, uint32_t n_tex, const uint32_t* maps,
                  const float* rot, const uint32_t* prm, const float* fprm, void* const* ptrs, const uint32_t* sprm, float cell_size, const uint32_t* cprm, float strength)
{
    RmHostScene hs;
    hs.set(spheres, materials, n, texels, tex_info, n_tex, maps, rot);
    rm_call(hs, prm, fprm, ptrs, sprm, cell_size, cprm, strength);
}

// count cone samples: in = {P[3], C[3], r, u1, u2} -> out = {L[3], inv_pdf, valid}
void rm_host_sample_cone(const float* in, uint32_t count, float* out)
{
    for (uint32_t i = 0; i < count; i++) {
        const float* a = in + 9u * i;
        const LightSample s = sample_sphere_cone(make_f3(a[0], a[1], a[2]), make_f3(a[3], a[4], a[5]), a[6], a[7], a[8]);
        float* o = out + 5u * i;
        o[0] = s.L.x; o[1] = s.L.y; o[2] = s.L.z; o[3] = s.inv_pdf; o[4] = s.valid ? 1.0f : 0.0f;
    }
}

// ... and their inverses: in = {P[3], C[3], r, L[3]} -> out = {u1, u2}
void rm_host_invert_cone(const float* in, uint32_t count, float* out)
{
    for (uint32_t i = 0; i < count; i++) {
        const float* a = in + 10u * i;
        invert_sphere_cone(make_f3(a[0], a[1], a[2]), make_f3(a[3], a[4], a[5]), a[6], make_f3(a[7], a[8], a[9]), out[2u * i], out[2u * i + 1u]);
    }
}

// surf = {base[3], metallic, roughness, ior, transmission, Ng[3], Ns[3], V[3]}; L[3 count] -> out[4 count] = {bsdf_pdf_all, and
// bsdf_pdf of the diffuse, specular and transmission lobes}; w_out[3]: the lobe weights
void rm_host_bsdf_pdf(const float* surf, const float* L, uint32_t count, float* out, float* w_out)
{
    const f3 Ng = make_f3(surf[7], surf[8], surf[9]), Ns = make_f3(surf[10], surf[11], surf[12]), V = make_f3(surf[13], surf[14], surf[15]);
    const bool front = dot(Ng, V) > 0.0f;
    const Surf s = surf_init(front, Ng, Ns);
    const Bsdf b = bsdf_init(make_f3(surf[0], surf[1], surf[2]), surf[3], surf[4], surf[5], surf[6], front);
    float w[3];
    lobe_weights(b, s, V, w);
    for (int k = 0; k < 3; k++) w_out[k] = w[k];
    for (uint32_t i = 0; i < count; i++) {
        const f3 l = make_f3(L[3u * i], L[3u * i + 1u], L[3u * i + 2u]);
        out[4u * i] = bsdf_pdf_all(b, s, l, V, w);
        for (int k = 0; k < 3; k++) out[4u * i + 1u + k] = bsdf_pdf(b, s, l, V, w, k);
    }
}

// the boiling filter over one block: w[64] -> the butterfly sum (returned), *n, flags[64] (1: emptied)
float rm_host_boiling(const float* w, float strength, uint32_t* n, uint32_t* flags)
{
    const float sum = ri_boiling_sum64(w, *n);
    const float mult = ri_boiling_multiplier(strength);
    for (uint32_t l = 0; l < 64u; l++) flags[l] = ri_boiled(w[l], sum, *n, mult) ? 1u : 0u;
    return sum;
}

float rm_host_boiling_multiplier(float strength) { return ri_boiling_multiplier(strength); }

}  // extern "C"
