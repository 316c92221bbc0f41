// denoiser_host.cpp -- TEST SHIM: the lobe split of row N7 (csrc/pt_light.h bsdf_eval_reflective_lobes, DESIGN.md spec S13) compiled
// as host C++ for tests/test_denoiser_split.py.  Not part of the product; never loaded by it.
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_light.h"

using namespace pt;

extern "C" {

// One evaluation per row of `in` (17 floats: BaseColor rgb, Metallic, Roughness, IOR, Transmission, front, N xyz, V xyz, L xyz; unit
// vectors).  out, 18 floats per row: bsdf_eval_reflective, its diffuse half, its specular half, and the estimates di_estimate forms
// from them, (le * f) * k, (le * f_d) * k, (le * f_s) * k, for le = `le` and k = `k`.
void dn_lobes(const float* in, uint32_t n, const float* le3, float k, float* out)
{
    const f3 le = make_f3(le3[0], le3[1], le3[2]);
    for (uint32_t i = 0; i < n; i++) {
        const float* p = in + (size_t)i * 17u;
        const bool front = p[7] != 0.0f;
        const f3 N = make_f3(p[8], p[9], p[10]), V = make_f3(p[11], p[12], p[13]), L = make_f3(p[14], p[15], p[16]);
        const Bsdf b = bsdf_init(make_f3(p[0], p[1], p[2]), p[3], p[4], p[5], p[6], front);
        const Surf s = surf_init(front, N, front ? N : -N);
        float w[3];
        lobe_weights(b, s, V, w);
        const f3 f = bsdf_eval_reflective(b, s, L, V, w);
        f3 fd, fs;
        bsdf_eval_reflective_lobes(b, s, L, V, w, fd, fs);
        const f3 r[6] = { f, fd, fs, (le * f) * k, (le * fd) * k, (le * fs) * k };
        float* o = out + (size_t)i * 18u;
        for (int j = 0; j < 6; j++) { o[3 * j] = r[j].x; o[3 * j + 1] = r[j].y; o[3 * j + 2] = r[j].z; }
    }
}

}  // extern "C"
