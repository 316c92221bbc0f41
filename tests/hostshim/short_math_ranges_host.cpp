// short_math_ranges_host.cpp -- TEST SHIM: pt_math.h / pt_bsdf.h compiled as host C++ with PT_RANGED defined, so that every operand that
// reaches a call site of pt_sqrt_ranged / pt_rcp_ranged / pt_half_rcp_ranged passes through smr::probe first.  Per site (pt::RangedSite) it keeps
// the smallest and largest magnitude among the finite non-zero operands, and how many operands it saw (specials included).
// tests/test_short_math_ranges.py drives the shading step with random and adversarial inputs and holds the records against the contracts.
#include <cmath>
#include <cstdint>
#include <limits>

namespace smr {
constexpr int kMaxSites = 32;
float g_min[kMaxSites], g_max[kMaxSites];
uint64_t g_seen[kMaxSites], g_special[kMaxSites];
inline float probe(int site, float x)
{
    g_seen[site]++;
    const float a = std::fabs(x);
    if (!(a > 0.0f) || !std::isfinite(a)) { g_special[site]++; return x; }
    if (a < g_min[site]) g_min[site] = a;
    if (a > g_max[site]) g_max[site] = a;
    return x;
}
}  // namespace smr

#define PT_RANGED(site, x) smr::probe((int)(site), (x))
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_bsdf.h"

static_assert(pt::kRsCount <= smr::kMaxSites);

extern "C" {

int smr_site_count() { return pt::kRsCount; }

void smr_reset()
{
    for (int k = 0; k < smr::kMaxSites; k++) {
        smr::g_min[k] = std::numeric_limits<float>::infinity();
        smr::g_max[k] = 0.0f;
        smr::g_seen[k] = smr::g_special[k] = 0;
    }
}

void smr_get(float* mn, float* mx, uint64_t* seen, uint64_t* special)
{
    for (int k = 0; k < pt::kRsCount; k++) { mn[k] = smr::g_min[k]; mx[k] = smr::g_max[k]; seen[k] = smr::g_seen[k]; special[k] = smr::g_special[k]; }
}

// rows of 18 floats: base colour (3), metallic, roughness, ior, transmission, front (0 / 1), a (3), V (3), rnd (4).  The shading normal is
// normalize(a) -- get_basis_unit's premise -- and the step is the bounce loop's: surf_init_unit, lobe_weights, then, for the lobe the weights
// choose AND for each of the three lobes forced, bsdf_sample and bsdf_pdf_eval.
void smr_steps(uint32_t n, const float* rows)
{
    using namespace pt;
    for (uint32_t i = 0; i < n; i++) {
        const float* r = rows + (size_t)i * 18u;
        const bool front = r[7] != 0.0f;
        const f3 Ng = normalize(make_f3(r[8], r[9], r[10])), V = make_f3(r[11], r[12], r[13]);
        const Bsdf b = bsdf_init(make_f3(r[0], r[1], r[2]), r[3], r[4], r[5], r[6], front);
        const Surf s = surf_init_unit(front, Ng, front ? Ng : -Ng);
        float w[4][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
        lobe_weights(b, s, V, w[0]);
        for (int k = 0; k < 4; k++) {
            f3 L = make_f3(0, 0, 0), f;
            int lobe;
            float pdf;
            if (bsdf_sample(b, s, V, w[k], r + 14, L, lobe)) (void)bsdf_pdf_eval(b, s, L, V, w[k], lobe, pdf, f);
            // the evaluation alone too, for a direction the sampler did not choose (rnd as a direction: any L may be asked about)
            (void)bsdf_pdf_eval(b, s, make_f3(r[14] - 0.5f, r[15] - 0.5f, r[16] - 0.5f), V, w[k], k == 0 ? kLobeSpecular : k - 1, pdf, f);
        }
    }
}

// rows of 2 floats: u0, u1 of cosine_ray
void smr_cosine(uint32_t n, const float* rows)
{
    for (uint32_t i = 0; i < n; i++) (void)pt::cosine_ray(rows[2 * i], rows[2 * i + 1]);
}

}
