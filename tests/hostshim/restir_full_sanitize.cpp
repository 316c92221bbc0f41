// restir_full_sanitize.cpp -- spec S26's header paths (csrc/pt_restir.h: the visibility word through launch 1 and the spatial pass,
// ri_final_reuse, pairwise MIS in both reuse passes) compiled as host C++ and run under AddressSanitizer + UBSan as a stand-alone program
// (a CPU test builds and runs it; no sanitizer is ever loaded into Python).  Every array is a heap allocation of exactly its size: the
// per-sphere alpha classes and emitter index, the history slots, a G-buffer whose size is no multiple of 8 on either axis, and motion
// vectors that send some pixels' reprojection outside the image and some offsets beyond an axis' range.
#include "restir_full_host.cpp"  // the tests' shim itself (its rf_host_call is what a whole call runs through)
#include <cstdio>
#include <cstdlib>

namespace {

int failures = 0;
void check(bool ok, const char* what)
{
    if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

void make_scene(uint32_t n_lights, std::vector<PtSphere>& spheres, std::vector<PtMaterial>& mats)
{
    const uint32_t n = n_lights + 2u;  // ground, emitters, and a last sphere that is no emitter
    spheres.assign(n, PtSphere{});
    mats.assign(n, PtMaterial{});
    uint32_t rng = 4321u;
    auto unit = [&]() { return rng_float(rng); };
    for (uint32_t i = 0; i < n; i++) {
        PtMaterial& m = mats[i];
        m.BaseColor[0] = m.BaseColor[1] = m.BaseColor[2] = 0.6f; m.BaseColor[3] = 1.0f;
        m.Roughness = 0.3f; m.IOR = 1.5f;
        float* s = reinterpret_cast<float*>(&spheres[i]);
        if (i == 0) { s[0] = 0.0f; s[1] = -1000.0f; s[2] = 0.0f; s[3] = 1000.0f; continue; }
        s[0] = 12.0f * unit() - 6.0f; s[1] = 1.0f + 4.0f * unit(); s[2] = 12.0f * unit() - 4.0f; s[3] = 0.3f + 0.6f * unit();
        if (i == n - 1u) continue;
        m.EmissiveStrength = 0.1f + 100.0f * unit() * unit();
        m.EmissiveColor[0] = 0.1f + 0.9f * unit(); m.EmissiveColor[1] = 0.1f + 0.9f * unit(); m.EmissiveColor[2] = 0.1f + 0.9f * unit();
    }
}

void word_steps()
{
    uint32_t rng = 7u;
    uint32_t word = rf_host_vis_fresh();
    for (uint32_t k = 0; k < 5000u; k++) {
        const int dx = (int)(rng_next(rng) % 1201u) - 600, dy = (int)(rng_next(rng) % 61u) - 30;
        const uint32_t next = rf_host_vis_moved(word, dx, dy);
        check((next & 1u) == 1u && (next >> 24) == 0u, "the bit stays and the top byte stays clear");
        if (((word >> 8) & 0xFFu) == 0u) check(((next >> 8) & 0xFFu) == 0u, "a saturated axis stays saturated");
        word = k % 97u == 0u ? rf_host_vis_fresh() : next;
        (void)rf_host_vis_usable(1u, k % 256u, (float)(k % 40u), k % 300u, word);
    }
    check(rf_host_vis_moved(rf_host_vis_fresh(), 2147483647, -2147483647 - 1) == 1u, "the largest steps saturate both axes");
}

// whole calls over a G-buffer of w x h points of the ground plane y = 0 seen from above
void calls(uint32_t mode, uint32_t brdf, uint32_t filter, uint32_t tbias, uint32_t sbias, uint32_t reuse)
{
    const uint32_t w = 19, h = 13, n = w * h;
    std::vector<PtSphere> spheres;
    std::vector<PtMaterial> mats;
    make_scene(9, spheres, mats);
    float* gbuf[8];
    const uint32_t width[8] = { 4, 2, 1, 3, 4, 4, 1, 1 };
    for (int k = 0; k < 8; k++) gbuf[k] = new float[(size_t)n * width[k]]();
    const float cam[3] = { 0.0f, 6.0f, 0.0f };
    for (uint32_t i = 0; i < n; i++) {
        const float x = -9.0f + (float)(i % w), z = -6.0f + (float)(i / w);
        gbuf[0][4 * i] = x; gbuf[0][4 * i + 1] = 0.0f; gbuf[0][4 * i + 2] = z; gbuf[0][4 * i + 3] = 1e-3f;
        gbuf[1][2 * i] = 0.0f; gbuf[1][2 * i + 1] = 1.0f;  // octahedral (0, 1, 0)
        gbuf[2][i] = i % 7u == 3u ? kInf : 6.0f;           // pixels without a surface inside every block
        gbuf[3][3 * i] = i % 11u == 0u ? 40.0f : (i % 3u == 0u ? -2.0f : 0.0f);  // reprojection: outside the image, two pixels away, in place
        gbuf[3][3 * i + 1] = i % 13u == 0u ? -40.0f : 0.0f;
        gbuf[4][4 * i] = gbuf[4][4 * i + 1] = gbuf[4][4 * i + 2] = 0.6f;
        gbuf[5][4 * i + 1] = 1.0f; gbuf[5][4 * i + 3] = 0.3f;
        gbuf[6][i] = 1.5f;
        gbuf[7][i] = i % 5u == 0u ? 0.5f : 0.0f;
    }
    float* slots[2][7];
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < 7; k++) slots[s][k] = new float[(size_t)n * (k == 4 ? 1 : 4)]();
    float* out_d = new float[4 * (size_t)n]();
    float* out_s = new float[4 * (size_t)n]();
    uint64_t* counters = new uint64_t[4]();
    uint32_t lit = 0;
    uint64_t free_pixels = 0;
    for (uint32_t f = 0; f < 4; f++) {
        const uint32_t prm[12] = { w, h, f, 8, 1, tbias, 20, 1, sbias, 3, f ? 1u : 0u, 3 };
        const float fprm[7] = { 7.0f, cam[0], cam[1], cam[2], cam[0], cam[1], cam[2] };
        const uint32_t sprm[6] = { mode, 100, 3, 4, 33, 4 };
        const uint32_t cprm[2] = { brdf, filter };
        const uint32_t shprm[2] = { reuse, 4 };
        void* ptrs[24];
        for (int k = 0; k < 8; k++) ptrs[k] = gbuf[k];
        for (int k = 0; k < 7; k++) { ptrs[8 + k] = slots[f & 1][k]; ptrs[15 + k] = slots[(f & 1) ^ 1][k]; }
        ptrs[22] = out_d; ptrs[23] = out_s;
        rf_host_call(spheres.data(), mats.data(), (uint32_t)spheres.size(), nullptr, nullptr, 0, nullptr, nullptr, prm, fprm, ptrs, sprm, 2.5f, cprm, 0.2f, shprm, 16.0f,
                     counters);
        for (uint32_t i = 0; i < n; i++) lit += out_d[4 * i] > 0.0f;
        free_pixels += counters[3];
    }
    check(lit > 0, "some pixel received direct light");
    check(out_d[4 * 3] == 0.0f && out_d[4 * 3 + 3] == 0.0f, "a pixel without a surface is not written");
    check(reuse ? free_pixels > 0 : free_pixels == 0, "final rays are skipped exactly where reuse is on");
    delete[] counters;
    delete[] out_s; delete[] out_d;
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < 7; k++) delete[] slots[s][k];
    for (int k = 0; k < 8; k++) delete[] gbuf[k];
}

}  // namespace

int main()
{
    word_steps();
    for (uint32_t mode = 0; mode < 3; mode++) {
        calls(mode, 1, 1, 2, 2, 1);
        calls(mode, 0, 0, 2, 1, 0);
        calls(mode, 0, 1, 3, 2, 1);
    }
    calls(0, 8, 1, 1, 1, 1);
    calls(0, 0, 0, 1, 3, 0);
    if (failures) return 1;
    std::printf("restir_full_sanitize ok\n");
    return 0;
}
