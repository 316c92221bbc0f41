// restir_mis_sanitize.cpp -- spec S23's header paths (csrc/pt_restir.h: ri_initial_mis, invert_sphere_cone, the boiling filter over
// whole 8x8 blocks; csrc/pt_light.h: bsdf_pdf_all) compiled as host C++ and run under AddressSanitizer + UBSan as a stand-alone program
// (a CPU test builds and runs it; no sanitizer is ever loaded into Python).  Every array is a heap allocation of exactly the size the
// spec gives it: the per-sphere emitter index, the pyramid, the tiles and cells, and a G-buffer whose size is no multiple of 8 on either
// axis, so that the lanes of an edge block outside the image, which take part in the filter's sum, must not touch memory.
#include "../hostshim/restir_mis_host.cpp"  // the tests' shim itself (its rm_host_call is what a whole call runs through)
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
    const uint32_t n = n_lights + 2u;  // ground, emitters, and a last sphere that is no emitter (its emitter index is "none")
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

void round_trips()
{
    uint32_t rng = 99u;
    float* in = new float[9];
    float* out = new float[5];
    float* inv_in = new float[10];
    float* u = new float[2];
    for (uint32_t k = 0; k < 2000u; k++) {
        for (int c = 0; c < 3; c++) { in[c] = 8.0f * rng_float(rng) - 4.0f; in[3 + c] = 8.0f * rng_float(rng) - 4.0f; }
        in[6] = 0.01f + 3.0f * rng_float(rng);  // (some points lie inside the sphere: the sample is invalid and the inverse is (1, 1))
        in[7] = rng_float(rng); in[8] = rng_float(rng);
        rm_host_sample_cone(in, 1, out);
        for (int c = 0; c < 7; c++) inv_in[c] = in[c];
        for (int c = 0; c < 3; c++) inv_in[7 + c] = out[c];
        rm_host_invert_cone(inv_in, 1, u);
        check(u[0] > 0.0f && u[0] <= 1.0f && u[1] > 0.0f && u[1] <= 1.0f, "an inverted sample lies in (0, 1]");
    }
    delete[] u; delete[] inv_in; delete[] out; delete[] in;
}

void filter_blocks()
{
    float* w = new float[64];
    uint32_t* flags = new uint32_t[64];
    for (int l = 0; l < 64; l++) w[l] = 1.0f;
    w[17] = 200.0f;
    uint32_t n = 0;
    const float sum = rm_host_boiling(w, 0.2f, &n, flags);
    check(sum == 263.0f && n == 64u, "the block's sum and count");
    uint32_t emptied = 0;
    for (int l = 0; l < 64; l++) emptied += flags[l];
    check(emptied == 1u && flags[17] == 1u, "the one over-weighted lane is emptied");
    delete[] flags; delete[] w;
}

// whole calls over a G-buffer of w x h points of the ground plane y = 0 seen from above
void calls(uint32_t mode, uint32_t brdf, uint32_t filter)
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
        gbuf[4][4 * i] = gbuf[4][4 * i + 1] = gbuf[4][4 * i + 2] = 0.6f;
        gbuf[5][4 * i + 1] = 1.0f; gbuf[5][4 * i + 3] = 0.3f;
        gbuf[6][i] = 1.5f;
        gbuf[7][i] = i % 5u == 0u ? 0.5f : 0.0f;           // some surfaces with a transmission lobe
    }
    float* slots[2][7];
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < 7; k++) slots[s][k] = new float[(size_t)n * (k == 4 ? 1 : 4)]();
    float* out_d = new float[4 * (size_t)n]();
    float* out_s = new float[4 * (size_t)n]();
    uint32_t lit = 0;
    for (uint32_t f = 0; f < 3; f++) {
        const uint32_t prm[12] = { w, h, f, 8, 1, 3, 20, 1, 1, 2, f ? 1u : 0u, 3 };
        const float fprm[7] = { 4.0f, cam[0], cam[1], cam[2], cam[0], cam[1], cam[2] };
        const uint32_t sprm[6] = { mode, 100, 3, 4, 33, 4 };
        const uint32_t cprm[2] = { brdf, filter };
        void* ptrs[24];
        for (int k = 0; k < 8; k++) ptrs[k] = gbuf[k];
        for (int k = 0; k < 7; k++) { ptrs[8 + k] = slots[f & 1][k]; ptrs[15 + k] = slots[(f & 1) ^ 1][k]; }
        ptrs[22] = out_d; ptrs[23] = out_s;
        rm_host_call(spheres.data(), mats.data(), (uint32_t)spheres.size(), nullptr, nullptr, 0, nullptr, nullptr, prm, fprm, ptrs, sprm, 2.5f, cprm, 0.2f);
        for (uint32_t i = 0; i < n; i++) lit += out_d[4 * i] > 0.0f;
    }
    check(lit > 0, "some pixel received direct light");
    check(out_d[4 * 3] == 0.0f && out_d[4 * 3 + 3] == 0.0f, "a pixel without a surface is not written");
    delete[] out_s; delete[] out_d;
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < 7; k++) delete[] slots[s][k];
    for (int k = 0; k < 8; k++) delete[] gbuf[k];
}

}  // namespace

int main()
{
    round_trips();
    filter_blocks();
    for (uint32_t mode = 0; mode < 3; mode++) {
        calls(mode, 1, 0);
        calls(mode, 8, 1);
        calls(mode, 0, 1);
    }
    calls(0, 0, 0);
    if (failures) return 1;
    std::printf("restir_mis_sanitize ok\n");
    return 0;
}
