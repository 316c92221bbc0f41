// lightris_sanitize.cpp -- csrc/pt_lightris.h and the initial sampling of csrc/pt_restir.h that consumes it, compiled as host C++ and
// run under AddressSanitizer + UBSan as a stand-alone program (a CPU test builds and runs it; no sanitizer is ever loaded into Python).
// Every array is a heap allocation of exactly the size the spec gives it, so an index past a level, a tile or a cell is an error
// here: pyramids of 1, 5, 17 and 1025 emitters, tiles that are no power of two, ReGIR grids of 2^3 and 3^3 cells, and whole calls
// in the three modes over a small G-buffer written by hand (surfaces inside and outside the grid).
#include "../hostshim/lightris_host.cpp"  // the tests' shim itself (its lr_host_call is what a whole call runs through)
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
    const uint32_t n = n_lights + 1u;
    spheres.assign(n, PtSphere{});
    mats.assign(n, PtMaterial{});
    uint32_t rng = 12345u;
    auto unit = [&]() { return rng_float(rng); };
    for (uint32_t i = 0; i < n; i++) {
        PtMaterial& m = mats[i];
        m.BaseColor[0] = m.BaseColor[1] = m.BaseColor[2] = 0.6f; m.BaseColor[3] = 1.0f;
        m.Roughness = 0.6f; m.IOR = 1.5f;
        float* s = reinterpret_cast<float*>(&spheres[i]);
        if (i == 0) { s[0] = 0.0f; s[1] = -1000.0f; s[2] = 0.0f; s[3] = 1000.0f; continue; }
        s[0] = 12.0f * unit() - 6.0f; s[1] = 0.5f + 5.0f * unit(); s[2] = 12.0f * unit() - 4.0f; s[3] = 0.05f + 0.25f * unit();
        m.EmissiveStrength = 0.1f + 100.0f * unit() * unit();
        m.EmissiveColor[0] = 0.1f + 0.9f * unit(); m.EmissiveColor[1] = 0.1f + 0.9f * unit(); m.EmissiveColor[2] = 0.1f + 0.9f * unit();
    }
}

void structures(uint32_t n_lights, uint32_t tile_size, uint32_t tile_count, uint32_t grid, uint32_t lights_per_cell, uint32_t build_samples)
{
    std::vector<PtSphere> spheres;
    std::vector<PtMaterial> mats;
    make_scene(n_lights, spheres, mats);
    LrHostScene hs;
    hs.set(spheres.data(), mats.data(), (uint32_t)spheres.size());
    check(hs.lights.size() == n_lights, "emitter count");
    float* powers = new float[n_lights];
    for (uint32_t j = 0; j < n_lights; j++) powers[j] = lr_light_power(hs.sph.data(), hs.mats.data(), hs.lights.data(), j);
    const uint32_t lv = lr_levels(n_lights);
    float* pyramid = new float[lr_pyramid_floats(lv)];
    lr_host_build_pyramid(powers, n_lights, pyramid);
    check(pyramid[lr_level_offset(lv, lv)] > 0.0f, "the top of the pyramid is positive");
    LrEntry* power = new LrEntry[(size_t)tile_size * tile_count];
    lr_host_build_power(pyramid, n_lights, tile_size, tile_count, 7u, power);
    for (size_t i = 0; i < (size_t)tile_size * tile_count; i++) check(power[i].light < n_lights && power[i].inv_pdf >= 1.0f, "a Power_RIS entry is a real emitter");
    LrGrid g{};
    g.cam = make_f3(0.5f, 2.0f, -3.0f); g.grid = grid; g.cell_size = 2.5f; g.lights_per_cell = lights_per_cell; g.build_samples = build_samples;
    g.tile_size = tile_size; g.tile_count = tile_count;
    const size_t n_regir = (size_t)grid * grid * grid * lights_per_cell;
    LrEntry* regir = new LrEntry[n_regir];
    lr_host_build_regir(hs, g, power, 7u, regir);
    size_t valid = 0;
    for (size_t i = 0; i < n_regir; i++) {
        check(regir[i].light == kLrInvalid || (regir[i].light < n_lights && regir[i].inv_pdf > 0.0f), "a ReGIR entry is a real emitter or invalid");
        valid += regir[i].light != kLrInvalid;
    }
    check(valid == n_regir, "every emitter has a positive volume target: every slot selects");
    delete[] regir; delete[] power; delete[] pyramid; delete[] powers;
}

// whole calls over a G-buffer of w x h points of the ground plane y = 0 seen from above
void calls(uint32_t mode)
{
    const uint32_t w = 19, h = 5, n = w * h;
    std::vector<PtSphere> spheres;
    std::vector<PtMaterial> mats;
    make_scene(9, spheres, mats);
    float* gbuf[8];
    const uint32_t width[8] = { 4, 2, 1, 3, 4, 4, 1, 1 };
    for (int k = 0; k < 8; k++) gbuf[k] = new float[(size_t)n * width[k]]();
    const float cam[3] = { 0.0f, 6.0f, 0.0f };
    for (uint32_t i = 0; i < n; i++) {
        const float x = -9.0f + (float)(i % w), z = -2.0f + (float)(i / w);  // some points outside a 4^3 grid of 2.5 around the camera
        gbuf[0][4 * i] = x; gbuf[0][4 * i + 1] = 0.0f; gbuf[0][4 * i + 2] = z; gbuf[0][4 * i + 3] = 1e-3f;
        gbuf[1][2 * i] = 0.0f; gbuf[1][2 * i + 1] = 1.0f;  // octahedral (0, 1, 0)
        gbuf[2][i] = i == 3 ? kInf : 6.0f;                 // one pixel without a surface
        gbuf[4][4 * i] = gbuf[4][4 * i + 1] = gbuf[4][4 * i + 2] = 0.6f;
        gbuf[5][4 * i + 1] = 1.0f; gbuf[5][4 * i + 3] = 0.6f;
        gbuf[6][i] = 1.5f;
    }
    float* slots[2][7];
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < 7; k++) slots[s][k] = new float[(size_t)n * (k == 4 ? 1 : 4)]();
    float* out_d = new float[4 * (size_t)n]();
    float* out_s = new float[4 * (size_t)n]();
    uint32_t lit = 0;
    for (uint32_t f = 0; f < 3; f++) {
        const uint32_t prm[12] = { w, h, f, 8, 1, 1, 20, 1, 1, 2, f ? 1u : 0u, 3 };
        const float fprm[7] = { 4.0f, cam[0], cam[1], cam[2], cam[0], cam[1], cam[2] };
        const uint32_t sprm[6] = { mode, 100, 3, 4, 33, 4 };
        void* ptrs[24];
        for (int k = 0; k < 8; k++) ptrs[k] = gbuf[k];
        for (int k = 0; k < 7; k++) { ptrs[8 + k] = slots[f & 1][k]; ptrs[15 + k] = slots[(f & 1) ^ 1][k]; }
        ptrs[22] = out_d; ptrs[23] = out_s;
        float* pyramid = new float[lr_pyramid_floats(lr_levels(9))];
        LrEntry* ris = new LrEntry[100 * 3 + (mode == kLrRegirRis ? 64 * 33 : 0)];
        lr_host_call(spheres.data(), mats.data(), (uint32_t)spheres.size(), prm, fprm, ptrs, sprm, 2.5f, mode ? pyramid : nullptr, mode ? ris : nullptr);
        for (uint32_t i = 0; i < n; i++) lit += out_d[4 * i] > 0.0f;
        delete[] ris; delete[] pyramid;
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
    structures(1, 7, 3, 2, 5, 1);
    structures(5, 100, 3, 2, 70, 8);
    structures(17, 64, 4, 3, 256, 32);
    structures(1025, 129, 2, 2, 33, 4);
    for (uint32_t mode = 0; mode < 3; mode++) calls(mode);
    if (failures) return 1;
    std::printf("lightris_sanitize ok\n");
    return 0;
}
