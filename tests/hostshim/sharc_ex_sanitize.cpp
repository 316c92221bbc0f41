// sharc_ex_sanitize.cpp -- TEST PROGRAM: csrc/pt_sharc.h's update, resolve and query with a DI (row N18, DESIGN.md spec S24) in the three
// denoiser modes and without one, three frames each, stand-alone, so that tests/test_sharc_ex.py can build it with
// -fsanitize=address,undefined and run it as a child process.  The DI has zeros, a NaN, an inf and a negative texel; the buffers are
// exactly as large as the contract says, so a read or write outside them is the sanitizer's finding.  Exit status 0 = every invariant held.
#include "sharc_ex_host.h"
#include <cstdio>
#include <limits>

using namespace shhost;

static PtCamera camera(float x, float y, float z)
{
    PtCamera c{};
    c.Position[0] = x; c.Position[1] = y; c.Position[2] = z;
    c.RightDirection[0] = 1.5f; c.UpDirection[1] = 1.0f; c.ForwardDirection[2] = 1.0f;
    c.NearDepth = 0.01f; c.FarDepth = kInf;
    return c;
}

static int run(uint32_t mode, bool alias)
{
    const uint32_t n = 5, w = 24, h = 16, capacity = 1u << 12;
    PtSphere sp[n] = { { 0.0f, -1000.0f, 0.0f, 1000.0f }, { -1.5f, 1.0f, 0.0f, 1.0f }, { 1.5f, 0.8f, 0.5f, 0.8f }, { 0.0f, 3.0f, 1.0f, 0.5f }, { 0.0f, 0.6f, -1.5f, 0.6f } };
    PtMaterial mt[n] = {};
    for (uint32_t i = 0; i < n; i++) {
        mt[i].BaseColor[0] = 0.3f + 0.15f * (float)i; mt[i].BaseColor[1] = 0.6f; mt[i].BaseColor[2] = 0.8f - 0.15f * (float)i; mt[i].BaseColor[3] = 1.0f;
        mt[i].Roughness = 0.5f; mt[i].IOR = 1.5f;
    }
    mt[2].Metallic = 1.0f; mt[2].Roughness = 0.1f;
    mt[3].EmissiveStrength = 10.0f; mt[3].EmissiveColor[0] = 1.0f; mt[3].EmissiveColor[1] = 0.9f; mt[3].EmissiveColor[2] = 0.7f;
    mt[4].Transmission = 1.0f; mt[4].Roughness = 0.05f;
    const float env[4] = { 0.2f, 0.25f, 0.3f, 1.0f };
    HostScene hs;
    hs.set(sp, mt, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    std::vector<uint64_t> keys(capacity, 0);
    std::vector<uint4> a(capacity), b(capacity);
    std::memset(a.data(), 0, capacity * sizeof(uint4));
    std::memset(b.data(), 0, capacity * sizeof(uint4));
    const size_t px = (size_t)w * h;
    std::vector<float> out(px * 4u), shd(px), dif(px * 4u), spe(px * 4u), did(px * 4u), dis(px * 4u);
    uint4 *accum = a.data(), *resolved = b.data();
    uint32_t written = 0;
    for (uint32_t frame = 0; frame < 3; frame++) {
        for (size_t i = 0; i < px; i++) {
            const float v = (i % 7u == 0u) ? 0.0f : 0.05f * (float)(i % 13u);
            for (int k = 0; k < 3; k++) { did[4 * i + k] = v; dis[4 * i + k] = 0.5f * v; }
            did[4 * i + 3] = dis[4 * i + 3] = 3.0f;
        }
        did[4 * 5] = std::numeric_limits<float>::quiet_NaN();
        did[4 * 9 + 1] = kInf;
        dis[4 * 11 + 2] = -2.0f;
        for (size_t i = 0; i < px; i++) shd[i] = -1.0f;
        if (!alias) for (size_t i = 0; i < 4 * px; i++) dif[i] = spe[i] = -1.0f;
        const PtCamera cam = camera(frame == 2 ? 0.5f : 0.0f, 1.5f, -6.0f);
        const uint32_t prm[16] = { w, h, frame, 6, 2, 1, capacity, 2, 4, 8, 0, 7, 0, 0, w, h };
        const float fprm[3] = { 1e-3f, 50.0f, 0.4f };
        const Frame f(&cam, prm, fprm);
        Extras x;
        x.di_diffuse = reinterpret_cast<const float4*>(did.data());
        x.di_specular = reinterpret_cast<const float4*>(dis.data());
        x.mode = mode;
        x.spec_hit_dist = mode == 1 ? shd.data() : nullptr;
        x.diffuse = mode >= 2 ? reinterpret_cast<float4*>(alias ? did.data() : dif.data()) : nullptr;
        x.specular = mode >= 2 ? reinterpret_cast<float4*>(alias ? dis.data() : spe.data()) : nullptr;
        uint64_t counters[2];
        run_call_ex(hs, &cam, f, keys.data(), accum, resolved, out.data(), counters, x);
        std::swap(accum, resolved);
        if (counters[1]) { std::printf("mode %u: an insert failed\n", mode); return 1; }
        for (size_t i = 0; i < px; i++) {
            if (i != 5 && i != 9 && !(out[4 * i] - out[4 * i] == 0.0f)) { std::printf("mode %u: pixel %zu is not finite\n", mode, i); return 1; }
            if (out[4 * i + 3] != 1.0f) { std::printf("mode %u: alpha\n", mode); return 1; }
            if (mode == 1 && shd[i] != -1.0f) { written++; if (!(shd[i] > 0.0f)) return 1; }
            if (mode >= 2 && !alias && dif[4 * i] != -1.0f) { written++; if (!(dif[4 * i] >= 0.0f && spe[4 * i] >= 0.0f)) return 1; }
        }
        uint32_t occupied = 0;
        for (uint64_t k : keys) occupied += k != 0u;
        std::printf("mode %u%s frame %u: rays %llu occupied %u\n", mode, alias ? " (aliased)" : "", frame, (unsigned long long)counters[0], occupied);
        if (!occupied) return 1;
    }
    if (mode && !alias && !written) { std::printf("mode %u wrote no output\n", mode); return 1; }
    return 0;
}

int main()
{
    for (uint32_t mode = 0; mode < 4; mode++)
        if (run(mode, false)) return 1;
    if (run(2, true)) return 2;
    std::printf("ok\n");
    return 0;
}
