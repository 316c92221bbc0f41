// sharc_sanitize.cpp -- TEST PROGRAM: csrc/pt_sharc.h's update, resolve and query over a small scene for three frames, stand-alone, so that
// tests/test_sharc.py can build it with -fsanitize=address,undefined and run it as a child process.  Two runs: a roomy cache whose voxels
// are evicted after the camera jumps away (MaxStaleFrames 1), and a cache of one bucket, which overflows.  Prints what it saw; exit
// status 0 = every invariant held (the sanitizers abort on their own findings).
#include "sharc_host.h"
#include <cstdio>
#include <set>

using namespace shhost;

static PtCamera camera(float x, float y, float z)
{
    PtCamera c{};
    c.Position[0] = x; c.Position[1] = y; c.Position[2] = z;
    c.RightDirection[0] = 1.5f; c.UpDirection[1] = 1.0f; c.ForwardDirection[2] = 1.0f;
    c.NearDepth = 0.01f; c.FarDepth = kInf;
    return c;
}

static int run(uint32_t capacity, uint32_t max_stale, bool jump, uint64_t& failed_total, uint32_t& evicted)
{
    const uint32_t n = 5, w = 24, h = 16;
    PtSphere sp[n] = { { 0.0f, -1000.0f, 0.0f, 1000.0f }, { -1.5f, 1.0f, 0.0f, 1.0f }, { 1.5f, 0.8f, 0.5f, 0.8f }, { 0.0f, 3.0f, 1.0f, 0.5f }, { 0.0f, 0.6f, -1.5f, 0.6f } };
    PtMaterial mt[n] = {};
    for (uint32_t i = 0; i < n; i++) {
        mt[i].BaseColor[0] = 0.3f + 0.15f * (float)i; mt[i].BaseColor[1] = 0.6f; mt[i].BaseColor[2] = 0.8f - 0.15f * (float)i; mt[i].BaseColor[3] = 1.0f;
        mt[i].Roughness = 0.5f; mt[i].IOR = 1.5f;
    }
    mt[3].EmissiveStrength = 10.0f; mt[3].EmissiveColor[0] = 1.0f; mt[3].EmissiveColor[1] = 0.9f; mt[3].EmissiveColor[2] = 0.7f;
    mt[4].Transmission = 1.0f; mt[4].Roughness = 0.05f;
    const float env[4] = { 0.2f, 0.25f, 0.3f, 1.0f };
    HostScene hs;
    hs.set(sp, mt, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    std::vector<uint64_t> keys(capacity, 0);
    std::vector<uint4> a(capacity), b(capacity);
    std::memset(a.data(), 0, capacity * sizeof(uint4));
    std::memset(b.data(), 0, capacity * sizeof(uint4));
    std::vector<float> out((size_t)w * h * 4u);
    uint4 *accum = a.data(), *resolved = b.data();
    std::set<uint64_t> first;
    evicted = 0;
    for (uint32_t frame = 0; frame < 3; frame++) {
        const PtCamera cam = (jump && frame > 0) ? camera(0.0f, 300.0f, -900.0f) : camera(0.0f, 1.5f, -6.0f);
        const uint32_t prm[16] = { w, h, frame, 6, 1, 1, capacity, 2, 4, max_stale, 0, 7, 0, 0, w, h };
        const float fprm[3] = { 1e-3f, 50.0f, 0.4f };
        const Frame f(&cam, prm, fprm);
        uint64_t counters[2];
        run_call(hs, &cam, f, keys.data(), accum, resolved, out.data(), counters);
        std::swap(accum, resolved);
        failed_total += counters[1];
        std::set<uint64_t> now;
        uint32_t occupied = 0;
        for (uint64_t k : keys) if (k) { occupied++; if (!now.insert(k).second) { std::printf("duplicate key\n"); return 1; } }
        if (occupied > capacity) return 1;
        if (frame == 0) first = now;
        else for (uint64_t k : first) if (!now.count(k)) evicted++;
        for (float v : out) if (!(v == v) || v - v != 0.0f) { std::printf("pixel not finite\n"); return 1; }
        std::printf("capacity %u frame %u: rays %llu failed %llu occupied %u\n", capacity, frame, (unsigned long long)counters[0], (unsigned long long)counters[1], occupied);
    }
    return 0;
}

int main()
{
    uint64_t failed = 0;
    uint32_t evicted = 0;
    if (run(1u << 12, 1, true, failed, evicted)) return 1;
    if (failed != 0 || evicted == 0) { std::printf("roomy cache: failed %llu evicted %u\n", (unsigned long long)failed, evicted); return 2; }
    failed = 0;
    if (run(16, 1, false, failed, evicted)) return 1;
    if (failed == 0) { std::printf("one bucket did not overflow\n"); return 3; }
    std::printf("ok\n");
    return 0;
}
