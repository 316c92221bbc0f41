// lens_sanitize.cpp -- TEST PROGRAM: csrc/pt_lens.h's frame over a small scene, stand-alone, so that tests/test_lens.py can build it with
// -fsanitize=address,undefined and run it as a child process: apertures 0 and > 0, a 1x1 frame, a ragged frame and a sub-rect of it.
// Prints what it saw; exit status 0 = every invariant held (the sanitizers abort on their own findings).
#include "lens_host.h"
#include <cstdio>

using namespace lenshost;

static int run(const shhost::HostScene& hs, float aperture, uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, uint32_t spp)
{
    PtCamera cam{};
    cam.Position[1] = 1.5f; cam.Position[2] = -6.0f;
    cam.RightDirection[0] = 1.5f * 6.0f; cam.UpDirection[1] = 6.0f; cam.ForwardDirection[2] = 6.0f;  // in focus at view depth 6
    cam.ApertureRadius = aperture;
    cam.NearDepth = 0.01f; cam.FarDepth = kInf;
    const uint32_t prm[10] = { w, h, 2, 6, spp, 1, rx, ry, rw, rh };
    std::vector<float> out((size_t)rw * rh * 4u);
    std::vector<uint32_t> per_pixel((size_t)rw * rh);
    const uint64_t rays = run_frame(hs, HostEnvMap{}, frame_of(&cam, prm, 1e-3f), prm + 6, out.data(), per_pixel.data());
    uint64_t sum = 0;
    for (uint32_t r : per_pixel) sum += r;
    if (sum != rays || rays < (uint64_t)rw * rh) { std::printf("ray counts disagree\n"); return 1; }
    for (float v : out) if (!(v == v) || v - v != 0.0f) { std::printf("pixel not finite\n"); return 1; }
    std::printf("aperture %g %ux%u rect %u,%u %ux%u spp %u: rays %llu\n", aperture, w, h, rx, ry, rw, rh, spp, (unsigned long long)rays);
    return 0;
}

int main()
{
    const uint32_t n = 5;
    PtSphere sp[n] = { { 0.0f, -1000.0f, 0.0f, 1000.0f }, { -1.5f, 1.0f, 0.0f, 1.0f }, { 1.5f, 0.8f, 0.5f, 0.8f }, { 0.0f, 3.0f, 1.0f, 0.5f }, { 0.0f, 0.6f, -1.5f, 0.6f } };
    PtMaterial mt[n] = {};
    for (uint32_t i = 0; i < n; i++) {
        mt[i].BaseColor[0] = 0.3f + 0.15f * (float)i; mt[i].BaseColor[1] = 0.6f; mt[i].BaseColor[2] = 0.8f - 0.15f * (float)i; mt[i].BaseColor[3] = 1.0f;
        mt[i].Roughness = 0.5f; mt[i].IOR = 1.5f;
    }
    mt[3].EmissiveStrength = 10.0f; mt[3].EmissiveColor[0] = 1.0f; mt[3].EmissiveColor[1] = 0.9f; mt[3].EmissiveColor[2] = 0.7f;
    mt[4].Transmission = 1.0f; mt[4].Roughness = 0.05f;
    const float env[4] = { 0.2f, 0.25f, 0.3f, 1.0f };
    shhost::HostScene hs;
    hs.set(sp, mt, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    for (float aperture : { 0.0f, 0.05f, 1.0f }) {
        if (run(hs, aperture, 1, 1, 0, 0, 1, 1, 3)) return 1;
        if (run(hs, aperture, 19, 13, 0, 0, 19, 13, 2)) return 1;
        if (run(hs, aperture, 19, 13, 5, 3, 11, 9, 1)) return 1;
    }
    std::printf("ok\n");
    return 0;
}
