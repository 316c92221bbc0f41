// gbframe_sanitize.cpp -- TEST PROGRAM: csrc/pt_pixfmt.h's packers and csrc/pt_gbframe.h's frame over a small scene, stand-alone, so that
// tests/test_gbframe.py can build it with -fsanitize=address,undefined and run it as a child process: every half pattern through both
// conversions, the conversions' edge inputs, then the G-buffer pass into exactly sized float32 and packed buffers and the frame from both,
// with and without DI, over a 1x1 frame, a ragged frame and a sub-rect of it.  Prints what it saw; exit status 0 = every invariant held
// (the sanitizers abort on their own findings).
#include "gbframe_host.h"
#include <cstdio>

using namespace gbfhost;

static int formats()
{
    for (uint32_t h = 0; h < 65536u; h++) {
        const float f = half_decode(h);
        const uint32_t back = half_encode(f);
        const bool nan = (h & 0x7C00u) == 0x7C00u && (h & 0x3FFu);
        if (nan ? back != ((h & 0x8000u) | 0x7E00u) : back != h) { std::printf("half %04x -> %g -> %04x\n", h, f, back); return 1; }
    }
    const float edge[] = { 0.0f, -0.0f, 1e-30f, -1e-30f, 5.9604645e-08f, 2.9802322e-08f, 2.9802326e-08f, 6.1035156e-05f, 0.5f, 1.0f, -1.0f, 2.0f, -2.0f, 65504.0f, 65519.996f,
                           65520.0f, 1e30f, -1e30f, kInf, -kInf, kInf - kInf, 3.4028235e38f, 1.1754944e-38f, 1e-45f };
    uint32_t sum = 0;
    for (float x : edge) {
        sum += half_encode(x) + unorm8_encode(x) + snorm16_encode(x);
        const float u = unorm8_decode(unorm8_encode(x)), s = snorm16_decode(snorm16_encode(x));
        if (!(u >= 0.0f && u <= 1.0f) || !(s >= -1.0f && s <= 1.0f)) { std::printf("decode out of range for %g\n", x); return 1; }
    }
    for (uint32_t q = 0; q < 65536u; q++)
        if (!(snorm16_decode(q) >= -1.0f && snorm16_decode(q) <= 1.0f)) { std::printf("snorm16 %u\n", q); return 1; }
    std::printf("formats: checksum %u\n", sum);
    return 0;
}

static int run(const shhost::HostScene& hs, uint32_t w, uint32_t h, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, uint32_t spp, uint32_t bounces)
{
    PtCamera cam{};
    cam.Position[1] = 1.5f; cam.Position[2] = -6.0f;
    cam.RightDirection[0] = 1.5f; cam.UpDirection[1] = 1.0f; cam.ForwardDirection[2] = 1.0f;
    cam.NearDepth = 0.01f; cam.FarDepth = kInf;
    for (int m = 0; m < 8; m++)
        for (int k = 0; k < 4; k++) cam.Matrices[m][5 * k] = 1.0f;  // identities: the projected channels are not what this program is about
    const uint32_t rect[4] = { rx, ry, rw, rh };
    const size_t n = (size_t)rw * rh;
    // exactly sized buffers: one byte past a channel is the sanitizer's
    std::vector<float> f32(n * kFloatsPerPixel, -7.0f);
    std::vector<uint32_t> mask(n);
    std::vector<std::vector<uint8_t>> packed(13);
    void* pp[13];
    for (int k = 0; k < 13; k++) { packed[k].assign(n * kGbPackedTexelBytes[k], 0xAB); pp[k] = packed[k].data(); }
    run_gbuffer(hs, HostEnvMap{}, false, &cam, w, h, rect, nullptr, nullptr, false, kGbAll, f32.data(), mask.data(), nullptr, nullptr, pp);
    // the float32 channels the frame reads, as PtGBuffer lays them out
    std::vector<float> pos(n * 4), fn(n * 2), gn(n * 2), bcm(n * 4), nr(n * 4), ior(n), tr(n), rad(n * 3);
    for (size_t i = 0; i < n; i++) {
        const float* v = f32.data() + i * kFloatsPerPixel;
        std::memcpy(&pos[4 * i], v, 16); std::memcpy(&fn[2 * i], v + 4, 8); std::memcpy(&gn[2 * i], v + 6, 8); std::memcpy(&bcm[4 * i], v + 13, 16);
        std::memcpy(&nr[4 * i], v + 23, 16); ior[i] = v[27]; tr[i] = v[28]; std::memcpy(&rad[3 * i], v + 29, 12);
    }
    std::vector<float> di_d(n * 4, 0.25f), di_s(n * 4, 0.0f);
    const uint32_t prm[10] = { w, h, 2, bounces, spp, 1, rx, ry, rw, rh };
    const GbFrame fr = frame_of(&cam, prm, 1e-3f);
    for (uint32_t format = 0; format < 2; format++)
        for (int with_di = 0; with_di < 2; with_di++) {
            GbInput in{};
            in.format = format;
            in.Position = reinterpret_cast<const float4*>(format ? pp[0] : (void*)pos.data());
            in.FlatNormal = format ? pp[1] : (void*)fn.data(); in.GeometricNormal = format ? pp[2] : (void*)gn.data();
            in.BaseColorMetalness = format ? pp[6] : (void*)bcm.data(); in.NormalRoughness = format ? pp[9] : (void*)nr.data();
            in.IOR = format ? pp[10] : (void*)ior.data(); in.Transmission = format ? pp[11] : (void*)tr.data(); in.Radiance = format ? pp[12] : (void*)rad.data();
            if (with_di) { in.di_diffuse = reinterpret_cast<const float4*>(di_d.data()); in.di_specular = reinterpret_cast<const float4*>(di_s.data()); }
            std::vector<float> out(n * 4);
            std::vector<uint32_t> per_pixel(n);
            const uint64_t rays = run_frame(hs, HostEnvMap{}, fr, in, rect, out.data(), per_pixel.data());
            uint64_t sum = 0;
            for (uint32_t r : per_pixel) sum += r;
            if (sum != rays) { std::printf("ray counts disagree\n"); return 1; }
            for (size_t i = 0; i < n; i++) {
                const bool miss = !(mask[i] & kGbFlatNormal);
                if (miss && per_pixel[i] != 0u) { std::printf("a miss traced rays\n"); return 1; }
                if (bounces == 0u && per_pixel[i] != 0u) { std::printf("Bounces 0 traced rays\n"); return 1; }
            }
            for (float v : out) if (!(v == v) || v - v != 0.0f) { std::printf("pixel not finite\n"); return 1; }
            std::printf("%ux%u rect %u,%u %ux%u spp %u bounces %u format %u di %d: rays %llu\n", w, h, rx, ry, rw, rh, spp, bounces, format, with_di, (unsigned long long)rays);
        }
    return 0;
}

int main()
{
    if (formats()) return 1;
    const uint32_t n = 5;
    PtSphere sp[n] = { { 0.0f, -1000.0f, 0.0f, 1000.0f }, { -1.5f, 1.0f, 0.0f, 1.0f }, { 1.5f, 0.8f, 0.5f, 0.8f }, { 0.0f, 3.0f, 1.0f, 0.5f }, { 0.0f, 0.6f, -1.5f, 0.6f } };
    PtMaterial mt[n] = {};
    for (uint32_t i = 0; i < n; i++) {
        mt[i].BaseColor[0] = 0.3f + 0.15f * (float)i; mt[i].BaseColor[1] = 0.6f; mt[i].BaseColor[2] = 0.8f - 0.15f * (float)i; mt[i].BaseColor[3] = 1.0f;
        mt[i].Roughness = 0.5f; mt[i].IOR = 1.5f;
    }
    mt[2].Metallic = 1.0f;  // its Transmission texel is never written, and never read
    mt[3].EmissiveStrength = 10.0f; mt[3].EmissiveColor[0] = 1.0f; mt[3].EmissiveColor[1] = 0.9f; mt[3].EmissiveColor[2] = 0.7f;
    mt[4].Transmission = 1.0f; mt[4].Roughness = 0.05f;
    const float env[4] = { 0.2f, 0.25f, 0.3f, 1.0f };
    shhost::HostScene hs;
    hs.set(sp, mt, n, env, nullptr, nullptr, 0, nullptr, nullptr);
    if (run(hs, 1, 1, 0, 0, 1, 1, 3, 6)) return 1;
    if (run(hs, 19, 13, 0, 0, 19, 13, 2, 6)) return 1;
    if (run(hs, 19, 13, 5, 3, 11, 9, 1, 0)) return 1;
    if (run(hs, 19, 13, 5, 3, 11, 9, 3, 8)) return 1;
    std::printf("ok\n");
    return 0;
}
