// framegen_sanitize.cpp -- a stand-alone program for AddressSanitizer + UBSan over the frame-interpolation header (csrc/pt_framegen.h)
// as host C++: the scatter and the gather over 1x1, 3x2, 33x9 and 20x12 -> 40x24 images in both Formats, with huge and non-finite
// vectors and depths among the inputs.  Every buffer is a heap block of exactly its size (so the sanitizer sees the first byte out of
// bounds) inside which the data sits between two bands of guard bytes that must come back untouched.  Each case runs twice, the pixels
// in row order and in reverse: a min does not depend on the order, so field and output must agree bit for bit.  Built and run by
// tests/test_framegen.py with g++ -fsanitize=address,undefined; prints "framegen_sanitize ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_framegen.h"

using namespace pt;

namespace {

constexpr size_t kGuard = 64;  // bytes either side
constexpr unsigned char kFill = 0xA5;

struct Guarded {
    unsigned char* base;
    size_t bytes;
    explicit Guarded(size_t n) : base(static_cast<unsigned char*>(std::malloc(n + 2 * kGuard))), bytes(n)
    {
        if (!base) std::abort();
        std::memset(base, kFill, n + 2 * kGuard);
    }
    ~Guarded() { std::free(base); }
    template <class T> T* data() { return reinterpret_cast<T*>(base + kGuard); }
    bool intact() const
    {
        for (size_t i = 0; i < kGuard; i++)
            if (base[i] != kFill || base[kGuard + bytes + i] != kFill) return false;
        return true;
    }
};

uint32_t g_rng = 2463534242u;
uint32_t next_u32()
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 4;
}

float next_vector()
{
    const uint32_t r = next_u32();
    if (r % 53 == 0) return std::numeric_limits<float>::quiet_NaN();
    if (r % 47 == 0) return std::numeric_limits<float>::infinity();
    if (r % 43 == 0) return -std::numeric_limits<float>::infinity();
    if (r % 41 == 0) return 1e30f;
    if (r % 37 == 0) return -3.0e38f;
    if (r % 31 == 0) return 4.0e9f;  // beyond int32 once it is a pixel coordinate
    return ((float)(r % 2049u) - 1024.0f) / 64.0f;  // -16 .. 16 in steps of 1/64
}

float next_depth()
{
    const uint32_t r = next_u32();
    if (r % 29 == 0) return std::numeric_limits<float>::quiet_NaN();
    if (r % 23 == 0) return -2.0f;
    if (r % 19 == 0) return -0.0f;
    if (r % 5 == 0) return std::numeric_limits<float>::infinity();
    return (float)(1u << (r % 3u));
}

int run(uint32_t w, uint32_t h, uint32_t W, uint32_t H, uint32_t format)
{
    const size_t n = (size_t)w * h, N = (size_t)W * H;
    Guarded color(N * 4), prev_color(N * 4), hist_color(N * 4), depth(n * 4), prev_z(n * 4), hist_z(n * 4), mv(n * 12);
    Guarded out_a(N * 4), out_b(N * 4), field_a(n * 8), field_b(n * 8);
    for (size_t i = 0; i < N; i++) { color.data<uint32_t>()[i] = next_u32() * 16u + 7u; prev_color.data<uint32_t>()[i] = next_u32() * 16u + 3u; }
    for (size_t i = 0; i < n; i++) {
        depth.data<float>()[i] = next_depth();
        prev_z.data<float>()[i] = next_depth();
        for (int k = 0; k < 3; k++) mv.data<float>()[3 * i + k] = k == 2 ? 0.25f * (float)((int)(next_u32() % 3u) - 1) : next_vector();
    }
    const FgParams P = fg_params(w, h, W, H, format);
    FgBuffers b{};
    b.color = color.data<uint32_t>(); b.depth = depth.data<float>(); b.mv = mv.data<float>();
    b.prev_color = prev_color.data<uint32_t>(); b.prev_z = prev_z.data<float>();
    b.hist_color = hist_color.data<uint32_t>(); b.hist_z = hist_z.data<float>();
    for (int pass = 0; pass < 2; pass++) {
        b.out = (pass ? out_b : out_a).data<uint32_t>();
        b.field = (pass ? field_b : field_a).data<unsigned long long>();
        for (size_t i = 0; i < n; i++) b.field[i] = kFgHole;
        for (size_t j = 0; j < n; j++) {
            const size_t i = pass ? n - 1 - j : j;
            fg_scatter_pixel(P, b, (int)(i % w), (int)(i / w));
        }
        for (size_t j = 0; j < N; j++) {
            const size_t o = pass ? N - 1 - j : j;
            FgTrace t;
            b.out[o] = fg_gather_pixel(P, b, (int)(o % W), (int)(o / W), pass ? &t : nullptr);
        }
    }
    for (const Guarded* g : { &color, &prev_color, &hist_color, &depth, &prev_z, &hist_z, &mv, &out_a, &out_b, &field_a, &field_b })
        if (!g->intact()) { std::fprintf(stderr, "%ux%u -> %ux%u format %u: a guard band was written\n", w, h, W, H, format); return 1; }
    if (std::memcmp(field_a.data<char>(), field_b.data<char>(), n * 8) || std::memcmp(out_a.data<char>(), out_b.data<char>(), N * 4)) {
        std::fprintf(stderr, "%ux%u -> %ux%u format %u: the result depends on the order\n", w, h, W, H, format);
        return 1;
    }
    if (std::memcmp(hist_color.data<char>(), color.data<char>(), N * 4) || std::memcmp(hist_z.data<char>(), depth.data<char>(), n * 4)) {
        std::fprintf(stderr, "%ux%u -> %ux%u format %u: the history is not the current frame\n", w, h, W, H, format);
        return 1;
    }
    for (size_t i = 0; i < n; i++)
        if (field_a.data<unsigned long long>()[i] != kFgHole && (uint32_t)field_a.data<unsigned long long>()[i] >= n) {
            std::fprintf(stderr, "%ux%u format %u: field entry %zu names no pixel\n", w, h, format, i);
            return 1;
        }
    return 0;
}

}  // namespace

int main()
{
    const uint32_t sizes[4][4] = { {1, 1, 1, 1}, {3, 2, 3, 2}, {33, 9, 33, 9}, {20, 12, 40, 24} };
    int bad = 0;
    for (int rep = 0; rep < 8; rep++)
        for (const auto& s : sizes)
            for (uint32_t format = 0; format < 2; format++) bad += run(s[0], s[1], s[2], s[3], format);
    if (bad) return 1;
    std::printf("framegen_sanitize ok\n");
    return 0;
}
