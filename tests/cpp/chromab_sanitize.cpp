// chromab_sanitize.cpp -- a stand-alone program for AddressSanitizer + UBSan over the chromatic-aberration header (csrc/pt_chromab.h) as
// host C++: the per-pixel functions over 1x1, 1x40, 40x1, 31x7, 33x9 and 67x19 images with zero, default, extreme and mixed offsets and
// four foci, and over 16384x8 and 8x16384 with the focus in a corner and k = +-1/16 (the largest coordinates and displacements the API
// admits), once on whole-image planes and once the way pt_chromab.hip runs them (per 32 x 8 block three 35 x 10 windows staged from
// cab_origin; tests/hostshim/chromab_host.h).  Every buffer, the window included, is a heap block of exactly its size (so the
// sanitizer sees the first byte out of bounds) inside which the data sits between two bands of guard bytes that must come back
// untouched.  The two paths must agree bit for bit and no tap may fall outside its window.  Built and run by
// tests/test_chromatic_aberration.py with g++ -fsanitize=address,undefined; prints "chromab_sanitize ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../hostshim/chromab_host.h"

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

uint32_t g_rng = 12345u;
float next_float()
{
    g_rng = g_rng * 1664525u + 1013904223u;
    const uint32_t r = g_rng >> 8;
    if (r % 97 == 0) return std::numeric_limits<float>::quiet_NaN();
    if (r % 89 == 0) return std::numeric_limits<float>::infinity();
    if (r % 83 == 0) return -std::numeric_limits<float>::infinity();
    if (r % 79 == 0) return -1.5f;
    return 0.01f * (float)(1u + r % 10000u);  // 0.01 .. 100
}

int run(int w, int h, const float* focus_uv, const float* offsets)
{
    const size_t n = (size_t)w * h;
    Guarded color(n * sizeof(float4)), whole(n * sizeof(float4)), tiled(n * sizeof(float4)), planes(3 * n * sizeof(float));
    Guarded window(3 * kCabPlane * sizeof(float));
    float4* c = color.data<float4>();
    for (size_t i = 0; i < n; i++) c[i] = up_f4(next_float(), next_float(), next_float(), next_float());
    const CabConfig k = cab_config((uint32_t)w, (uint32_t)h, focus_uv, offsets);
    chromab_frame(w, h, k, c, whole.data<float4>(), planes.data<float>());
    const uint64_t outside = chromab_frame_tiled(w, h, k, c, tiled.data<float4>(), window.data<float>());
    const char* what = nullptr;
    if (!color.intact() || !whole.intact() || !tiled.intact() || !planes.intact() || !window.intact()) what = "a guard band was written";
    else if (outside) what = "a tap fell outside its window";
    else if (std::memcmp(whole.data<float4>(), tiled.data<float4>(), n * sizeof(float4)) != 0) what = "the tiled path differs from the whole-image path";
    for (size_t i = 0; i < n && !what; i++) {
        const float4 o = whole.data<float4>()[i];
        // a convex combination of values in [0, 65504], up to a few roundings
        if (!(o.x >= 0.0f && o.x <= 65520.0f) || !(o.y >= 0.0f && o.y <= 65520.0f) || !(o.z >= 0.0f && o.z <= 65520.0f)) what = "a texel is not a finite non-negative colour";
        if (std::memcmp(&o.w, &c[i].w, 4) != 0) what = "alpha did not pass through";
    }
    if (what) std::fprintf(stderr, "%dx%d focus %g %g offsets %g %g %g: %s\n", w, h, focus_uv[0], focus_uv[1], offsets[0], offsets[1], offsets[2], what);
    return what ? 1 : 0;
}

}  // namespace

int main()
{
    constexpr float m = kCabMaxOffset;
    const int sizes[6][2] = { {1, 1}, {1, 40}, {40, 1}, {31, 7}, {33, 9}, {67, 19} };
    const float foci[4][2] = { {0.5f, 0.5f}, {0.0f, 0.0f}, {1.0f, 1.0f}, {0.3f, 0.8f} };
    const float offsets[7][3] = { {0.0f, 0.0f, 0.0f}, {0.003f, 0.003f, -0.003f}, {-0.003f, -0.003f, 0.003f}, {m, m, m}, {-m, -m, -m}, {m, -0.003f, -m}, {-m, 0.02f, m} };
    int bad = 0;
    for (const auto& s : sizes)
        for (const auto& f : foci)
            for (const auto& k : offsets) bad += run(s[0], s[1], f, k);
    const int extremes[2][2] = { {16384, 8}, {8, 16384} };
    for (const auto& s : extremes)
        for (const int corner : { 1, 2 })
            for (const int k : { 3, 4, 5 }) bad += run(s[0], s[1], foci[corner], offsets[k]);
    if (bad) return 1;
    std::printf("chromab_sanitize ok\n");
    return 0;
}
