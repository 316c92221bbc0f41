// reblur_sanitize.cpp -- a stand-alone program for AddressSanitizer + UBSan over the ReBLUR stand-in's header (csrc/pt_reblur.h) as
// host C++: three calls (a restart, then two with history and motion vectors that point far outside the image) of all four passes over
// 1 x 1, 1 x 40 and 37 x 11 images with misses, zero hit distances and a hit distance of 1 everywhere else, MinBlurRadius =
// MaxBlurRadius = 64 and a roughness of 1, so that every pixel's taps are 64 pixels long and leave the image on every border.  Every
// buffer is a heap block of exactly its size (so the sanitizer sees the first byte out of bounds) inside which the data sits between
// two bands of guard bytes that must come back untouched.  Built and run by tests/test_nrd_reblur.py with g++
// -fsanitize=address,undefined; prints "reblur_sanitize ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../hostshim/reblur_host.h"

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
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
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
    return g_rng >> 8;
}
float next_float() { return 0.01f * (float)(1u + next_u32() % 1000u); }  // 0.01 .. 10

int run(int w, int h)
{
    const size_t n = (size_t)w * h;
    Guarded viewz(n * 4), mv(n * 12), nr(n * 16), in_d(n * 16), in_s(n * 16), out_d(n * 16), out_s(n * 16), x_d(n * 16), x_s(n * 16);
    Guarded* slot[2][5];
    for (auto& s : slot)
        for (auto& p : s) {
            p = new Guarded(n * 16);
            std::memset(p->data<float>(), 0, n * 16);
        }
    int bad = 0;
    for (uint32_t call = 0; call < 3; call++) {
        for (size_t i = 0; i < n; i++) {
            const uint32_t r = next_u32();
            viewz.data<float>()[i] = r % 7 == 0 ? std::numeric_limits<float>::infinity() : (r % 11 == 0 ? std::numeric_limits<float>::quiet_NaN() : 5.0f + 0.01f * (float)(i % 13));
            float* m = mv.data<float>() + 3 * i;
            m[0] = r % 5 == 0 ? 1e9f : (r % 13 == 0 ? -1e9f : (r % 17 == 0 ? std::numeric_limits<float>::quiet_NaN() : 0.3f * (float)((int)(r % 9) - 4)));
            m[1] = r % 3 == 0 ? -70.0f : 0.4f * (float)((int)(r % 7) - 3);
            m[2] = 0.0f;
            nr.data<float4>()[i] = pt::dn_f4(0.0f, 0.0f, -1.0f, 1.0f);
            in_d.data<float4>()[i] = pt::dn_f4(next_float(), next_float() - 5.0f, next_float() - 5.0f, r % 4 == 0 ? 0.0f : 1.0f);
            in_s.data<float4>()[i] = pt::dn_f4(next_float(), next_float() - 5.0f, next_float() - 5.0f, r % 6 == 0 ? 0.0f : 1.0f);
        }
        const uint32_t cur = (call + 1) & 1u, prev = call & 1u;
        void* ptrs[kRbHostPtrs] = { viewz.data<float>(), mv.data<float>(), nr.data<float4>(), in_d.data<float4>(), in_s.data<float4>(),
                                    out_d.data<float4>(), out_s.data<float4>(),
                                    slot[prev][0]->data<float4>(), slot[prev][1]->data<float4>(), slot[prev][2]->data<float4>(),
                                    slot[prev][3]->data<float4>(), slot[prev][4]->data<float4>(),
                                    slot[cur][0]->data<float4>(), slot[cur][1]->data<float4>(), slot[cur][2]->data<float4>(),
                                    slot[cur][3]->data<float4>(), slot[cur][4]->data<float4>(), x_d.data<float4>(), x_s.data<float4>() };
        const uint32_t prm[7] = { (uint32_t)w, (uint32_t)h, 30u, 6u, 3u, call == 0 ? 1u : 0u, 0xFFFFFFF0u + call };
        const float radii[2] = { pt::kRbMaxRadius, pt::kRbMaxRadius };
        const pt::RbBuffers b = rb_host_buffers((uint32_t)w, (uint32_t)h, ptrs);
        const pt::RbParams P = rb_host_params(prm, radii);
        if (pt::rb_radius(P, 1.0f, 0.0f) != pt::kRbMaxRadius || pt::rb_radius(P, 30.0f, 1.0f) != pt::kRbMaxRadius) bad++;
        for (uint32_t pass = 0; pass < 4; pass++) rb_host_run(pass, b, P);
        for (size_t i = 0; i < n; i++) {
            if (!pt::is_finite(viewz.data<float>()[i])) continue;
            const float4 o = out_d.data<float4>()[i], s = out_s.data<float4>()[i];
            if (!pt::is_finite(o.x) || !pt::is_finite(s.x) || !(o.x > 0.0f && o.x <= 10.001f) || !(s.x > 0.0f && s.x <= 10.001f)) bad++;
        }
    }
    for (Guarded* g : { &viewz, &mv, &nr, &in_d, &in_s, &out_d, &out_s, &x_d, &x_s })
        if (!g->intact()) bad++;
    for (auto& s : slot)
        for (auto& p : s) {
            if (!p->intact()) bad++;
            delete p;
        }
    if (bad) std::fprintf(stderr, "reblur_sanitize: %d x %d: %d failures\n", w, h, bad);
    return bad;
}

}  // namespace

int main()
{
    int bad = 0;
    bad += run(1, 1);
    bad += run(1, 40);
    bad += run(37, 11);
    if (bad) return 1;
    std::printf("reblur_sanitize ok\n");
    return 0;
}
