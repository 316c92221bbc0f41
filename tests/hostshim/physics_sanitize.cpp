// physics_sanitize.cpp -- TEST PROGRAM: the paths of csrc/pt_physics.h (row N23, DESIGN.md spec S27) through tests/hostshim/physics_host.h
// behind a main of its own, for a build with -fsanitize=address,undefined (__graft_entry__.build_physics_sanitizer).  Every array is a
// std::vector of exactly n records, so an index past a body is an ASan report; the clamp, the freeze, coincident centres, an empty and a
// one-body state and non-finite contributions run through the integer conversions UBSan watches.  Prints "physics_sanitize ok".
#include <cstdio>
#include <limits>
#include <vector>

#include "physics_host.h"

using namespace phhost;

namespace {

uint32_t g_seed = 12345u;
float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) * (1.0f / 16777216.0f); }

int run(uint32_t n, bool attract, bool wild, uint32_t steps, uint32_t& contacts, uint32_t& frozen, uint32_t& clamped)
{
    std::vector<PtSphere> sph(n);
    std::vector<PtPhysicsBody> body(n);
    std::vector<float> lin((size_t)n * 3), ang((size_t)n * 3);
    const float side = 0.25f * std::cbrt((float)(n ? n : 1));
    for (uint32_t i = 0; i < n; i++) {
        sph[i] = { rnd() * side, rnd() * side, rnd() * side, 0.05f + 0.1f * rnd() };
        if (i % 11 == 3 && i > 0) { sph[i].cx = sph[i - 1].cx; sph[i].cy = sph[i - 1].cy; sph[i].cz = sph[i - 1].cz; }  // coincident centres
        body[i] = { i % 8 == 0 ? 0.0f : 1.0f / (4.19f * sph[i].r * sph[i].r * sph[i].r), (i % 5 == 0 ? (uint32_t)PT_PHYSICS_SPRING : 0u) | (i % 9 == 1 ? (uint32_t)PT_PHYSICS_LARGE : 0u)
                    | (i % 17 == 5 ? (uint32_t)PT_PHYSICS_DISABLED : 0u), sph[i].cy, 4.4f };
        for (int k = 0; k < 3; k++) { lin[3 * i + k] = 2.0f * rnd() - 1.0f; ang[3 * i + k] = 6.0f * rnd() - 3.0f; }
        if (wild && i % 13 == 2) { if (i % 2) ang[3 * i] = 3.0e38f; else lin[3 * i] = 1.0e7f; }  // overflows the quaternion's length / exceeds the clamp
    }
    State st;
    st.set(sph.data(), body.data(), lin.data(), ang.data(), nullptr, n);
    PtPhysicsSettings s{ 4, 0, 0.6f, 0.5f, 0.2f, 0.005f, 2.0f, 0 };
    PtPhysicsAttractor att[2] = { { 0, PT_PHYSICS_INVERSE_SQUARE, 3.0f, PT_PHYSICS_ALL_BODIES }, { n > 1 ? 1u : 0u, PT_PHYSICS_CONSTANT, 10.0f, n > 2 ? 2u : 0u } };
    const PhParams p = make_params(s, att, attract && n ? 2u : 0u, 1.0f / 60.0f);
    uint32_t report[3] = { 0, 0, 0 };
    for (uint32_t k = 0; k < steps; k++) step(st, s, p, report);
    contacts = report[0]; clamped = report[1]; frozen = report[2];
    for (uint32_t i = 0; i < n; i++)
        for (float v : { st.sph[i].x, st.sph[i].y, st.sph[i].z, st.rot[i].x, st.rot[i].y, st.rot[i].z, st.rot[i].w })
            if (!std::isfinite(v)) { std::printf("body %u of %u left the step not finite\n", i, n); return 1; }
    if (st.rule_violations) { std::printf("%u pairs without exactly one handler\n", st.rule_violations); return 1; }
    return 0;
}

}  // namespace

int main()
{
    uint32_t contacts = 0, frozen = 0, clamped = 0;
    for (uint32_t n : { 0u, 1u, 2u, 3u, 64u, 65u, 300u, 1025u }) {
        if (run(n, false, false, 6, contacts, frozen, clamped)) return 1;
        if (run(n, true, false, 6, contacts, frozen, clamped)) return 1;
        if (n >= 64u && contacts == 0u) { std::printf("no contacts among %u bodies\n", n); return 1; }
    }
    if (run(300, true, true, 6, contacts, frozen, clamped)) return 1;
    if (!frozen || !clamped) { std::printf("the wild state froze %u bodies and clamped %u\n", frozen, clamped); return 1; }
    // the leaf conversions at their edges
    bool c = false;
    const float inf = std::numeric_limits<float>::infinity();
    long long sum = 0;
    for (float x : { 0.0f, -0.0f, 1e-30f, 32768.0f, -32768.0f, 32768.01f, 1e30f, -1e30f, inf, -inf, std::numeric_limits<float>::quiet_NaN() }) sum += ph_quantize(x, c);
    if (!c || sum != (1ll << 39)) { std::printf("ph_quantize: sum %lld clamped %d\n", sum, (int)c); return 1; }
    if (ph_apply(1.0f, 1ll << 62) != 1.0f + 274877906944.0f) { std::printf("ph_apply\n"); return 1; }
    std::printf("physics_sanitize ok\n");
    return 0;
}
