// sharc_ff_sanitize.cpp -- TEST PROGRAM: csrc/pt_sharc.h's anti-firefly filter (row N19, DESIGN.md spec S25) stand-alone, so that
// tests/test_sharc_ff.py can build it with -fsanitize=address,undefined and run it as a child process: the clamp and the weight
// threshold on edge voxels (zeros, saturated sums, counts past 16 bits, NaN and infinite radiance through sh_quantise, NaN and infinite
// weights), then eight frames of update, resolve and query with the filter on over buffers exactly as large as the contract says.
// Exit status 0 = every invariant held.
#include "sharc_ff_host.h"
#include <cstdio>
#include <limits>

using namespace shhost;

static uint4 u4(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    uint4 v;
    v.x = x; v.y = y; v.z = z; v.w = w;
    return v;
}

static uint32_t w_word(uint32_t n, uint32_t frames, uint32_t stale) { return n | (frames << 16) | (stale << 24); }

static int edge_voxels()
{
    const uint32_t top = 0xFFFFFFFFu;
    const uint32_t sums[] = { 0u, 1u, 1023u, 1u << 24, (1u << 24) + 1u, 0x7FFFFFFFu, 0x80000000u, top - 128u, top - 1u, top };
    const uint32_t counts[] = { 0u, 1u, 7u, 8u, 65535u, 65536u, 1u << 20, top };
    const uint4 prevs[] = { u4(0, 0, 0, 0), u4(0, 0, 0, w_word(8, 2, 0)), u4(1, 1, 1, w_word(8, 2, 0)), u4(top, top, top, w_word(8, 2, 0)), u4(top, 0, 0, w_word(65535, 255, 254)),
                            u4(8192, 8192, 8192, w_word(8, 2, 3)), u4(8192, 8192, 8192, w_word(7, 200, 0)), u4(8192, 8192, 8192, w_word(60000, 1, 0)) };
    unsigned clamped = 0, cases = 0;
    for (uint32_t sx : sums)
        for (uint32_t sy : { 0u, sx, top })
            for (uint32_t n : counts)
                for (const uint4& prev : prevs) {
                    const uint4 acc = u4(sx, sy, sx / 3u, n);
                    uint4 a = acc;
                    const bool c = sh_ff_clamp(a, prev);
                    if (a.x > acc.x || a.y > acc.y || a.z > acc.z || a.w != acc.w) { std::printf("a sum rose or a count changed\n"); return 1; }
                    if (!c && (a.x != acc.x || a.y != acc.y || a.z != acc.z)) { std::printf("changed without clamping\n"); return 1; }
                    if (c && (n == 0u || sh_samples(prev) < kShFfMinSamples || sh_frames(prev) < kShFfMinFrames)) { std::printf("clamped without samples or history\n"); return 1; }
                    for (uint32_t A : { 1u, 10u, 255u }) {
                        bool clear_ff, clear;
                        const uint4 r = sh_resolve_slot_ff(acc, prev, A, 64u, clear_ff), want = sh_resolve_slot(a, prev, A, 64u, clear);
                        if (r.x != want.x || r.y != want.y || r.z != want.z || r.w != want.w || clear_ff != clear) { std::printf("the join differs\n"); return 1; }
                    }
                    clamped += c;
                    cases++;
                }
    std::printf("clamp: %u of %u edge voxels clamped\n", clamped, cases);
    if (!clamped || clamped == cases) return 1;
    for (float s : { 1.0f, 0.99999994f, 0.5f, 5.9604645e-8f, 1e-30f })
        for (uint32_t v : sums)
            if (sh_ff_scale(v, s) > v) { std::printf("sh_ff_scale rose\n"); return 1; }
    return 0;
}

static int edge_walks()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float values[] = { 0.0f, -0.0f, -1.0f, 1e-30f, 1.0f, 1.9f, 2.0f, 2.1f, 256.0f, 1e30f, kInf, -kInf, nan };
    std::vector<uint4> accum(4);
    unsigned stopped = 0, walks = 0;
    for (float w0 : values)
        for (float w1 : values)
            for (float r : values)
                for (uint32_t length = 0; length <= 3u; length++) {
                    std::memset(accum.data(), 0, accum.size() * sizeof(uint4));
                    ShMap m{};
                    m.accum = accum.data(); m.capacity = 4;
                    ShState st;
                    st.length = length; st.skipped = false; st.stopped = 0u;
                    for (uint32_t i = 0; i < 3u; i++) st.slot[i] = i + 1u;
                    st.weight[0] = make_f3(w0, w0, w1); st.weight[1] = make_f3(w1, w0, w1); st.weight[2] = make_f3(1.0f, w1, w0);
                    sh_propagate_ff(m, st, make_f3(r, 1.0f, nan));
                    if (st.stopped > 1u || (length == 0u && st.stopped)) { std::printf("a walk stopped twice, or with nothing stored\n"); return 1; }
                    if (accum[0].x || accum[0].w || accum[1].w || accum[2].w || accum[3].w) { std::printf("the walk wrote a slot or a count it must not\n"); return 1; }
                    for (uint32_t i = length + 1u; i < 4u; i++)
                        if (accum[i].x || accum[i].y || accum[i].z) { std::printf("the walk wrote past its length\n"); return 1; }
                    stopped += st.stopped;
                    walks++;
                }
    std::printf("weight threshold: %u of %u walks stopped\n", stopped, walks);
    return stopped && stopped < walks ? 0 : 1;
}

static PtCamera camera(float x, float y, float z)
{
    PtCamera c{};
    c.Position[0] = x; c.Position[1] = y; c.Position[2] = z;
    c.RightDirection[0] = 1.5f; c.UpDirection[1] = 1.0f; c.ForwardDirection[2] = 1.0f;
    c.NearDepth = 0.01f; c.FarDepth = kInf;
    return c;
}

// the scene of sharc_ex_sanitize.cpp with a stronger emitter, large voxels (SceneScale 5) so that histories form, a DI with a NaN, an
// inf and a negative texel, and a block of DI 1000 in the last frame
static int frames(uint32_t mode, bool with_di)
{
    const uint32_t n = 5, w = 24, h = 16, capacity = 1u << 10;
    PtSphere sp[n] = { { 0.0f, -1000.0f, 0.0f, 1000.0f }, { -1.5f, 1.0f, 0.0f, 1.0f }, { 1.5f, 0.8f, 0.5f, 0.8f }, { 0.0f, 3.0f, 1.0f, 0.2f }, { 0.0f, 0.6f, -1.5f, 0.6f } };
    PtMaterial mt[n] = {};
    for (uint32_t i = 0; i < n; i++) {
        mt[i].BaseColor[0] = 0.3f + 0.15f * (float)i; mt[i].BaseColor[1] = 0.6f; mt[i].BaseColor[2] = 0.8f - 0.15f * (float)i; mt[i].BaseColor[3] = 1.0f;
        mt[i].Roughness = 0.5f; mt[i].IOR = 1.5f;
    }
    mt[2].Metallic = 1.0f; mt[2].Roughness = 0.1f;
    mt[3].EmissiveStrength = 250.0f; mt[3].EmissiveColor[0] = 1.0f; mt[3].EmissiveColor[1] = 0.9f; mt[3].EmissiveColor[2] = 0.7f;
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
    uint64_t clamped = 0, stopped = 0;
    const uint32_t n_frames = 8;
    for (uint32_t frame = 0; frame < n_frames; frame++) {
        for (size_t i = 0; i < px; i++) {
            const bool spike = frame + 1u == n_frames && (i % w) >= 8u && (i % w) < 16u && (i / w) >= 4u && (i / w) < 12u;
            const float v = spike ? 1000.0f : 0.25f;
            for (int k = 0; k < 3; k++) { did[4 * i + k] = v; dis[4 * i + k] = 0.0f; }
            did[4 * i + 3] = dis[4 * i + 3] = 3.0f;
        }
        did[4 * 5] = std::numeric_limits<float>::quiet_NaN();
        did[4 * 9 + 1] = kInf;
        dis[4 * 11 + 2] = -2.0f;
        const PtCamera cam = camera(0.0f, 1.5f, -6.0f);
        const uint32_t prm[16] = { w, h, frame, 6, 1, 1, capacity, 1, 10, 8, 0, 7, 0, 0, w, h };
        const float fprm[3] = { 1e-3f, 5.0f, 0.4f };
        const Frame f(&cam, prm, fprm);
        Extras x;
        if (with_di) {
            x.di_diffuse = reinterpret_cast<const float4*>(did.data());
            x.di_specular = reinterpret_cast<const float4*>(dis.data());
        }
        x.mode = mode;
        x.spec_hit_dist = mode == 1 ? shd.data() : nullptr;
        x.diffuse = mode >= 2 ? reinterpret_cast<float4*>(dif.data()) : nullptr;
        x.specular = mode >= 2 ? reinterpret_cast<float4*>(spe.data()) : nullptr;
        uint64_t counters[2], ffc[2];
        run_call_ff(hs, &cam, f, keys.data(), accum, resolved, out.data(), counters, x, true, ffc);
        std::swap(accum, resolved);
        clamped += ffc[0]; stopped += ffc[1];
        for (size_t i = 0; i < px; i++)
            if (out[4 * i + 3] != 1.0f) { std::printf("mode %u: alpha\n", mode); return 1; }
        uint32_t occupied = 0;
        for (uint64_t k : keys) occupied += k != 0u;
        std::printf("mode %u%s frame %u: rays %llu failed %llu occupied %u clamped %llu stopped %llu\n", mode, with_di ? " with DI" : "", frame,
                    (unsigned long long)counters[0], (unsigned long long)counters[1], occupied, (unsigned long long)ffc[0], (unsigned long long)ffc[1]);
        if (!occupied) return 1;
    }
    if (with_di && !clamped) { std::printf("the DI spike clamped nothing\n"); return 1; }
    return 0;
}

int main()
{
    if (edge_voxels()) return 1;
    if (edge_walks()) return 2;
    if (frames(0, false)) return 3;
    if (frames(1, true)) return 4;
    if (frames(2, true)) return 5;
    std::printf("ok\n");
    return 0;
}
