// physics_host.h -- TEST SHIM: a whole step of row N23 (DESIGN.md spec S27) over csrc/pt_physics.h compiled as plain host C++: the state of
// pt_physics_*, the same sequence of passes as pt_physics_step queues, pairs found by a sort-and-sweep along x instead of the tree.  Shared by
// physics_host.cpp (the library the tests and tools load) and physics_sanitize.cpp.  Not part of the product; never loaded by it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_physics.h"

namespace phhost {

using namespace pt;

struct State {
    std::vector<PhVec4> sph, rot, vel, ang, v0, vel_start, ang_start;
    std::vector<PtPhysicsBody> body;
    std::vector<uint32_t> count;
    std::vector<long long> acc;
    std::vector<uint8_t> walks;  // S27.4: 0 for the first PT_PHYSICS_MAX_LARGE bodies flagged LARGE
    uint32_t n = 0;
    uint32_t rule_violations = 0;  // pairs that S27.4 gave to no body or to more than one (must stay 0)
    uint64_t steps = 0;

    void set(const PtSphere* spheres, const PtPhysicsBody* bodies, const float* lin_vel, const float* ang_vel, const float* rotations, uint32_t n_)
    {
        n = n_;
        sph.resize(n); rot.resize(n); vel.resize(n); ang.resize(n); v0.assign(n, PhVec4{}); vel_start.assign(n, PhVec4{}); ang_start.assign(n, PhVec4{});
        body.assign(bodies, bodies + n);
        count.assign(n, 0u);
        acc.assign((size_t)n * kPhAccPerBody, 0);
        walks.assign(n, 1);
        uint32_t n_large = 0;
        for (uint32_t i = 0; i < n; i++) {
            sph[i] = { spheres[i].cx, spheres[i].cy, spheres[i].cz, spheres[i].r };
            vel[i] = lin_vel ? PhVec4{ lin_vel[3 * i], lin_vel[3 * i + 1], lin_vel[3 * i + 2], 0.0f } : PhVec4{ 0, 0, 0, 0 };
            ang[i] = ang_vel ? PhVec4{ ang_vel[3 * i], ang_vel[3 * i + 1], ang_vel[3 * i + 2], 0.0f } : PhVec4{ 0, 0, 0, 0 };
            rot[i] = rotations ? PhVec4{ rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3] } : PhVec4{ 0, 0, 0, 1 };
            if ((body[i].Flags & PT_PHYSICS_LARGE) && n_large < PT_PHYSICS_MAX_LARGE) { walks[i] = 0; n_large++; }
        }
    }
};

inline PhParams make_params(const PtPhysicsSettings& s, const PtPhysicsAttractor* attractors, uint32_t n_attractors, float h)
{
    PhParams p{};
    p.h = h;
    p.restitution = s.Restitution; p.friction = s.Friction; p.baumgarte = s.Baumgarte; p.slop = s.Slop; p.bounce_threshold = s.BounceThreshold;
    p.n_attractors = n_attractors;
    for (uint32_t k = 0; k < n_attractors; k++) p.attractors[k] = attractors[k];
    return p;
}

// candidate pairs (lo < hi) of the step's positions: intervals along x, widened by more than any rounding of ph_contact
inline void candidate_pairs(const State& st, std::vector<std::pair<uint32_t, uint32_t>>& out)
{
    out.clear();
    std::vector<uint32_t> order(st.n);
    std::iota(order.begin(), order.end(), 0u);
    std::vector<float> lo(st.n), hi(st.n);
    for (uint32_t i = 0; i < st.n; i++) {
        const float pad = 1e-5f * (std::fabs(st.sph[i].x) + st.sph[i].w) + 1e-30f;
        lo[i] = st.sph[i].x - st.sph[i].w - pad;
        hi[i] = st.sph[i].x + st.sph[i].w + pad;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lo[a] < lo[b] || (lo[a] == lo[b] && a < b); });
    for (uint32_t a = 0; a < st.n; a++) {
        const uint32_t i = order[a];
        if (st.body[i].Flags & PT_PHYSICS_DISABLED) continue;
        for (uint32_t b = a + 1; b < st.n && lo[order[b]] <= hi[i]; b++) {
            const uint32_t j = order[b];
            if (st.body[j].Flags & PT_PHYSICS_DISABLED) continue;
            if (std::fabs(st.sph[i].y - st.sph[j].y) > 1.001f * (st.sph[i].w + st.sph[j].w) || std::fabs(st.sph[i].z - st.sph[j].z) > 1.001f * (st.sph[i].w + st.sph[j].w)) continue;
            out.emplace_back(std::min(i, j), std::max(i, j));
        }
    }
}

// one step of h; report: [0] += contacts, [1] |= clamped, [2] += frozen
inline void step(State& st, const PtPhysicsSettings& s, const PhParams& p, uint32_t report[3])
{
    const uint32_t n = st.n;
    for (uint32_t i = 0; i < n; i++) {
        st.vel_start[i] = st.vel[i];
        st.ang_start[i] = st.ang[i];
        const f3 a = ph_acceleration(st.sph.data(), i, st.body[i], p);
        PhVec4& v = st.vel[i];
        v.x = v.x + p.h * a.x; v.y = v.y + p.h * a.y; v.z = v.z + p.h * a.z;
        st.v0[i] = v;
        st.count[i] = 0u;
    }
    if (n > 1u) {
        std::vector<std::pair<uint32_t, uint32_t>> cand, pairs;
        candidate_pairs(st, cand);
        for (const auto& [lo, hi] : cand) {
            f3 nrm;
            float pen;
            if (!ph_contact(st.sph[lo], st.sph[hi], nrm, pen)) continue;
            // S27.4: exactly one of the lower body's walk, the higher body's walk and the LARGE list handles the pair
            const uint32_t handlers = (st.walks[lo] && ph_walker_handles(st.sph[lo].w, lo, st.sph[hi].w, hi, st.walks[hi] != 0) ? 1u : 0u)
                                      + (st.walks[hi] && ph_walker_handles(st.sph[hi].w, hi, st.sph[lo].w, lo, st.walks[lo] != 0) ? 1u : 0u)
                                      + (!st.walks[lo] && !st.walks[hi] ? 1u : 0u);
            if (handlers != 1u) st.rule_violations++;
            pairs.emplace_back(lo, hi);
            st.count[lo]++;
            st.count[hi]++;
            report[0]++;
        }
        const uint32_t iterations = s.Iterations ? s.Iterations : 4u;
        for (uint32_t it = 0; it < iterations; it++) {
            bool clamped = false;
            for (const auto& [lo, hi] : pairs) {
                PhPair q;
                q.sa = st.sph[lo]; q.sb = st.sph[hi];
                q.va = ph_xyz(st.vel[lo]); q.vb = ph_xyz(st.vel[hi]);
                q.wa = ph_xyz(st.ang[lo]); q.wb = ph_xyz(st.ang[hi]);
                q.v0a = ph_xyz(st.v0[lo]); q.v0b = ph_xyz(st.v0[hi]);
                q.ima = st.body[lo].InvMass; q.imb = st.body[hi].InvMass;
                q.na = st.count[lo]; q.nb = st.count[hi];
                PhImpulse r;
                if (!ph_pair_impulse(q, p, r)) continue;
                long long* a = &st.acc[(size_t)lo * kPhAccPerBody];
                long long* b = &st.acc[(size_t)hi * kPhAccPerBody];
                a[0] += ph_quantize(r.dva.x, clamped); a[1] += ph_quantize(r.dva.y, clamped); a[2] += ph_quantize(r.dva.z, clamped);
                a[3] += ph_quantize(r.dwa.x, clamped); a[4] += ph_quantize(r.dwa.y, clamped); a[5] += ph_quantize(r.dwa.z, clamped);
                b[0] += ph_quantize(r.dvb.x, clamped); b[1] += ph_quantize(r.dvb.y, clamped); b[2] += ph_quantize(r.dvb.z, clamped);
                b[3] += ph_quantize(r.dwb.x, clamped); b[4] += ph_quantize(r.dwb.y, clamped); b[5] += ph_quantize(r.dwb.z, clamped);
            }
            if (clamped) report[1] |= 1u;
            for (uint32_t i = 0; i < n; i++) {
                long long* a = &st.acc[(size_t)i * kPhAccPerBody];
                PhVec4 &v = st.vel[i], &w = st.ang[i];
                v.x = ph_apply(v.x, a[0]); v.y = ph_apply(v.y, a[1]); v.z = ph_apply(v.z, a[2]);
                w.x = ph_apply(w.x, a[3]); w.y = ph_apply(w.y, a[4]); w.z = ph_apply(w.z, a[5]);
                for (uint32_t k = 0; k < kPhAccPerBody; k++) a[k] = 0;
            }
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        if (st.body[i].Flags & PT_PHYSICS_DISABLED) continue;
        if (!ph_integrate(st.sph[i], st.rot[i], ph_xyz(st.vel[i]), ph_xyz(st.ang[i]), p.h)) {
            st.vel[i] = st.vel_start[i];
            st.ang[i] = st.ang_start[i];
            st.body[i].Flags |= PT_PHYSICS_DISABLED;
            report[2]++;
        }
    }
    st.steps++;
}

}  // namespace phhost
