// pt_physics.h -- row N23: the rules of the rigid-sphere dynamics step (pt_physics_*, a stand-in for PhysX; DESIGN.md spec S27) as PT_HD
// functions.  The kernels (pt_physics.hip) and the host (host/Physics.hpp, tests/hostshim/physics_host.cpp) compile this one text with
// -ffp-contract=off: the device state equals the host's bit for bit.  What a pair adds to a body goes through 64-bit fixed-point
// accumulators (integer addition is associative), so a step depends on neither the tree nor the order in which pairs are met.
#pragma once

#include "pt_math.h"
#include "../../include/pt_types.h"

namespace pt {

struct alignas(16) PhVec4 {
    float x, y, z, w;
};

// internal to the device copy of PtPhysicsBody::Flags: a LARGE body inside the cap -- it does not walk the tree (S27.4)
constexpr uint32_t kPhNoWalk = 0x100u;
constexpr uint32_t kPhFlagMask = PT_PHYSICS_SPRING | PT_PHYSICS_LARGE | PT_PHYSICS_DISABLED;

// S27.6: a contribution is rounded once to a multiple of 2^-24 (m/s, rad/s) and clamped to +-2^15: at most 2^39 quanta, so 2^23
// contributions to one accumulator stay below 2^62 (a body of 2^20 contacts receives 2^20 per iteration; the apply kernel clears them)
constexpr float kPhScale = 16777216.0f;      // 1 / quantum
constexpr float kPhQuantum = 1.0f / 16777216.0f;
constexpr float kPhClamp = 32768.0f;
constexpr uint32_t kPhAccPerBody = 6;        // dv.xyz, dw.xyz

struct PhParams {
    float h;                // the step
    float restitution, friction, baumgarte, slop, bounce_threshold;
    uint32_t n_attractors;
    PtPhysicsAttractor attractors[PT_PHYSICS_MAX_ATTRACTORS];
};

PT_HD f3 ph_cross(f3 a, f3 b) { return make_f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
PT_HD f3 ph_xyz(PhVec4 v) { return make_f3(v.x, v.y, v.z); }
PT_HD bool ph_finite3(f3 v) { return is_finite(v.x) && is_finite(v.y) && is_finite(v.z); }

// S27.2: the acceleration of body i at the step's positions (sph: every body's centre and radius).  Immovable and DISABLED bodies take none.
PT_HD f3 ph_acceleration(const PhVec4* sph, uint32_t i, const PtPhysicsBody& b, const PhParams& p)
{
    f3 a = make_f3(0.0f, 0.0f, 0.0f);
    if (!(b.InvMass > 0.0f) || (b.Flags & PT_PHYSICS_DISABLED)) return a;
    const f3 x = ph_xyz(sph[i]);
    if (b.Flags & PT_PHYSICS_SPRING) a.y = -(b.SpringOmega2 * (x.y - b.SpringY0));
    for (uint32_t k = 0; k < p.n_attractors; k++) {
        const PtPhysicsAttractor& t = p.attractors[k];
        if (t.Body == i || (t.Target != PT_PHYSICS_ALL_BODIES && t.Target != i)) continue;
        const f3 d = ph_xyz(sph[t.Body]) - x;
        const float d2 = dot(d, d);
        if (!(d2 > 0.0f)) continue;  // a distance of 0 exerts no force
        const float dist = pt_sqrt(d2);
        const float mag = t.Kind == PT_PHYSICS_INVERSE_SQUARE ? t.Strength / d2 : t.Strength;
        a = a + d * (mag / dist);
    }
    return a;
}

// S27.3: the discrete contact test, arguments in canonical order (a = the lower index).  n: the unit normal from a to b (+y when the
// centres coincide), pen: the penetration depth.
PT_HD bool ph_contact(PhVec4 sa, PhVec4 sb, f3& n, float& pen)
{
    const f3 d = ph_xyz(sb) - ph_xyz(sa);
    const float dist = pt_sqrt(dot(d, d));
    const float reach = sa.w + sb.w;
    if (!(dist < reach)) return false;
    n = dist > 0.0f ? d * (1.0f / dist) : make_f3(0.0f, 1.0f, 0.0f);
    pen = reach - dist;
    return true;
}

// S27.4: whether walking body i (radius ri) handles its pair with j: always when j does not walk, else the smaller radius, a tie to the
// lower index
PT_HD bool ph_walker_handles(float ri, uint32_t i, float rj, uint32_t j, bool j_walks) { return !j_walks || ri < rj || (ri == rj && i < j); }

struct PhPair {  // a = the lower index
    PhVec4 sa, sb;            // centre, radius
    f3 va, wa, vb, wb;        // current linear and angular velocities
    f3 v0a, v0b;              // pre-solve linear velocities
    float ima, imb;           // inverse masses
    uint32_t na, nb;          // contact counts
};
struct PhImpulse {
    f3 dva, dwa, dvb, dwb;
    float lambda, jt;         // the normal and the friction impulse (tests)
};

// S27.5: one pair of one Jacobi iteration.  false: not in contact, or both bodies immovable (nothing is added).
PT_HD bool ph_pair_impulse(const PhPair& q, const PhParams& p, PhImpulse& out)
{
    f3 n;
    float pen;
    if (!ph_contact(q.sa, q.sb, n, pen)) return false;
    const float den = (float)q.na * q.ima + (float)q.nb * q.imb;
    if (!(den > 0.0f)) return false;
    const float vn = dot(q.vb - q.va, n), vn0 = dot(q.v0b - q.v0a, n);
    const float target = -vn0 > p.bounce_threshold ? -(p.restitution * vn0) : 0.0f;
    const float bias = p.baumgarte * pt_max(0.0f, pen - p.slop) / p.h;
    const float lambda = pt_max(0.0f, (target + bias - vn) / den);
    // the relative velocity of b's contact point against a's, spin included
    const f3 vrel = (q.vb + ph_cross(q.wb, n * -q.sb.w)) - (q.va + ph_cross(q.wa, n * q.sa.w));
    const f3 vt = vrel - n * dot(vrel, n);
    const float tl = pt_sqrt(dot(vt, vt));
    f3 J = n * lambda;  // the impulse on b; a takes its negation
    float jt = 0.0f;
    if (p.friction > 0.0f && tl > 0.0f) {
        jt = pt_min(tl / (3.5f * den), p.friction * lambda);
        J = J - vt * (jt / tl);
    }
    const f3 nxJ = ph_cross(n, J);
    out.dvb = J * q.imb;
    out.dva = -(J * q.ima);
    // solid spheres: 1 / I = 2.5 / (m r^2); the lever arms are +ra n and -rb n, so both spins change by -(r / I) n x J
    out.dwa = nxJ * -(2.5f * q.ima / q.sa.w);
    out.dwb = nxJ * -(2.5f * q.imb / q.sb.w);
    out.lambda = lambda;
    out.jt = jt;
    return true;
}

// S27.6: one component of a contribution in quanta; `clamped` is set (never cleared) when the clamp acted (a NaN counts as 0)
PT_HD long long ph_quantize(float x, bool& clamped)
{
    if (!(pt_abs(x) <= kPhClamp)) {
        clamped = true;
        x = x != x ? 0.0f : (x > 0.0f ? kPhClamp : -kPhClamp);
    }
    return (long long)__builtin_rintf(x * kPhScale);
}
PT_HD float ph_apply(float v, long long acc) { return acc != 0 ? v + (float)acc * kPhQuantum : v; }

// S27.7: x += h v, q += h/2 (w, 0) q, renormalised.  false: a result is not finite (the caller freezes the body); nothing is written then.
PT_HD bool ph_integrate(PhVec4& s, PhVec4& rot, f3 v, f3 w, float h)
{
    const f3 x = ph_xyz(s) + v * h;
    const float k = 0.5f * h;
    const f3 qv = make_f3(rot.x, rot.y, rot.z);
    const f3 dv = w * rot.w + ph_cross(w, qv);
    const float qx = rot.x + k * dv.x, qy = rot.y + k * dv.y, qz = rot.z + k * dv.z, qw = rot.w - k * dot(w, qv);
    const float len = pt_sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    const float inv = 1.0f / len;
    const f3 qn = make_f3(qx * inv, qy * inv, qz * inv);
    const float qwn = qw * inv;
    if (!(len > 0.0f) || !is_finite(len) || !ph_finite3(x) || !ph_finite3(v) || !ph_finite3(w) || !ph_finite3(qn) || !is_finite(qwn)) return false;
    s.x = x.x; s.y = x.y; s.z = x.z;
    rot.x = qn.x; rot.y = qn.y; rot.z = qn.z; rot.w = qwn;
    return true;
}

#if defined(__HIPCC__)
struct SceneView;
// the device state of pt_physics_* (all arrays of n records)
struct PhDevice {
    PhVec4* sph;         // centre, radius: the layout of pt_update_spheres
    PhVec4* rot;         // orientation (x, y, z, w): the layout of pt_update_rotations
    PhVec4* vel;         // linear velocity (w unused)
    PhVec4* ang;         // angular velocity
    PhVec4* v0;          // pre-solve linear velocity of the step
    PhVec4* vel_start;   // the velocities the step started from (a frozen body returns to them)
    PhVec4* ang_start;
    PtPhysicsBody* body;
    uint32_t* count;     // contacts of the step
    long long* acc;      // kPhAccPerBody accumulators per body
    uint32_t* report;    // [0] contacts, [1] clamped, [2] frozen
    const uint32_t* large;  // the LARGE bodies that do not walk
    uint32_t n, n_large;
};
hipError_t launch_physics_forces(const PhDevice& d, const PhParams& p, hipStream_t stream);
// the tree walk of the walking bodies and the brute-force pass over the LARGE list: counting (count = true) or one Jacobi iteration
hipError_t launch_physics_pairs(const SceneView& sv, const PhDevice& d, const PhParams& p, bool count, hipStream_t stream);
hipError_t launch_physics_apply(const PhDevice& d, hipStream_t stream);
hipError_t launch_physics_integrate(const PhDevice& d, const PhParams& p, hipStream_t stream);
#endif

}  // namespace pt
