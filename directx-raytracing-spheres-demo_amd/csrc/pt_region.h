// pt_region.h -- reflection beams (DESIGN.md "Reflection beams"): the region record of an 8x8 block whose camera rays all land on one
// mirror-like sphere, the conservative test of a BVH box against the region, and the run-time test of a spawned ray.  Plain functions of
// floats, compiled for the device (beam_kernel builds the records, bounce_kernel reads them) and as host C++ by the tests
// (tests/hostshim/region_host.cpp).
//
// A region is the swept set R = { o + t d : o in O, d in the cone (axis a, half-angle theta), t >= 0 } of an axis-aligned origin box O.
// Its candidate list holds every sphere whose padded leaf box meets R.  A bounce-1 ray (o, d) with o in O and angle(d, a) <= theta lies
// in R for every t >= 0, so every sphere it can hit is on the list, and the closest hit over the list (same intersect_sphere, same tie
// rule) is the traversal's answer bit for bit -- whatever surface the ray left: the geometry below only decides how often rays fall
// outside their block's region (and then traverse), never what they hit.
#pragma once

#include "pt_bsdf.h"

#if !defined(__HIPCC__)
#include <math.h>
#endif

namespace pt {

// Record (kReflRecord dwords per 8x8 block): { count, O.lo[3], O.hi[3], axis[3], cos_run, ids[kReflListCap] }.  count = 0: no region
// (the block failed a test of region_from_hits, or its list overflowed); else 1..kReflListCap ids, with their alpha class bits.
constexpr uint32_t kReflRecord = 32;
constexpr uint32_t kReflIds = 11;  // first id
constexpr uint32_t kReflListCap = kReflRecord - kReflIds;
// A block gets a region only for a sphere whose (clamped) roughness is at most this: the GGX half-vector of vndf_ray then leaves the
// normal by more than kReflGgxCap only for u1 within (kReflMaxRoughness^2 / kReflGgxCap)^2 ~ 1.5e-5 of 1 (tan = m sqrt(u1 / (1 - u1))).
constexpr float kReflMaxRoughness = 2.5e-3f;
constexpr float kReflGgxCap = 2e-3f;       // radians the sampled half-vector may leave the normal (the reflection then turns by twice that)
constexpr float kReflMinCos = 0.05f;       // every hit of the block's pyramid at least this far from grazing (bounds the footprint's bulge)
constexpr float kReflMaxTheta = 0.5f;      // wider cones are not worth a list
constexpr float kReflCosMargin = 4e-6f;    // the list's cone is this much wider in cosine than cos_run: covers the rounding of dot(d, a) and |d|, |a| != 1
constexpr float kReflAngleMargin = 1e-4f;  // radians added to every angle bound of the box test (atan2f / asinf rounding)

struct ReflRegion {
    f3 lo, hi;       // O
    f3 axis;         // unit cone axis
    float theta;     // half-angle the candidate list is built for ...
    float cos_run;   // ... and the run-time test's threshold, kReflCosMargin above cos(theta)
};

PT_HD float r_len(f3 v) { return pt_sqrt(dot(v, v)); }
PT_HD float r_abs_sum(f3 v) { return pt_abs(v.x) + pt_abs(v.y) + pt_abs(v.z); }
PT_HD f3 r_cross(f3 a, f3 b) { return make_f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// angle between two nonzero vectors (any lengths), well conditioned near 0 and pi
PT_HD float r_angle(f3 u, f3 v) { return atan2f(r_len(r_cross(u, v)), dot(u, v)); }

// Can a ray of the region pass the box [lo, hi]?  false = certainly not.  R meets B iff the cone from O's centre c meets B enlarged by
// O's half-extents h (Minkowski sum); that box lies inside its bounding sphere (m, rho), and a cone (apex c, axis a, half-angle theta)
// meets a ball iff c is inside it or angle(m - c, a) <= theta + asin(rho / |m - c|).  The slop covers the rounding of c, h, m, rho and
// |m - c| (relative 1e-5 of the magnitudes involved); kReflAngleMargin covers atan2f / asinf.  NaN anywhere: true (never culled).
PT_HD bool region_meets_box(const ReflRegion& g, f3 lo, f3 hi)
{
    const f3 c = (g.lo + g.hi) * 0.5f;
    const f3 h = (g.hi - g.lo) * 0.5f;
    const f3 m = (lo + hi) * 0.5f;
    const f3 e = (hi - lo) * 0.5f + h;
    const f3 v = m - c;
    const float slop = 1e-5f * (r_abs_sum(c) + r_abs_sum(m) + r_abs_sum(e));
    const float rho = r_len(e) + slop;
    const float dist = r_len(v);
    if (!(dist > rho)) return true;  // the apex lies inside the ball (or NaN)
    const float ang = r_angle(v, g.axis);
    return !(ang > g.theta + asinf(rho / dist) + kReflAngleMargin);
}

// The run-time test of a spawned ray: o in O (six compares) and dot(d, a) >= cos_run.  With |d|, |a| within 1e-6 of 1 and the dot
// product's rounding below 1e-6, an accepted d makes an angle of at most g.theta with a.
PT_HD bool region_contains(const ReflRegion& g, f3 o, f3 d)
{
    return o.x >= g.lo.x && o.x <= g.hi.x && o.y >= g.lo.y && o.y <= g.hi.y && o.z >= g.lo.z && o.z <= g.hi.z && dot(d, g.axis) >= g.cos_run;
}

// The cone of a region: the run-time test accepts directions within `theta` of the axis (to rounding), the candidate list is built for the
// wider g.theta whose cosine is kReflCosMargin lower (plus acosf's rounding).
PT_HD void region_set_cone(ReflRegion& g, f3 axis, float theta)
{
    g.axis = axis;
    g.cos_run = cosf(theta);
    g.theta = acosf(pt_max(g.cos_run - kReflCosMargin, -1.0f)) + kReflAngleMargin;
}

// The region of a block from where its camera rays land.  cam_o: the camera position; dir[0..3]: unit directions of the pyramid's four
// corner rays, dir[4]: its centre ray; t[k]: where each meets the sphere (C, r) (all five must hit it first: the projection of a sphere
// is convex, so then every ray of the pyramid meets it).  Returns false when the block gets no region.
//   O: the box of the five hit points, widened by the footprint's bulge -- chord^2 / (8 r) for the cap itself, chord^2 / (8 r cos_min)
//      for an edge (the plane of two corner rays cuts the sphere in a circle of radius >= r cos_min) -- plus the spawn offset and slop.
//   cone: the centre ray reflected about the centre normal.  A lane's direction differs from it by at most the pyramid's angular radius
//      (incoming direction) + 2 x its normal's turn from the centre normal (<= |O| / r) + 2 x the GGX half-vector's tilt (kReflGgxCap).
PT_HD bool region_from_hits(f3 cam_o, const f3 dir[5], const float t[5], f3 C, float r, ReflRegion& g)
{
    f3 P[5];
    float cos_min = 1.0f, offset = 0.0f;
    for (int k = 0; k < 5; k++) {
        const HitFrame hf = hit_frame(cam_o, dir[k], t[k], C, r);
        P[k] = hf.P;
        cos_min = pt_min(cos_min, pt_abs(dot(hf.N, dir[k])));
        offset = pt_max(offset, hf.offset);
        if (!hf.front) return false;
    }
    if (!(cos_min >= kReflMinCos)) return false;
    f3 lo = P[0], hi = P[0];
    for (int k = 1; k < 5; k++) {
        lo = make_f3(pt_min(lo.x, P[k].x), pt_min(lo.y, P[k].y), pt_min(lo.z, P[k].z));
        hi = make_f3(pt_max(hi.x, P[k].x), pt_max(hi.y, P[k].y), pt_max(hi.z, P[k].z));
    }
    const float chord = r_len(hi - lo);
    const float bulge = chord * chord / (8.0f * r) * (1.0f + 1.0f / cos_min);
    const float pad = bulge * 1.01f + 2.0f * offset + 1e-5f * (r_abs_sum(C) + r) + 1e-3f * chord;
    g.lo = make_f3(lo.x - pad, lo.y - pad, lo.z - pad);
    g.hi = make_f3(hi.x + pad, hi.y + pad, hi.z + pad);
    const HitFrame hc = hit_frame(cam_o, dir[4], t[4], C, r);
    float pyr = 0.0f;
    for (int k = 0; k < 4; k++) pyr = pt_max(pyr, r_angle(dir[k], dir[4]));
    const f3 refl = dir[4] - hc.N * (2.0f * dot(dir[4], hc.N));
    const float turn = r_len(g.hi - g.lo) / r;
    region_set_cone(g, normalize(refl), pyr + 2.0f * turn + 2.0f * kReflGgxCap + kReflAngleMargin);
    return g.theta <= kReflMaxTheta && is_finite(g.cos_run) && is_finite(chord);
}

PT_HD void region_store(const ReflRegion& g, uint32_t* rec)
{
    const float v[10] = { g.lo.x, g.lo.y, g.lo.z, g.hi.x, g.hi.y, g.hi.z, g.axis.x, g.axis.y, g.axis.z, g.cos_run };
    for (int k = 0; k < 10; k++) rec[1 + k] = as_uint(v[k]);
}

}  // namespace pt
