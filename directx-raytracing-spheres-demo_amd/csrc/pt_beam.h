// pt_beam.h -- primary beams (DESIGN.md "Primary beams"): the widened pyramid of an 8x8 block's camera rays and its conservative tests
// against a BVH box and a padded leaf box.  Plain functions of floats, compiled for the device (beam_kernel and the shares of a moving
// camera's build inside bounce_kernel, pt_trace.h beam_walk_block) and as host C++ by the tests (tests/hostshim/beam_host.cpp, which
// tests/test_primary_beams.py checks against float64 brute force).  pt_beam_cache.h holds the host half: which later poses may use the lists.
#pragma once

#include "pt_texture.h"

#if defined(__HIPCC__)
#define PT_BEAM_FN __device__ __forceinline__
#else
#include <math.h>
#define PT_BEAM_FN inline
#endif

namespace pt {

// Camera rays of one 8x8-pixel block (= one wave64 of the primary pass) share their origin and span a thin pyramid.  One
// lane per block walks the BVH with that pyramid (four planes through the camera position, a pixel wider than the block on
// every side: half a pixel for any jitter in [-0.5, 0.5], half a pixel of slack) and lists the spheres whose padded leaf boxes it meets -- at most kBeamListCap; the primary pass then
// tests exactly those spheres for all 64 rays with wave-uniform control flow instead of 64 divergent stack traversals
// (DESIGN.md "Primary beams").  The list is a superset of every sphere any ray of the block can hit: a ray inside the
// pyramid that passes a leaf's padded box (the per-ray slab test's precondition for testing the sphere) means that box
// meets the pyramid; rounding in the plane tests is covered by the half-pixel widening plus an explicit relative margin.
// Closest hit over a superset with the same intersect_sphere and the same tie rule = the per-ray traversal's answer, bit
// for bit.  Record = 16 dwords: { count, original sphere ids[15] }; count > kBeamListCap = overflow, the wave traverses.
constexpr uint32_t kBeamListCap = 15;
constexpr uint32_t kBeamRecord = 16;

struct Beam {
    f3 o;
    f3 n[4];  // inward unit normals of the four side planes (zero vector = plane that culls nothing)
    float slack;  // every plane is moved outwards by this distance: the lists then hold for every camera position within `slack` of o
                  // (same orientation): a point x of the pyramid with apex o' has n.(x - o) = n.(x - o') + n.(o' - o) >= -|o' - o|
};

// 1 / sqrt(x) for a plane's normalisation: the device's approximate instruction (1 ulp); the host build rounds twice (no tighter).
// The two are different arithmetic: tests/test_leaf_edges.py runs the bounds below with the host value moved one float either way, and
// tests/test_gpu_leaf_edges.py runs them on planes and decisions computed by the gfx950 build.  What keeps a block's rays inside is the
// half pixel of slack of beam_corners (>= 2e-4 rad at a 10 degree lens), far above a plane test's rounding: P1 also holds with the 4e-6
// factor of beam_meets_box set to 0, on either side.  That factor is a second defence, not what the tests depend on.
#if defined(__HIPCC__)
PT_BEAM_FN float beam_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
#elif defined(PT_BEAM_RSQ_TEST)
// Host test builds only (tests/hostshim/leaf_batch_host.cpp; the product never defines it): the host value moved by
// pt_beam_rsq_test_ulps floats, so that the CPU tests run the bounds below with the device's error class, in both directions.
extern int pt_beam_rsq_test_ulps;
PT_BEAM_FN float beam_rsq(float x)
{
    float r = 1.0f / sqrtf(x);
    for (int k = pt_beam_rsq_test_ulps; k > 0; k--) r = nextafterf(r, kInf);
    for (int k = pt_beam_rsq_test_ulps; k < 0; k++) r = nextafterf(r, -kInf);
    return r;
}
#else
PT_BEAM_FN float beam_rsq(float x) { return 1.0f / sqrtf(x); }
#endif

PT_BEAM_FN f3 beam_plane(f3 a, f3 b, f3 inside)
{
    f3 n = cross(a, b);
    if (dot(n, inside) < 0.0f) n = -n;
    const float l2 = dot(n, n);
    if (!(l2 > 0.0f) || !is_finite(l2)) return make_f3(0.f, 0.f, 0.f);
    return n * beam_rsq(l2);
}

// The directions (not normalised) of the four corner rays of the block at (px, py): c[0..3] = c00, c10, c11, c01 of make_beam.
PT_BEAM_FN void beam_corners(const CameraParams& cam, uint32_t px, uint32_t py, float margin_px, f3 c[4])
{
    // NDC of the block's outline: its pixel centres lie in [px, px + 8] for every jitter in [-0.5, 0.5] (the host checks the
    // jitter), widened by half a pixel each way -- the lists serve every frame of a resting view
    // (margin_px more on every side: the lists then hold for every orientation whose rays leave the image within that many pixels of where
    // this one's do -- a camera that turns; pt_beam_cache.h beam_within bounds the displacement)
    const float xa = ((float)px - 0.5f - margin_px) * cam.InvW, xb = ((float)px + 8.5f + margin_px) * cam.InvW;
    const float ya = ((float)py - 0.5f - margin_px) * cam.InvH, yb = ((float)py + 8.5f + margin_px) * cam.InvH;
    const float nxa = pt_fma(xa, 2.0f, -1.0f), nxb = pt_fma(xb, 2.0f, -1.0f), nya = pt_fma(ya, -2.0f, 1.0f), nyb = pt_fma(yb, -2.0f, 1.0f);
    const f3 c00 = mad(nya, cam.Up, cam.Right * nxa) + cam.Forward, c10 = mad(nya, cam.Up, cam.Right * nxb) + cam.Forward;
    const f3 c11 = mad(nyb, cam.Up, cam.Right * nxb) + cam.Forward, c01 = mad(nyb, cam.Up, cam.Right * nxa) + cam.Forward;
    c[0] = c00; c[1] = c10; c[2] = c11; c[3] = c01;
}

PT_BEAM_FN Beam make_beam(const CameraParams& cam, uint32_t px, uint32_t py, float slack, float margin_px = 0.0f)
{
    f3 c[4];
    beam_corners(cam, px, py, margin_px, c);
    const f3 c00 = c[0], c10 = c[1], c11 = c[2], c01 = c[3];
    const f3 mid = (c00 + c11) + (c10 + c01);
    Beam b;
    b.o = cam.Position;
    b.slack = slack;
    b.n[0] = beam_plane(c00, c10, mid);
    b.n[1] = beam_plane(c10, c11, mid);
    b.n[2] = beam_plane(c11, c01, mid);
    b.n[3] = beam_plane(c01, c00, mid);
    return b;
}

// false = the box lies outside one of the planes for certain (NaNs compare false everywhere: never culled)
PT_BEAM_FN bool beam_meets_box(const Beam& b, f3 lo, f3 hi)
{
    const f3 l = lo - b.o, h = hi - b.o;
    const float mag = pt_max(__builtin_fabsf(l.x), __builtin_fabsf(h.x)) + pt_max(__builtin_fabsf(l.y), __builtin_fabsf(h.y)) + pt_max(__builtin_fabsf(l.z), __builtin_fabsf(h.z));
    const float margin = -4e-6f * (mag + b.slack) - b.slack;
    bool meets = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) {
        const f3 n = b.n[k];
        // the box corner farthest along the inward normal
        const float d = pt_max(n.x * l.x, n.x * h.x) + pt_max(n.y * l.y, n.y * h.y) + pt_max(n.z * l.z, n.z * h.z);
        if (d < margin) meets = false;
    }
    return meets;
}

// leaf: the sphere that encloses the padded leaf box's inscribed sphere (centre = box centre, radius = largest half extent
// >= r + padding) against the planes
PT_BEAM_FN bool beam_meets_leaf(const Beam& b, f3 lo, f3 hi)
{
    const f3 c = (lo + hi) * 0.5f - b.o;
    const f3 e = (hi - lo) * 0.5f;
    const float r = pt_max(e.x, pt_max(e.y, e.z));
    const float margin = -(r + b.slack + 4e-6f * (__builtin_fabsf(c.x) + __builtin_fabsf(c.y) + __builtin_fabsf(c.z) + r + b.slack));
    bool meets = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++)
        if (dot(b.n[k], c) < margin) meets = false;
    return meets;
}

}  // namespace pt
