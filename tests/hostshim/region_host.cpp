// region_host.cpp -- TEST SHIM: compiles the product's reflection-beam header (csrc/pt_region.h) as plain host C++ (the flags of
// devmath_host.cpp) so tests/test_refl_region.py can check its box test, its run-time test and its record building against float64
// brute force.  A region travels as 11 floats: lo[3], hi[3], axis[3], theta, cos_run.  Not part of the product; never loaded by it.
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_region.h"

using namespace pt;

static f3 v3(const float* p) { return make_f3(p[0], p[1], p[2]); }
static ReflRegion unpack(const float* g)
{
    ReflRegion r;
    r.lo = v3(g); r.hi = v3(g + 3); r.axis = v3(g + 6); r.theta = g[9]; r.cos_run = g[10];
    return r;
}
static void pack(const ReflRegion& r, float* g)
{
    const float v[11] = { r.lo.x, r.lo.y, r.lo.z, r.hi.x, r.hi.y, r.hi.z, r.axis.x, r.axis.y, r.axis.z, r.theta, r.cos_run };
    for (int k = 0; k < 11; k++) g[k] = v[k];
}

extern "C" {

// a region from O, a unit axis and theta (region_set_cone)
void rg_make(const float lo[3], const float hi[3], const float axis[3], float theta, float* g)
{
    ReflRegion r;
    r.lo = v3(lo); r.hi = v3(hi);
    region_set_cone(r, v3(axis), theta);
    pack(r, g);
}

// n boxes (lo[3], hi[3] each) against one region: out[i] = region_meets_box
void rg_meets_boxes(const float* g, uint32_t n, const float* boxes, uint8_t* out)
{
    const ReflRegion r = unpack(g);
    for (uint32_t i = 0; i < n; i++) out[i] = region_meets_box(r, v3(boxes + 6 * i), v3(boxes + 6 * i + 3)) ? 1 : 0;
}

// n rays (o[3], d[3] each): out[i] = region_contains
void rg_contains(const float* g, uint32_t n, const float* rays, uint8_t* out)
{
    const ReflRegion r = unpack(g);
    for (uint32_t i = 0; i < n; i++) out[i] = region_contains(r, v3(rays + 6 * i), v3(rays + 6 * i + 3)) ? 1 : 0;
}

// the record of a block whose five rays (cam_o, dirs[3 k .. 3 k + 2]; k = 4: the centre ray) meet the sphere (C, r): 1 and g, or 0
// (a ray misses the sphere, or region_from_hits declines)
int rg_from_rays(const float cam_o[3], const float* dirs, const float C[3], float r, float* g)
{
    f3 dir[5];
    float t[5];
    for (int k = 0; k < 5; k++) {
        dir[k] = v3(dirs + 3 * k);
        if (!intersect_sphere(v3(cam_o), dir[k], 0.0f, kInf, v3(C), r, t[k])) return 0;
    }
    ReflRegion reg;
    if (!region_from_hits(v3(cam_o), dir, t, v3(C), r, reg)) return 0;
    pack(reg, g);
    return 1;
}

// A lane's bounce-1 ray as the kernels form it for a mirror: the camera ray d meets the sphere, the half-vector is the normal tilted
// by `tilt` radians towards angle phi of its tangent frame, L = reflect(-V, H), o = spawn_origin.  0 = the camera ray misses.
int rg_lane(const float cam_o[3], const float d[3], const float C[3], float r, float tilt, float phi, float* o, float* L)
{
    float t;
    if (!intersect_sphere(v3(cam_o), v3(d), 0.0f, kInf, v3(C), r, t)) return 0;
    const HitFrame hf = hit_frame(v3(cam_o), v3(d), t, v3(C), r);
    const Basis b = get_basis(hf.N);
    const float tn = tanf(tilt);
    const f3 H = normalize(hf.N + (b.T * (tn * cosf(phi)) + b.B * (tn * sinf(phi))));
    const f3 l = reflect(v3(d), H);
    const f3 so = spawn_origin(hf.P, hf.N, hf.offset, l);
    o[0] = so.x; o[1] = so.y; o[2] = so.z;
    L[0] = l.x; L[1] = l.y; L[2] = l.z;
    return 1;
}

}
