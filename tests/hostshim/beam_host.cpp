// beam_host.cpp -- TEST SHIM: compiles the product's primary-beam headers (csrc/pt_beam.h: the device half; csrc/pt_beam_cache.h: the
// host half) as plain host C++ (the flags of devmath_host.cpp) so tests/test_primary_beams.py can check the pyramids and the poses that
// may use them against float64 brute force.  A camera travels as 12 floats (Position, Right, Up, Forward), a beam as 16 (o[3], n[4][3],
// slack), a basis as 9 (Right, Up, Forward).  Not part of the product; never loaded by it.
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_beam.h"
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_beam_cache.h"

using namespace pt;

static f3 v3(const float* p) { return make_f3(p[0], p[1], p[2]); }
static PtCamera camera(const float* c, float jx, float jy)
{
    PtCamera cam{};
    for (int i = 0; i < 3; i++) { cam.Position[i] = c[i]; cam.RightDirection[i] = c[3 + i]; cam.UpDirection[i] = c[6 + i]; cam.ForwardDirection[i] = c[9 + i]; }
    cam.NearDepth = 0.0f; cam.FarDepth = kInf; cam.Jitter[0] = jx; cam.Jitter[1] = jy;
    return cam;
}
static Beam unpack(const float* g)
{
    Beam b;
    b.o = v3(g);
    for (int k = 0; k < 4; k++) b.n[k] = v3(g + 3 + 3 * k);
    b.slack = g[15];
    return b;
}
static BeamLens lens_of(uint32_t w, uint32_t h, const float* basis) { return beam_lens(w, h, beam_len3(basis), beam_len3(basis + 3), beam_len3(basis + 6)); }

extern "C" {

// make_beam for the block at (px, py) of a w x h image
void bm_make(const float* cam, uint32_t w, uint32_t h, uint32_t px, uint32_t py, float slack, float margin_px, float* g)
{
    const Beam b = make_beam(camera_params(camera(cam, 0.0f, 0.0f), w, h), px, py, slack, margin_px);
    g[0] = b.o.x; g[1] = b.o.y; g[2] = b.o.z;
    for (int k = 0; k < 4; k++) { g[3 + 3 * k] = b.n[k].x; g[4 + 3 * k] = b.n[k].y; g[5 + 3 * k] = b.n[k].z; }
    g[15] = b.slack;
}

// n boxes (lo[3], hi[3] each) against one beam: out[i] = beam_meets_box / beam_meets_leaf
void bm_meets_boxes(const float* g, uint32_t n, const float* boxes, uint8_t* out)
{
    const Beam b = unpack(g);
    for (uint32_t i = 0; i < n; i++) out[i] = beam_meets_box(b, v3(boxes + 6 * i), v3(boxes + 6 * i + 3)) ? 1 : 0;
}
void bm_meets_leaves(const float* g, uint32_t n, const float* boxes, uint8_t* out)
{
    const Beam b = unpack(g);
    for (uint32_t i = 0; i < n; i++) out[i] = beam_meets_leaf(b, v3(boxes + 6 * i), v3(boxes + 6 * i + 3)) ? 1 : 0;
}

// n camera rays as the kernels form them (primary_ray): pixel (pix[2 i], pix[2 i + 1]) with jitter (jit[2 i], jit[2 i + 1]) from
// position pos[3 i ..] (the camera's own when pos is null): o and d, 3 floats per ray
void bm_rays(const float* cam, uint32_t w, uint32_t h, uint32_t n, const uint32_t* pix, const float* jit, const float* pos, float* o, float* d)
{
    for (uint32_t i = 0; i < n; i++) {
        PtCamera c = camera(cam, jit[2 * i], jit[2 * i + 1]);
        if (pos) for (int k = 0; k < 3; k++) c.Position[k] = pos[3 * i + k];
        f3 oo, dd;
        float tmin, tmax;
        primary_ray(camera_params(c, w, h), pix[2 * i], pix[2 * i + 1], oo, dd, tmin, tmax);
        o[3 * i] = oo.x; o[3 * i + 1] = oo.y; o[3 * i + 2] = oo.z;
        d[3 * i] = dd.x; d[3 * i + 1] = dd.y; d[3 * i + 2] = dd.z;
    }
}

// out[i * n_sph + j] = intersect_sphere(ray i, sphere j (cx, cy, cz, r)) over t in (0, inf): what the kernels would find
void bm_hits(uint32_t n_rays, const float* o, const float* d, uint32_t n_sph, const float* sph, uint8_t* out)
{
    for (uint32_t i = 0; i < n_rays; i++)
        for (uint32_t j = 0; j < n_sph; j++) {
            float t;
            out[(size_t)i * n_sph + j] = intersect_sphere(v3(o + 3 * i), v3(d + 3 * i), 0.0f, kInf, v3(sph + 4 * j), sph[4 * j + 3], t) ? 1 : 0;
        }
}

// ---- pt_beam_cache.h.  The lens is that of `lens_basis` (beam_cache_lookup takes the current frame's axes).
void bc_lens(uint32_t w, uint32_t h, const float* lens_basis, double out[3])
{
    const BeamLens l = lens_of(w, h, lens_basis);
    out[0] = l.f_px; out[1] = l.corner; out[2] = l.half_diag_px;
}
double bc_rotation_between(const float* p, const float* q, double rot[3]) { return beam_rotation_between(p, q, rot); }
double bc_turn_px(uint32_t w, uint32_t h, const float* lens_basis, double angle) { return beam_turn_px(lens_of(w, h, lens_basis), angle); }
double bc_lens_px(uint32_t w, uint32_t h, const float* lens_basis, const float* p, const float* q) { return beam_lens_px(lens_of(w, h, lens_basis), p, q); }
int bc_same_lens(uint32_t w, uint32_t h, const float* lens_basis, const float* p, const float* q) { return beam_same_lens(lens_of(w, h, lens_basis), p, q) ? 1 : 0; }
int bc_within(uint32_t w, uint32_t h, const float* b_pos, const float* b_basis, float slack, float margin_px, const float* q_pos, const float* q_basis)
{
    return beam_within(lens_of(w, h, q_basis), b_pos, b_basis, slack, margin_px, q_pos, q_basis) ? 1 : 0;
}
void bc_ahead(const float* pos, const double* v, const float* basis, const double* turn, double turned, double f, float* out_pos, float* out_basis)
{
    beam_ahead(pos, v, basis, turn, turned, f, out_pos, out_basis);
}
// out: span, centre_ahead, slack, margin_px
void bc_plan(uint32_t w, uint32_t h, const float* lens_basis, double step, double acc, double turned, double turn_acc, double n_build, double lanes, double reach,
             double max_slack, double max_margin, double out[4])
{
    const BeamPlan p = beam_plan(lens_of(w, h, lens_basis), step, acc, turned, turn_acc, n_build, lanes, reach, max_slack, max_margin);
    out[0] = p.span; out[1] = p.centre_ahead; out[2] = p.slack; out[3] = p.margin_px;
}

}
