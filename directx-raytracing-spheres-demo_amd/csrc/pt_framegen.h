// pt_framegen.h -- the frame-interpolation stand-in (row N13): the frame half way between two rendered ones, made from the resources the
// reference tags for Streamline's DLSS-G plugin (App::ProcessDLSSFrameGeneration, Source/App.cpp:1673-1680): the G-buffer depth, the
// motion vectors and the tone-mapped HUD-less colour.  The plugin is a closed SDK that is not vendored; the arithmetic is this project's
// own, frozen by DESIGN.md spec S19: every render pixel is scattered half its motion vector back through a depth-tested 64-bit min
// (nearest surface wins, equal depths go to the lowest source index), then every output pixel gathers the current frame half a vector
// ahead and the previous frame half a vector behind and averages what is valid.
// Per-pixel functions for the kernels of pt_framegen.hip; they also compile as host C++ (tests/hostshim/framegen_host.cpp), where the
// min is a plain sequential one, so the GPU output is pinned bit for bit to the host-compiled header (a min does not depend on the
// order of its operands).  fp32 throughout, no contraction (-ffp-contract=off); pt_fma only in the bilinear lerps.
#pragma once

#include "pt_texture.h"

namespace pt {

constexpr uint32_t kFgMaxSize = 16384, kFgMaxRatio = 4;
constexpr uint32_t kFgFormatRGBA8 = 0, kFgFormatRGB10A2 = 1;  // pt_tonemap's two packings (pt_post.h: tonemap_pixel)
constexpr float kFgDepthRel = 0.1f;                           // |z_prev - (z + mv.z)| <= 0.1 (z + mv.z), spec S17's rule
constexpr unsigned long long kFgHole = ~0ull;                 // a field entry no render pixel reached
constexpr int kFgBlockW = 32, kFgBlockH = 8;

struct FgParams {
    uint32_t w, h, W, H;  // RenderSize and OutputSize
    float sx, sy;         // W / w, H / h
    float rx, ry;         // w / W, h / H
    uint32_t format;
};

PT_HD FgParams fg_params(uint32_t w, uint32_t h, uint32_t W, uint32_t H, uint32_t format)
{
    FgParams P;
    P.w = w; P.h = h; P.W = W; P.H = H;
    P.sx = (float)W / (float)w; P.sy = (float)H / (float)h;
    P.rx = (float)w / (float)W; P.ry = (float)h / (float)H;
    P.format = format;
    return P;
}

// The buffers of one call: the caller's (PtFrameGenTextures) and the context's.  prev_* = the history slot the previous call wrote
// (read), hist_* = this call's slot (written).
struct FgBuffers {
    const uint32_t* color;   // W * H
    const float* depth;      // w * h
    const float* mv;         // w * h * 3
    uint32_t* out;           // W * H
    const uint32_t* prev_color;
    const float* prev_z;
    uint32_t* hist_color;
    float* hist_z;
    unsigned long long* field;  // w * h
};

// field[i] = min(field[i], key): the vector global atomic on the device, a plain min on the host
PT_HD void fg_field_min(unsigned long long* p, unsigned long long key)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, key);
#else
    if (key < *p) *p = key;
#endif
}

// step 2's depth as the high word of the key: NaN, negative and infinite depths count as +inf, -0 as +0
PT_HD uint32_t fg_depth_bits(float z)
{
    if (!(z >= 0.0f) || !is_finite(z)) return 0x7F800000u;
    return z == 0.0f ? 0u : as_uint(z);
}

PT_HD unsigned long long fg_key(float z, uint32_t i) { return ((unsigned long long)fg_depth_bits(z) << 32) | i; }

// step 2, render pixel (x, y): up to four targets around q = p + mv / 2; each is tested against the image in float before it becomes an
// integer.  The lane also copies its depth into the history.
PT_HD void fg_scatter_pixel(const FgParams& P, const FgBuffers& b, int x, int y)
{
    const uint32_t i = (uint32_t)y * P.w + (uint32_t)x;
    const float z = b.depth[i];
    const float mx = b.mv[3 * (size_t)i], my = b.mv[3 * (size_t)i + 1];
    b.hist_z[i] = z;
    const float qx = (float)x + 0.5f * mx, qy = (float)y + 0.5f * my;
    if (!is_finite(qx) || !is_finite(qy)) return;
    const float x0 = pt_floor(qx), y0 = pt_floor(qy);
    const float fx = qx - x0, fy = qy - y0;
    const unsigned long long key = fg_key(z, i);
    const float fw = (float)P.w, fh = (float)P.h;
    for (int dy = 0; dy < 2; dy++) {
        if (dy == 1 && !(fy > 0.0f)) continue;
        const float ty = y0 + (float)dy;
        if (!(ty >= 0.0f && ty < fh)) continue;
        for (int dx = 0; dx < 2; dx++) {
            if (dx == 1 && !(fx > 0.0f)) continue;
            const float tx = x0 + (float)dx;
            if (!(tx >= 0.0f && tx < fw)) continue;
            fg_field_min(&b.field[(size_t)(int)ty * P.w + (size_t)(int)tx], key);
        }
    }
}

struct FgRGB { float r, g, b; };

// the three colour channels of a packed pixel as float(code), in pt_post.h's order (R in the low bits)
PT_HD FgRGB fg_decode(uint32_t p, uint32_t format)
{
    FgRGB c;
    if (format == kFgFormatRGB10A2) { c.r = (float)(p & 1023u); c.g = (float)((p >> 10) & 1023u); c.b = (float)((p >> 20) & 1023u); }
    else { c.r = (float)(p & 255u); c.g = (float)((p >> 8) & 255u); c.b = (float)((p >> 16) & 255u); }
    return c;
}

PT_HD bool fg_inside(float x, float y, float W, float H) { return x >= 0.0f && x < W && y >= 0.0f && y < H; }  // a NaN fails

// the four texels and two fractions of a bilinear sample at (px, py) - 0.5; (px, py) must lie inside [0, W) x [0, H)
struct FgTaps { size_t i00, i10, i01, i11; float fx, fy; };
PT_HD FgTaps fg_taps(float px, float py, uint32_t W, uint32_t H)
{
    const float x = px - 0.5f, y = py - 0.5f;
    const float xf = pt_floor(x), yf = pt_floor(y);
    const uint32_t x0 = clamp_index((int)xf, W), x1 = clamp_index((int)xf + 1, W);
    const uint32_t y0 = clamp_index((int)yf, H), y1 = clamp_index((int)yf + 1, H);
    FgTaps t;
    t.i00 = (size_t)y0 * W + x0; t.i10 = (size_t)y0 * W + x1;
    t.i01 = (size_t)y1 * W + x0; t.i11 = (size_t)y1 * W + x1;
    t.fx = x - xf; t.fy = y - yf;
    return t;
}

PT_HD FgRGB fg_bilinear(uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11, float fx, float fy, uint32_t format)
{
    const FgRGB a = fg_decode(p00, format), b = fg_decode(p10, format), c = fg_decode(p01, format), d = fg_decode(p11, format);
    FgRGB o;
    o.r = lerp1(lerp1(a.r, b.r, fx), lerp1(c.r, d.r, fx), fy);
    o.g = lerp1(lerp1(a.g, b.g, fx), lerp1(c.g, d.g, fx), fy);
    o.b = lerp1(lerp1(a.b, b.b, fx), lerp1(c.b, d.b, fx), fy);
    return o;
}

PT_HD int fg_render_index(float c, float r, uint32_t n)  // min(floor(c r), n - 1) for c r >= 0
{
    const int i = (int)pt_floor(c * r);
    return i >= (int)n ? (int)n - 1 : i;
}

// code = min(max(floor(v + 0.5), 0), M) per channel, under the alpha bits of `own`
PT_HD uint32_t fg_pack(FgRGB v, uint32_t own, uint32_t format)
{
    const float M = format == kFgFormatRGB10A2 ? 1023.0f : 255.0f;
    const uint32_t r = (uint32_t)pt_min(pt_max(pt_floor(v.r + 0.5f), 0.0f), M);
    const uint32_t g = (uint32_t)pt_min(pt_max(pt_floor(v.g + 0.5f), 0.0f), M);
    const uint32_t b = (uint32_t)pt_min(pt_max(pt_floor(v.b + 0.5f), 0.0f), M);
    if (format == kFgFormatRGB10A2) return r | (g << 10) | (b << 20) | (own & 0xC0000000u);
    return r | (g << 8) | (b << 16) | (own & 0xFF000000u);
}

// What step 3 decided for one output pixel, for the tests: the field entry, whether each side was valid, the unrounded colour
struct FgTrace {
    unsigned long long k;
    uint32_t valid_a, valid_b;
    FgRGB v;
};

// step 3, output pixel (ox, oy).  The loads come in three rounds, each issued whole before its first use: the field entry with the
// pixel's own and previous colour; the source record (vector + depth); the eight taps and the previous depth, whose addresses fall
// back to the pixel's own centre where a side is outside the image, so that they need no branch.
PT_HD uint32_t fg_gather_pixel(const FgParams& P, const FgBuffers& b, int ox, int oy, FgTrace* trace)
{
    const size_t o = (size_t)oy * P.W + ox;
    const float cx = (float)ox + 0.5f, cy = (float)oy + 0.5f;
    const unsigned long long k = b.field[(size_t)fg_render_index(cy, P.ry, P.h) * P.w + fg_render_index(cx, P.rx, P.w)];
    const uint32_t own = b.color[o], before = b.prev_color[o];
    b.hist_color[o] = own;
    if (trace) { trace->k = k; trace->valid_a = trace->valid_b = 0; trace->v = fg_decode(before, P.format); }
    if (k == kFgHole) return before;
    const uint32_t s = (uint32_t)k;
    const float mx = b.mv[3 * (size_t)s], my = b.mv[3 * (size_t)s + 1], mz = b.mv[3 * (size_t)s + 2];
    const float z = b.depth[s];
    const float hx = (0.5f * mx) * P.sx, hy = (0.5f * my) * P.sy;
    const float ax = cx - hx, ay = cy - hy, bx = cx + hx, by = cy + hy;
    const float fW = (float)P.W, fH = (float)P.H;
    const bool valid_a = fg_inside(ax, ay, fW, fH), in_b = fg_inside(bx, by, fW, fH);
    const FgTaps ta = fg_taps(valid_a ? ax : cx, valid_a ? ay : cy, P.W, P.H);
    const float sbx = in_b ? bx : cx, sby = in_b ? by : cy;
    const FgTaps tb = fg_taps(sbx, sby, P.W, P.H);
    const uint32_t a00 = b.color[ta.i00], a10 = b.color[ta.i10], a01 = b.color[ta.i01], a11 = b.color[ta.i11];
    const uint32_t b00 = b.prev_color[tb.i00], b10 = b.prev_color[tb.i10], b01 = b.prev_color[tb.i01], b11 = b.prev_color[tb.i11];
    const float zp = b.prev_z[(size_t)fg_render_index(sby, P.ry, P.h) * P.w + fg_render_index(sbx, P.rx, P.w)];
    const float e = z + mz;
    const bool depth_ok = (!is_finite(zp) && !is_finite(z)) || (is_finite(zp) && is_finite(e) && pt_abs(zp - e) <= kFgDepthRel * e);
    const bool valid_b = in_b && depth_ok;
    const FgRGB ca = fg_bilinear(a00, a10, a01, a11, ta.fx, ta.fy, P.format);
    const FgRGB cb = fg_bilinear(b00, b10, b01, b11, tb.fx, tb.fy, P.format);
    FgRGB v;
    if (valid_a && valid_b) { v.r = 0.5f * (ca.r + cb.r); v.g = 0.5f * (ca.g + cb.g); v.b = 0.5f * (ca.b + cb.b); }
    else if (valid_a) v = ca;
    else if (valid_b) v = cb;
    else v = fg_decode(own, P.format);
    if (trace) { trace->valid_a = valid_a; trace->valid_b = valid_b; trace->v = v; }
    return fg_pack(v, own, P.format);
}

#if defined(__HIPCC__)
// pt_framegen.hip: the scatter and gather launches of one generated frame on `stream` (the field must already be cleared there)
hipError_t launch_framegen(const FgBuffers& b, const FgParams& P, hipStream_t stream);
#endif

}  // namespace pt
