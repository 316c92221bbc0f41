// pt_upscale.h -- the super-resolution stand-in (row N11): a temporal upscaler of the TAAU / FSR2 family that reads and writes the
// resources the reference tags for XeSS (App::ProcessXeSSSuperResolution, Source/App.cpp:1682-1708): the jittered radiance, depth and
// motion vectors at RenderSize in, the frame at output size out, an accumulated history in between (DESIGN.md spec S17).
// Per-pixel functions for the kernel of pt_upscale.hip; they also compile as host C++ (tests/hostshim/upscale_host.cpp), so the GPU
// output is pinned bit for bit to the host-compiled header.  fp32 throughout, no contraction (-ffp-contract=off); pt_fma only where
// the spec says fma (the bilinear history tap and the blend).
#pragma once

#include "pt_texture.h"

namespace pt {

constexpr uint32_t kUpMaxSize = 16384, kUpMaxRatio = 4;
constexpr float kUpMaxRadiance = 65504.0f;      // step 1: the largest half float, what the reference's R16G16B16A16_FLOAT radiance holds
constexpr float kUpDefaultHistoryWeight = 16.0f, kUpMinHistoryWeight = 1.0f, kUpMaxHistoryWeight = 256.0f;
constexpr float kUpWeightMin = 0.0009765625f;   // 2^-10: a tap-weight sum at or below this falls back to the nearest input pixel
constexpr float kUpCoverageMin = 0.0625f;       // 1/16
constexpr float kUpDepthRel = 0.1f;             // history: |z_prev - (z + mv.z)| <= 0.1 (z + mv.z)
// the modes of pt_upscale_input_size: SuperResolutionMode (Source/MyAppData.h) in the reference's order
constexpr uint32_t kUpModeAuto = 0, kUpModeNative = 1, kUpModeUltraPerformance = 5;

// The tile of a 32 x 8 workgroup of pt_upscale.hip: 34 x 10 input pixels hold every tap of its lanes.  Along x (y alike, with 7 for 31):
// the lanes' centres c = X + 0.5 are exact in fp32 and at most 31 apart; r = fl(w / W) <= 1.  With r = 1 the products c r are exact and
// 31 apart.  Otherwise w <= W - 1, so r <= 1 - 2^-14 (W <= 16384) and 31 r <= 31 - 31 * 2^-14; each product is below 16384 and rounds by
// at most 2^-11, so fl(c1 r) - fl(c0 r) <= 31 - 31 * 2^-14 + 2^-10 < 31.  Either way floor(fl(c1 r)) - floor(fl(c0 r)) <= 31, and the
// clamp into the image does not widen it: the lanes' nearest input pixels span at most 32 columns, a tap either side makes 34.
// tests/test_upscale.py checks up_footprint_extent against this bound over a sweep of size pairs.
constexpr int kUpTileW = 34, kUpTileH = 10;

struct UpParams {
    uint32_t w, h, W, H;   // input and output size
    float jx, jy;          // PtUpscaleSettings.Jitter: input pixel i is a sample at i + 0.5 - Jitter
    float rx, ry;          // w / W, h / H
    float sx, sy;          // W / w, H / h
    float max_a;           // MaxHistoryWeight (0 already replaced by 16)
};

PT_HD UpParams up_params(uint32_t w, uint32_t h, uint32_t W, uint32_t H, float jx, float jy, float max_a)
{
    UpParams P;
    P.w = w; P.h = h; P.W = W; P.H = H;
    P.jx = jx; P.jy = jy;
    P.rx = (float)w / (float)W; P.ry = (float)h / (float)H;
    P.sx = (float)W / (float)w; P.sy = (float)H / (float)h;
    P.max_a = max_a;
    return P;
}

// The staged input the taps are read from: sanitised t-space colour with the depth in .w, and the velocity as three planes, over the
// input pixels [x0, x0 + ...) x [y0, y0 + ...) with `stride` texels per row.  The kernel's is its workgroup's footprint in LDS, the
// host shim's the whole image.
struct UpTile {
    const float4* tz;
    const float *vx, *vy, *vz;
    int x0, y0, stride;
};

// The buffers of one call: the caller's (PtUpscaleTextures) and the context's history, W * H texels each.  prev_* = the slot the
// previous call wrote (read), hist / hist_z = this call's slot (written).
struct UpBuffers {
    const float4* color;   // w * h
    const float* depth;    // w * h
    const float* velocity; // w * h * 3
    float4* out;           // W * H
    const float4* prev_hist;
    const float* prev_z;
    float4* hist;          // (t-space colour, accumulated weight A)
    float* hist_z;
};

PT_HD float4 up_f4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
PT_HD float up_max3(float a, float b, float c) { return pt_max(pt_max(a, b), c); }
// step 1: NaN -> 0, else min(max(c, 0), 65504)
PT_HD float up_sanitize(float c) { return !(c == c) ? 0.0f : pt_min(pt_max(c, 0.0f), kUpMaxRadiance); }

// step 1, once per input pixel: (t(c'), depth) with t(c) = c / (1 + max3(c))
PT_HD float4 up_stage_px(float4 c, float depth)
{
    const float r = up_sanitize(c.x), g = up_sanitize(c.y), b = up_sanitize(c.z);
    const float d = 1.0f + up_max3(r, g, b);
    return up_f4(r / d, g / d, b / d, depth);
}

// the inverse: c = t / (1 - max3(t))
PT_HD f3 up_inverse(f3 t)
{
    const float d = 1.0f - up_max3(t.x, t.y, t.z);
    return make_f3(t.x / d, t.y / d, t.z / d);
}

// FSR2's Lanczos-2 polynomial in x^2: (25/16 (2/5 x^2 - 1)^2 - 9/16) (x^2/4 - 1)^2 below 4, else 0
PT_HD float up_lanczos(float x2)
{
    if (!(x2 < 4.0f)) return 0.0f;
    const float a = 0.4f * x2 - 1.0f, b = 0.25f * x2 - 1.0f;
    return (1.5625f * (a * a) - 0.5625f) * (b * b);
}

// step 2: the input pixel that holds output pixel centre c (= o + 0.5) on one axis, clamped into the image
PT_HD int up_nearest(float c, float r, uint32_t n)
{
    const int i = (int)pt_floor(c * r);
    return i < 0 ? 0 : (i >= (int)n ? (int)n - 1 : i);
}

// The input footprint [x0, x0 + fw) x [y0, y0 + fh) of the workgroup whose first output pixel is (X0, Y0): up_nearest is monotonic in the
// output coordinate, so every lane's 3 x 3 taps lie between those of the block's corners.  up_footprint_extent is the footprint as the
// taps need it; fw <= kUpTileW and fh <= kUpTileH by the argument above, which the tests check on this function.  up_footprint, what
// the kernel stages, also bounds it by the tile so that no staging loop can leave the LDS arrays.
constexpr int kUpBlockW = 32, kUpBlockH = 8;
struct UpFootprint { int x0, y0, fw, fh; };
PT_HD UpFootprint up_footprint_extent(const UpParams& P, int X0, int Y0)
{
    const int X1 = (X0 + kUpBlockW < (int)P.W ? X0 + kUpBlockW : (int)P.W) - 1, Y1 = (Y0 + kUpBlockH < (int)P.H ? Y0 + kUpBlockH : (int)P.H) - 1;
    const int ax = up_nearest((float)X0 + 0.5f, P.rx, P.w) - 1, bx = up_nearest((float)X1 + 0.5f, P.rx, P.w) + 1;
    const int ay = up_nearest((float)Y0 + 0.5f, P.ry, P.h) - 1, by = up_nearest((float)Y1 + 0.5f, P.ry, P.h) + 1;
    UpFootprint f;
    f.x0 = ax < 0 ? 0 : ax;
    f.y0 = ay < 0 ? 0 : ay;
    const int x1 = bx > (int)P.w - 1 ? (int)P.w - 1 : bx, y1 = by > (int)P.h - 1 ? (int)P.h - 1 : by;
    f.fw = x1 - f.x0 + 1;
    f.fh = y1 - f.y0 + 1;
    return f;
}

PT_HD UpFootprint up_footprint(const UpParams& P, int X0, int Y0)
{
    UpFootprint f = up_footprint_extent(P, X0, Y0);
    f.fw = f.fw < kUpTileW ? f.fw : kUpTileW;
    f.fh = f.fh < kUpTileH ? f.fh : kUpTileH;
    return f;
}

PT_HD float up_clamp(float x, float lo, float hi) { return pt_min(pt_max(x, lo), hi); }

// Output pixel (ox, oy): steps 2-6 of spec S17.  kRestart: no history is read (the first call, Reset, a size change).
template <bool kRestart>
PT_HD void up_pixel(const UpParams& P, const UpTile& T, const UpBuffers& b, int ox, int oy)
{
    const float cx = (float)ox + 0.5f, cy = (float)oy + 0.5f;
    const float px = cx * P.rx, py = cy * P.ry;
    const int nx = up_nearest(cx, P.rx, P.w), ny = up_nearest(cy, P.ry, P.h);
    // step 3 and the search of step 4 over the 3 x 3 taps inside the image, row by row
    bool any = false;
    float sw = 0.0f, cov = 0.0f, z = 0.0f;
    f3 acc = make_f3(0.0f, 0.0f, 0.0f), lo = acc, hi = acc;
    int bx = nx, by = ny;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int ix = nx + dx, iy = ny + dy;
            if (ix < 0 || iy < 0 || ix >= (int)P.w || iy >= (int)P.h) continue;
            const float4 tz = T.tz[(iy - T.y0) * T.stride + (ix - T.x0)];
            const f3 t = make_f3(tz.x, tz.y, tz.z);
            const float ddx = (((float)ix + 0.5f) - P.jx) - px, ddy = (((float)iy + 0.5f) - P.jy) - py;
            const float wt = up_lanczos(ddx * ddx) * up_lanczos(ddy * ddy);
            sw = sw + wt;
            acc = acc + t * wt;
            const float k = pt_max(0.0f, 1.0f - pt_abs(ddx) * P.sx) * pt_max(0.0f, 1.0f - pt_abs(ddy) * P.sy);
            if (!any) {
                lo = t; hi = t; cov = k; z = tz.w; bx = ix; by = iy;
                any = true;
            } else {
                lo = make_f3(pt_min(lo.x, t.x), pt_min(lo.y, t.y), pt_min(lo.z, t.z));
                hi = make_f3(pt_max(hi.x, t.x), pt_max(hi.y, t.y), pt_max(hi.z, t.z));
                cov = pt_max(cov, k);
                if (tz.w < z) { z = tz.w; bx = ix; by = iy; }
            }
        }
    const float4 tn = T.tz[(ny - T.y0) * T.stride + (nx - T.x0)];
    f3 u = sw <= kUpWeightMin ? make_f3(tn.x, tn.y, tn.z) : make_f3(acc.x / sw, acc.y / sw, acc.z / sw);
    u = make_f3(up_clamp(u.x, lo.x, hi.x), up_clamp(u.y, lo.y, hi.y), up_clamp(u.z, lo.z, hi.z));
    const float kappa = up_clamp(cov, kUpCoverageMin, 1.0f);
    f3 t_out = u;
    float a_out = kappa;
    if (!kRestart) {
        // steps 4-6: the dilated motion vector, the history tap and the blend
        const int vi = (by - T.y0) * T.stride + (bx - T.x0);
        const float mx = T.vx[vi], my = T.vy[vi], mz = T.vz[vi];
        const float qx = cx + mx * P.sx, qy = cy + my * P.sy;
        if (qx >= 0.0f && qy >= 0.0f && qx < (float)P.W && qy < (float)P.H) {
            const float zp = b.prev_z[(size_t)(int)pt_floor(qy) * P.W + (int)pt_floor(qx)];
            const float ze = z + mz;
            const bool fin = is_finite(z), finp = is_finite(zp);
            if ((!fin && !finp) || (fin && finp && pt_abs(zp - ze) <= kUpDepthRel * ze)) {
                const float x = qx - 0.5f, y = qy - 0.5f;
                const float xf = pt_floor(x), yf = pt_floor(y);
                const float fx = x - xf, fy = y - yf;
                const uint32_t x0 = clamp_index((int)xf, P.W), x1 = clamp_index((int)xf + 1, P.W);
                const uint32_t y0 = clamp_index((int)yf, P.H), y1 = clamp_index((int)yf + 1, P.H);
                const float4 c00 = b.prev_hist[(size_t)y0 * P.W + x0], c10 = b.prev_hist[(size_t)y0 * P.W + x1];
                const float4 c01 = b.prev_hist[(size_t)y1 * P.W + x0], c11 = b.prev_hist[(size_t)y1 * P.W + x1];
                const float ap = lerp1(lerp1(c00.w, c10.w, fx), lerp1(c01.w, c11.w, fx), fy);
                if (ap > 0.0f) {
                    f3 hc = make_f3(lerp1(lerp1(c00.x, c10.x, fx), lerp1(c01.x, c11.x, fx), fy),
                                    lerp1(lerp1(c00.y, c10.y, fx), lerp1(c01.y, c11.y, fx), fy),
                                    lerp1(lerp1(c00.z, c10.z, fx), lerp1(c01.z, c11.z, fx), fy));
                    hc = make_f3(up_clamp(hc.x, lo.x, hi.x), up_clamp(hc.y, lo.y, hi.y), up_clamp(hc.z, lo.z, hi.z));
                    const float alpha = kappa / (kappa + ap);
                    t_out = make_f3(pt_fma(u.x - hc.x, alpha, hc.x), pt_fma(u.y - hc.y, alpha, hc.y), pt_fma(u.z - hc.z, alpha, hc.z));
                    a_out = pt_min(ap + kappa, P.max_a);
                }
            }
        }
    }
    const size_t o = (size_t)oy * P.W + ox;
    b.hist[o] = up_f4(t_out.x, t_out.y, t_out.z, a_out);
    b.hist_z[o] = z;
    const f3 c = up_inverse(t_out);
    b.out[o] = up_f4(c.x, c.y, c.z, b.color[(size_t)ny * P.w + nx].w);
}

// pt_upscale_input_size: xessGetInputResolution's ratios (x 10) by mode 1..5, and the reference's Auto rule (App.cpp:1381-1394)
PT_HD uint32_t up_ratio10(uint32_t mode)
{
    return mode == 1 ? 10u : (mode == 2 ? 15u : (mode == 3 ? 17u : (mode == 4 ? 20u : 30u)));
}

PT_HD uint32_t up_auto_mode(uint32_t out_w, uint32_t out_h)
{
    const uint64_t n = (uint64_t)out_w * out_h;
    if (n <= 1280u * 800u) return 1;
    if (n <= 1920u * 1200u) return 2;
    if (n <= 2560u * 1600u) return 3;
    if (n <= 3840u * 2400u) return 4;
    return 5;
}

PT_HD uint32_t up_input_extent(uint32_t out, uint32_t r10)
{
    const uint64_t v = ((uint64_t)out * 10u + r10 / 2u) / r10;
    return v ? (uint32_t)v : 1u;
}

#if defined(__HIPCC__)
// pt_upscale.hip: one launch on `stream`
hipError_t launch_upscale(const UpBuffers& b, const UpParams& P, bool restart, hipStream_t stream);
#endif

}  // namespace pt
