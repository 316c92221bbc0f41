// pt_rr.h -- the ray-reconstruction stand-in (row N15): a denoising temporal upscaler that reads and writes the resources the
// reference tags for DLSS-RR (App::ProcessDLSSRayReconstruction, Source/App.cpp:1654-1671): the noisy radiance, depth, motion vectors,
// NormalRoughness, both albedos and SpecularHitDistance at RenderSize in, the colour at output size out, a history in between
// (DESIGN.md spec S21).  Per-pixel functions for the two kernels of pt_rr.hip; they also compile as host C++
// (tests/hostshim/rr_host.cpp), so the GPU output is pinned bit for bit to the host-compiled header.  fp32 throughout, no contraction
// (-ffp-contract=off); pt_fma only where the spec says fma (the projections, the kernel mix, the history mix and the blend).
// A pixel whose nearest input pixel is a miss runs up_pixel of pt_upscale.h (spec S17) on the same tile.
#pragma once

#include "pt_upscale.h"

namespace pt {

constexpr float kRrAlbedoMin = 0.0009765625f;    // step 1: 2^-10, the floor of the demodulation's divisor
constexpr float kRrVirtualRoughness = 2.5f;      // step 1: f(r) = max(0, 1 - 2.5 r): the virtual motion fades out at roughness 0.4
constexpr float kRrDepthEdge = 0.05f;            // step 3: a tap's weight falls to 0 at |z_k - z| = 0.05 z
constexpr float kRrDepthEdgeMin = 1e-30f;
constexpr float kRrNormalEdge = 0.8f;            // ... at N_k . N = 0.8, linearly from 1 at N_k . N = 1
constexpr float kRrNormalScale = 5.0f;           // 1 / (1 - 0.8)
constexpr float kRrRoughnessEdge = 4.0f;         // ... at |r_k - r| = 0.25
constexpr float kRrWideInvR2 = 0.1111111111f;    // step 3: the wide kernel (1 - d^2 / 9)^2 per axis
constexpr float kRrLongHistory = 0.25f;          // step 3: the kernel is all narrow from a history weight of 4 up
constexpr float kRrClipSigma = 1.5f;             // step 5: the history is clipped to mean +- 1.5 sigma of the taps
constexpr float kRrHistoryNormal = 0.8f;         // step 2: a history corner needs N_prev . N >= 0.8
constexpr float kRrHistoryWeightMin = 0.015625f; // step 2: accepted bilinear weight at or below 1/64: no history

// The tile of a 32 x 8 workgroup of pt_rr.hip: the lanes' nearest input pixels span at most 32 x 8 (the argument above kUpTileW), two
// taps either side make 36 x 12.  tests/test_ray_reconstruction.py checks rr_footprint_extent against this bound.
constexpr int kRrTileW = 36, kRrTileH = 12;

struct RrParams {
    UpParams up;            // sizes, Jitter, ratios and MaxHistoryWeight as pt_upscale holds them
    float inv_w, inv_h;     // 1 / RenderSize
    f3 position;            // PtRayReconstructionSettings.Position
    float proj_to_view[16], view_to_world[16], prev_world_to_proj[16];
};

PT_HD RrParams rr_params(uint32_t w, uint32_t h, uint32_t W, uint32_t H, float jx, float jy, float max_a, const float* position,
                         const float* proj_to_view, const float* view_to_world, const float* prev_world_to_proj)
{
    RrParams R;
    R.up = up_params(w, h, W, H, jx, jy, max_a);
    R.inv_w = 1.0f / (float)w;
    R.inv_h = 1.0f / (float)h;
    R.position = make_f3(position[0], position[1], position[2]);
    for (int i = 0; i < 16; i++) {
        R.proj_to_view[i] = proj_to_view[i];
        R.view_to_world[i] = view_to_world[i];
        R.prev_world_to_proj[i] = prev_world_to_proj[i];
    }
    return R;
}

// What the prepare pass leaves per render pixel (the context's work buffers), and what the resolve pass stages of it
struct RrRecord {
    float4 tz;    // demodulated t-space colour, depth (+inf = a miss)
    float4 nr;    // sanitised normal, roughness (0 for a miss)
    float4 virt;  // the virtual motion (x, y) in input pixels, its weight, 0
};

struct RrTile {
    const float4 *tz, *nr;
    const float *vx, *vy, *vz;  // MotionVector as three planes
    int x0, y0, stride;
};

// The buffers of one call: the caller's, the prepare pass's records (w * h each) and the two history slots (W * H each).
struct RrBuffers {
    const float4* color;            // w * h
    const float* depth;             // w * h
    const float* motion;            // w * h * 3
    const float4* normal_roughness; // w * h
    const float* diffuse_albedo;    // w * h * 3
    const float* specular_albedo;   // w * h * 3
    const float* hit_distance;      // w * h
    float4* out;                    // W * H
    float4 *rec_tz, *rec_nr, *rec_virt;
    const float4 *prev_hist, *prev_n;
    const float* prev_z;
    float4 *hist, *hist_n;          // (t-space demodulated colour, weight A), (normal, roughness)
    float* hist_z;
};

PT_HD float rr_unit(float v) { return !(v == v) ? 0.0f : pt_min(pt_max(v, -1.0f), 1.0f); }

// [p, 1] . M with M's 16 floats as DirectXMath rows (Geometry::ProjectiveTransform)
PT_HD float4 rr_project(const float* m, f3 p)
{
    return up_f4(pt_fma(p.z, m[8], pt_fma(p.y, m[4], pt_fma(p.x, m[0], m[12]))), pt_fma(p.z, m[9], pt_fma(p.y, m[5], pt_fma(p.x, m[1], m[13]))),
                 pt_fma(p.z, m[10], pt_fma(p.y, m[6], pt_fma(p.x, m[2], m[14]))), pt_fma(p.z, m[11], pt_fma(p.y, m[7], pt_fma(p.x, m[3], m[15]))));
}

// the albedo the colour is divided by and the output multiplied with: sanitised DiffuseAlbedo + SpecularAlbedo
PT_HD f3 rr_albedo(const float* da, const float* sa, size_t i)
{
    return make_f3(up_sanitize(da[3 * i] + sa[3 * i]), up_sanitize(da[3 * i + 1] + sa[3 * i + 1]), up_sanitize(da[3 * i + 2] + sa[3 * i + 2]));
}

// Camera::ReconstructWorldPosition (Shaders/Camera.hlsli:56-63), restated: the view-space point of NDC at depth 0.5 scaled so that its
// z is the linear depth, through ViewToWorld
PT_HD f3 rr_world_position(const RrParams& R, float ndc_x, float ndc_y, float z)
{
    const float4 p = rr_project(R.proj_to_view, make_f3(ndc_x, ndc_y, 0.5f));
    const f3 v = make_f3((p.x / p.z) * z, (p.y / p.z) * z, z);
    const float4 X = rr_project(R.view_to_world, v);
    return make_f3(X.x, X.y, X.z);
}

// step 1, once per render pixel (x, y)
PT_HD RrRecord rr_prepare_px(const RrParams& R, const RrBuffers& b, int x, int y)
{
    const UpParams& P = R.up;
    const size_t i = (size_t)y * P.w + x;
    const float4 c = b.color[i];
    const float depth = b.depth[i];
    const bool surface = is_finite(depth) && depth > 0.0f;
    float r = up_sanitize(c.x), g = up_sanitize(c.y), bl = up_sanitize(c.z);
    RrRecord rec;
    rec.nr = up_f4(0.0f, 0.0f, 0.0f, 0.0f);
    const float mx = b.motion[3 * i], my = b.motion[3 * i + 1];
    rec.virt = up_f4(mx, my, 0.0f, 0.0f);
    if (surface) {
        const f3 A = rr_albedo(b.diffuse_albedo, b.specular_albedo, i);
        r = pt_min(r / pt_max(A.x, kRrAlbedoMin), kUpMaxRadiance);
        g = pt_min(g / pt_max(A.y, kRrAlbedoMin), kUpMaxRadiance);
        bl = pt_min(bl / pt_max(A.z, kRrAlbedoMin), kUpMaxRadiance);
        const float4 n = b.normal_roughness[i];
        rec.nr = up_f4(rr_unit(n.x), rr_unit(n.y), rr_unit(n.z), saturate(n.w));
        const float hit = b.hit_distance[i];
        if (is_finite(hit) && hit > 0.0f) {
            const float f = pt_max(0.0f, 1.0f - rec.nr.w * kRrVirtualRoughness);
            const float u = (((float)x + 0.5f) - P.jx) * R.inv_w, v = (((float)y + 0.5f) - P.jy) * R.inv_h;
            const f3 X = rr_world_position(R, pt_fma(u, 2.0f, -1.0f), pt_fma(v, -2.0f, 1.0f), depth);
            const f3 V = normalize(X - R.position);
            const float4 clip = rr_project(R.prev_world_to_proj, mad(hit * f, V, X));
            if (clip.w > 0.0f) {
                const float up = pt_fma(clip.x / clip.w, 0.5f, 0.5f), vp = pt_fma(clip.y / clip.w, -0.5f, 0.5f);
                const float ld = luminance(make_f3(up_sanitize(b.diffuse_albedo[3 * i]), up_sanitize(b.diffuse_albedo[3 * i + 1]), up_sanitize(b.diffuse_albedo[3 * i + 2])));
                const float ls = luminance(make_f3(up_sanitize(b.specular_albedo[3 * i]), up_sanitize(b.specular_albedo[3 * i + 1]), up_sanitize(b.specular_albedo[3 * i + 2])));
                const float share = ld + ls > 0.0f ? ls / (ld + ls) : 0.0f;
                rec.virt = up_f4((up - u) * (float)P.w, (vp - v) * (float)P.h, share * f, 0.0f);
            }
        }
    }
    const float d = 1.0f + up_max3(r, g, bl);
    rec.tz = up_f4(r / d, g / d, bl / d, surface ? depth : kInf);
    return rec;
}

PT_HD int rr_tile_origin(int nearest) { return nearest - 2 < 0 ? 0 : nearest - 2; }

// The input footprint of the workgroup whose first output pixel is (X0, Y0), as up_footprint_extent with two taps either side;
// rr_footprint, what the kernel stages, also bounds it by the tile so that no staging loop can leave the LDS arrays.
PT_HD UpFootprint rr_footprint_extent(const UpParams& P, int X0, int Y0)
{
    const int X1 = (X0 + kUpBlockW < (int)P.W ? X0 + kUpBlockW : (int)P.W) - 1, Y1 = (Y0 + kUpBlockH < (int)P.H ? Y0 + kUpBlockH : (int)P.H) - 1;
    const int bx = up_nearest((float)X1 + 0.5f, P.rx, P.w) + 2, by = up_nearest((float)Y1 + 0.5f, P.ry, P.h) + 2;
    UpFootprint f;
    f.x0 = rr_tile_origin(up_nearest((float)X0 + 0.5f, P.rx, P.w));
    f.y0 = rr_tile_origin(up_nearest((float)Y0 + 0.5f, P.ry, P.h));
    const int x1 = bx > (int)P.w - 1 ? (int)P.w - 1 : bx, y1 = by > (int)P.h - 1 ? (int)P.h - 1 : by;
    f.fw = x1 - f.x0 + 1;
    f.fh = y1 - f.y0 + 1;
    return f;
}

PT_HD UpFootprint rr_footprint(const UpParams& P, int X0, int Y0)
{
    UpFootprint f = rr_footprint_extent(P, X0, Y0);
    f.fw = f.fw < kRrTileW ? f.fw : kRrTileW;
    f.fh = f.fh < kRrTileH ? f.fh : kRrTileH;
    return f;
}

// step 2: the history at output position (qx, qy), bilinear over the corners that pass the previous-depth test of S17 (against the
// expected depth ze) and the previous-normal test; (colour, weight), weight 0 = none
PT_HD float4 rr_history_tap(const UpParams& P, const RrBuffers& b, float qx, float qy, float ze, float4 n)
{
    const float4 none = up_f4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(qx >= 0.0f && qy >= 0.0f && qx < (float)P.W && qy < (float)P.H)) return none;
    const float x = qx - 0.5f, y = qy - 0.5f;
    const float xf = pt_floor(x), yf = pt_floor(y);
    const float fx = x - xf, fy = y - yf;
    const uint32_t xs[2] = { clamp_index((int)xf, P.W), clamp_index((int)xf + 1, P.W) };
    const uint32_t ys[2] = { clamp_index((int)yf, P.H), clamp_index((int)yf + 1, P.H) };
    const float wx[2] = { 1.0f - fx, fx }, wy[2] = { 1.0f - fy, fy };
    float sw = 0.0f;
    float4 acc = none;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            const size_t k = (size_t)ys[j] * P.W + xs[i];
            const float zp = b.prev_z[k];
            const float4 np = b.prev_n[k];
            if (!(is_finite(zp) && pt_abs(zp - ze) <= kUpDepthRel * ze)) continue;
            if (!(dot(make_f3(np.x, np.y, np.z), make_f3(n.x, n.y, n.z)) >= kRrHistoryNormal)) continue;
            const float4 hk = b.prev_hist[k];
            const float wk = wx[i] * wy[j];
            sw = sw + wk;
            acc = up_f4(acc.x + hk.x * wk, acc.y + hk.y * wk, acc.z + hk.z * wk, acc.w + hk.w * wk);
        }
    if (!(sw > kRrHistoryWeightMin)) return none;
    const float inv = 1.0f / sw;
    const float4 r = up_f4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    return r.w > 0.0f ? r : none;
}

// Output pixel (ox, oy): steps 2-6 of spec S21.  kRestart: no history is read (the first call, Reset, a size change).
template <bool kRestart>
PT_HD void rr_pixel(const RrParams& R, const RrTile& T, const RrBuffers& b, int ox, int oy)
{
    const UpParams& P = R.up;
    const float cx = (float)ox + 0.5f, cy = (float)oy + 0.5f;
    const float px = cx * P.rx, py = cy * P.ry;
    const int nx = up_nearest(cx, P.rx, P.w), ny = up_nearest(cy, P.ry, P.h);
    const int ci = (ny - T.y0) * T.stride + (nx - T.x0);
    const float4 c0 = T.tz[ci];
    const size_t o = (size_t)oy * P.W + ox;
    if (!is_finite(c0.w)) {
        // a miss: spec S17 unchanged, on the same tile and the same history planes
        UpTile U;
        U.tz = T.tz; U.vx = T.vx; U.vy = T.vy; U.vz = T.vz;
        U.x0 = T.x0; U.y0 = T.y0; U.stride = T.stride;
        UpBuffers ub;
        ub.color = b.color; ub.depth = b.depth; ub.velocity = b.motion; ub.out = b.out;
        ub.prev_hist = b.prev_hist; ub.prev_z = b.prev_z; ub.hist = b.hist; ub.hist_z = b.hist_z;
        up_pixel<kRestart>(P, U, ub, ox, oy);
        b.hist_n[o] = up_f4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 n0 = T.nr[ci];
    const f3 N = make_f3(n0.x, n0.y, n0.z);
    const float zc = c0.w;
    // step 2: the history at the surface motion, and at the virtual motion where the prepare pass left one
    float ap = 0.0f;
    f3 hc = make_f3(0.0f, 0.0f, 0.0f);
    if (!kRestart) {
        const float ze = zc + T.vz[ci];
        float4 hs = rr_history_tap(P, b, cx + T.vx[ci] * P.sx, cy + T.vy[ci] * P.sy, ze, n0);
        const float4 vm = b.rec_virt[(size_t)ny * P.w + nx];
        if (vm.z > 0.0f) {
            const float4 hv = rr_history_tap(P, b, cx + vm.x * P.sx, cy + vm.y * P.sy, ze, n0);
            if (hv.w > 0.0f) {
                if (hs.w > 0.0f) hs = up_f4(pt_fma(vm.z, hv.x - hs.x, hs.x), pt_fma(vm.z, hv.y - hs.y, hs.y), pt_fma(vm.z, hv.z - hs.z, hs.z), pt_fma(vm.z, hv.w - hs.w, hs.w));
                else hs = up_f4(hv.x, hv.y, hv.z, vm.z * hv.w);
            }
        }
        ap = hs.w;
        hc = make_f3(hs.x, hs.y, hs.z);
    }
    // step 3: the 5 x 5 taps inside the image, row by row
    const float narrow = pt_min(ap * kRrLongHistory, 1.0f);
    const float iz = 1.0f / pt_max(kRrDepthEdge * zc, kRrDepthEdgeMin);
    float sw = 0.0f, sww = 0.0f, cov = 0.0f;
    f3 m1 = make_f3(0.0f, 0.0f, 0.0f), m1w = m1, m2w = m1;
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            const int ix = nx + dx, iy = ny + dy;
            if (ix < 0 || iy < 0 || ix >= (int)P.w || iy >= (int)P.h) continue;
            const int ti = (iy - T.y0) * T.stride + (ix - T.x0);
            const float4 tz = T.tz[ti];
            if (!is_finite(tz.w)) continue;
            const float4 nr = T.nr[ti];
            const f3 t = make_f3(tz.x - c0.x, tz.y - c0.y, tz.z - c0.z);  // moments about the centre's colour: no cancellation on flat ground
            const float ddx = (((float)ix + 0.5f) - P.jx) - px, ddy = (((float)iy + 0.5f) - P.jy) - py;
            const float x2 = ddx * ddx, y2 = ddy * ddy;
            const float gx = pt_max(0.0f, 1.0f - x2 * kRrWideInvR2), gy = pt_max(0.0f, 1.0f - y2 * kRrWideInvR2);
            const float wide = (gx * gx) * (gy * gy);
            float ks;
            if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) {
                ks = pt_fma(narrow, pt_max(0.0f, up_lanczos(x2)) * pt_max(0.0f, up_lanczos(y2)) - wide, wide);
                cov = pt_max(cov, pt_max(0.0f, 1.0f - pt_abs(ddx) * P.sx) * pt_max(0.0f, 1.0f - pt_abs(ddy) * P.sy));
            } else {
                ks = pt_fma(narrow, -wide, wide);
            }
            const float wz = pt_max(0.0f, 1.0f - pt_abs(tz.w - zc) * iz);
            const float wn = saturate((dot(make_f3(nr.x, nr.y, nr.z), N) - kRrNormalEdge) * kRrNormalScale);
            const float wr = pt_max(0.0f, 1.0f - pt_abs(nr.w - n0.w) * kRrRoughnessEdge);
            const float edge = (wz * wn) * wr;
            const float wt = ks * edge, ww = wide * edge;
            sw = sw + wt;
            m1 = m1 + t * wt;
            sww = sww + ww;
            m1w = m1w + t * ww;
            m2w = m2w + (t * t) * ww;
        }
    // step 4: the resampled colour u (the mixed kernel) and the taps' mean and deviation (the wide kernel, whatever the history's
    // length), a division each per lane
    const f3 t0 = make_f3(c0.x, c0.y, c0.z);
    f3 u = t0, mean = t0, sg = make_f3(0.0f, 0.0f, 0.0f);
    if (sw > kUpWeightMin) u = t0 + m1 * (1.0f / sw);
    if (sww > kUpWeightMin) {
        const float inv = 1.0f / sww;
        const f3 e = m1w * inv;
        mean = t0 + e;
        const f3 q = m2w * inv - e * e;
        sg = make_f3(pt_sqrt(pt_max(q.x, 0.0f)), pt_sqrt(pt_max(q.y, 0.0f)), pt_sqrt(pt_max(q.z, 0.0f)));
    }
    const float kappa = up_clamp(cov, kUpCoverageMin, 1.0f);
    f3 t_out = u;
    float a_out = kappa;
    if (!kRestart && ap > 0.0f) {
        // steps 5-6: the clip and the blend
        const f3 lo = mean - sg * kRrClipSigma, hi = mean + sg * kRrClipSigma;
        hc = make_f3(up_clamp(hc.x, lo.x, hi.x), up_clamp(hc.y, lo.y, hi.y), up_clamp(hc.z, lo.z, hi.z));
        const float alpha = kappa / (kappa + ap);
        t_out = make_f3(pt_fma(u.x - hc.x, alpha, hc.x), pt_fma(u.y - hc.y, alpha, hc.y), pt_fma(u.z - hc.z, alpha, hc.z));
        a_out = pt_min(ap + kappa, P.max_a);
    }
    b.hist[o] = up_f4(t_out.x, t_out.y, t_out.z, a_out);
    b.hist_z[o] = zc;
    b.hist_n[o] = n0;
    const size_t ni = (size_t)ny * P.w + nx;
    const f3 c = up_inverse(t_out) * rr_albedo(b.diffuse_albedo, b.specular_albedo, ni);
    b.out[o] = up_f4(c.x, c.y, c.z, b.color[ni].w);
}

#if defined(__HIPCC__)
// pt_rr.hip: the two launches on `stream`
hipError_t launch_ray_reconstruction(const RrBuffers& b, const RrParams& R, bool restart, hipStream_t stream);
#endif

}  // namespace pt
