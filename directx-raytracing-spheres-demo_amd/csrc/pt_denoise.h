// pt_denoise.h -- the NRD stand-in (row N9): a ReLAX-style denoiser of the SVGF family that reads and writes the resources the
// reference tags for NRD (App::ProcessNRD, Source/App.cpp:1549-1642): temporal accumulation reprojected with the G-buffer's motion
// vectors, a variance estimate from luminance moments, and an edge-stopping a-trous wavelet filter (DESIGN.md spec S15).
// Per-pixel functions for the kernels of pt_denoise.hip; they also compile as host C++ (tests/hostshim/denoise_host.cpp), so the GPU
// output is pinned bit for bit to the host-compiled header.  fp32 throughout, no contraction (-ffp-contract=off), no pt_fma.
#pragma once

#include "pt_nrd.h"

namespace pt {

constexpr uint32_t kDnDefaultFrames = 30, kDnDefaultIterations = 5, kDnMaxIterations = 8;
constexpr float kDnLog2e = 1.44269504088896340736f;
constexpr float kDnDepthRel = 0.05f;     // reprojection and hit-distance reconstruction: |z' - z| <= 0.05 |z|
constexpr float kDnNormalMin = 0.9f;     // reprojection: dot(n', n) >= 0.9
constexpr float kDnWeightMin = 1e-3f;    // a bilinear footprint whose valid weights sum below this is disoccluded
constexpr float kDnSpatialBelow = 4.0f;  // history shorter than this: 7x7 spatial variance
constexpr float kDnSigmaZ = 1.0f, kDnEpsZ = 1e-3f;  // w_z = exp(-|z_p - z_q| / (sigma_z |grad z_p . (p - q)| + eps_z))
constexpr float kDnSigmaL = 4.0f, kDnEpsL = 1e-4f;  // w_l = exp(-|l_p - l_q| / (sigma_l sqrt(g3x3(var_p)) + eps_l))
constexpr float kDnRoughDen = 0.1f + 1e-6f;         // w_r = exp(-|r_p - r_q| / (0.1 + eps)), specular only
constexpr float kDnRoughFull = 0.5f;  // specular: history cap and a-trous strength reach their full value at this roughness

// the 5-tap B-spline of the a-trous steps and the 3x3 Gaussian of the variance, by |offset|
PT_HD float dn_bspline(int i) { return i == 0 ? 0.375f : (i == 1 ? 0.25f : 0.0625f); }
PT_HD float dn_gauss(int i) { return i == 0 ? 0.5f : 0.25f; }

PT_HD float4 dn_f4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
PT_HD f3 dn_rgb(float4 v) { return make_f3(v.x, v.y, v.z); }
// dot product and Rec.709 luminance, summed left to right (no fma)
PT_HD float dn_dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PT_HD float dn_lum(f3 c) { return c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f; }

// exp(-x) for x >= 0 as exp2_spec(-x log2e); x >= 80 (and NaN) -> 0, below exp2_spec's range
PT_HD float dn_exp_neg(float x) { return x < 80.0f ? exp2_spec(-x * kDnLog2e) : 0.0f; }

// max(0, n_p . n_q)^128 as seven squarings
PT_HD float dn_wn(f3 a, f3 b)
{
    float d = pt_max(dn_dot(a, b), 0.0f);
    for (int k = 0; k < 7; k++) d = d * d;
    return d;
}

PT_HD float dn_wz(float zp, float zq, float gx, float gy, int ox, int oy)
{
    const float den = kDnSigmaZ * pt_abs(gx * (float)ox + gy * (float)oy) + kDnEpsZ;
    return dn_exp_neg(pt_abs(zp - zq) / den);
}

// w_l and w_r multiply by a reciprocal formed once (an IEEE division per pixel, not per tap)
PT_HD float dn_wl(float lp, float lq, float inv_den) { return dn_exp_neg(pt_abs(lp - lq) * inv_den); }
PT_HD float dn_wr(float rp, float rq) { return dn_exp_neg(pt_abs(rp - rq) * (1.0f / kDnRoughDen)); }

// decode an In buffer's rgb to linear RGB (ReBLUR: YCoCg) and encode linear RGB back into the mode's Out encoding
template <uint32_t kMode>
PT_HD f3 dn_decode(float4 v) { return kMode == kNrdReblur ? nrd_ycocg_to_linear(dn_rgb(v)) : dn_rgb(v); }
template <uint32_t kMode>
PT_HD float4 dn_encode(f3 c, float w)
{
    if (kMode == kNrdReblur) c = nrd_linear_to_ycocg(c);
    return dn_f4(c.x, c.y, c.z, w);
}

// The buffers of one call: the caller's (the reference's nrd::ResourceType tags) and the context's history and work buffers, all
// w * h pixels, row-major.  prev_* = the history slot the previous call wrote (read), the others = this call's slot (written).
struct DnBuffers {
    uint32_t w, h;
    const float* viewz;          // IN_VIEWZ: G-buffer LinearDepth
    const float* mv;             // IN_MV: float3, previous - current, in pixels (.z: linear depth)
    const float4* nr;            // IN_NORMAL_ROUGHNESS
    const float4* in_d;          // IN_DIFF_RADIANCE_HITDIST (mode encoding)
    const float4* in_s;          // IN_SPEC_RADIANCE_HITDIST
    float4* out_d;               // OUT_DIFF_RADIANCE_HITDIST
    float4* out_s;               // OUT_SPEC_RADIANCE_HITDIST
    const float4* prev_sig_d;    // history: accumulated linear RGB, .w = history length
    const float4* prev_sig_s;
    const float4* prev_mom;      // history: luminance moments (m1 diffuse, m2 diffuse, m1 specular, m2 specular)
    const float4* prev_guide;    // history: (LinearDepth, normal)
    float4* sig_d;
    float4* sig_s;
    float4* mom;
    float4* guide;
    float* hitd;                 // reconstructed hit distance, 2 per pixel (diffuse, specular)
    float4* xd[2];               // a-trous ping-pong: (linear RGB, variance)
    float4* xs[2];
};

struct DnParams {
    uint32_t max_d, max_s;  // MaxDiffuseFrames / MaxSpecularFrames (0 already replaced by 30)
    uint32_t restart;       // nonzero: no history is read (RESTART, CLEAR_AND_RESTART, first call, size or mode change)
};

PT_HD bool dn_hit_at(const DnBuffers& b, int x, int y)
{
    return x >= 0 && y >= 0 && x < (int)b.w && y < (int)b.h && is_finite(b.viewz[(size_t)y * b.w + x]);
}

// one axis of grad z: of the one-sided differences towards hit neighbours inside the image, the one of smaller magnitude (the
// backward one on a tie); 0 without such a neighbour
PT_HD float dn_grad_axis(float z, bool hm, float zm, bool hp, float zp)
{
    const float dm = z - zm, dp = zp - z;
    if (hm && hp) return pt_abs(dp) < pt_abs(dm) ? dp : dm;
    if (hm) return dm;
    if (hp) return dp;
    return 0.0f;
}

PT_HD void dn_grad(const DnBuffers& b, int x, int y, float z, float& gx, float& gy)
{
    const bool xm = dn_hit_at(b, x - 1, y), xp = dn_hit_at(b, x + 1, y), ym = dn_hit_at(b, x, y - 1), yp = dn_hit_at(b, x, y + 1);
    const size_t i = (size_t)y * b.w + x;
    gx = dn_grad_axis(z, xm, xm ? b.viewz[i - 1] : 0.0f, xp, xp ? b.viewz[i + 1] : 0.0f);
    gy = dn_grad_axis(z, ym, ym ? b.viewz[i - b.w] : 0.0f, yp, yp ? b.viewz[i + b.w] : 0.0f);
}

// Pass (a) at pixel (x, y): hit-distance reconstruction, anti-firefly, reprojection, accumulation and moments of both lobes.
// Writes this call's history slot (a miss: zeros, history length 0, its depth in the guide) and the reconstructed hit distances.
template <uint32_t kMode>
PT_HD void dn_temporal_px(const DnBuffers& b, const DnParams& P, int x, int y)
{
    const size_t i = (size_t)y * b.w + x;
    const float z = b.viewz[i];
    if (!is_finite(z)) {
        const float4 zero = dn_f4(0.0f, 0.0f, 0.0f, 0.0f);
        b.sig_d[i] = zero;
        b.sig_s[i] = zero;
        b.mom[i] = zero;
        b.guide[i] = dn_f4(z, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 nr = b.nr[i];
    const f3 n = dn_rgb(nr);
    const float4 ind = b.in_d[i], ins = b.in_s[i];
    f3 cd = dn_decode<kMode>(ind), cs = dn_decode<kMode>(ins);
    // the 3x3 hit neighbours (row by row): the largest luminance, and the non-zero hit distances of those within the depth test
    bool any = false;
    float lmax_d = 0.0f, lmax_s = 0.0f, hsum_d = 0.0f, hsum_s = 0.0f, hn_d = 0.0f, hn_s = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if ((dx == 0 && dy == 0) || !dn_hit_at(b, x + dx, y + dy)) continue;
            const size_t j = (size_t)(y + dy) * b.w + (x + dx);
            const float4 qd = b.in_d[j], qs = b.in_s[j];
            const float ld = dn_lum(dn_decode<kMode>(qd)), ls = dn_lum(dn_decode<kMode>(qs));
            lmax_d = any ? pt_max(lmax_d, ld) : ld;
            lmax_s = any ? pt_max(lmax_s, ls) : ls;
            any = true;
            if (pt_abs(b.viewz[j] - z) <= kDnDepthRel * pt_abs(z)) {
                if (qd.w != 0.0f) { hsum_d = hsum_d + qd.w; hn_d = hn_d + 1.0f; }
                if (qs.w != 0.0f) { hsum_s = hsum_s + qs.w; hn_s = hn_s + 1.0f; }
            }
        }
    const float hd_d = (ind.w == 0.0f && hn_d > 0.0f) ? hsum_d / hn_d : ind.w;
    const float hd_s = (ins.w == 0.0f && hn_s > 0.0f) ? hsum_s / hn_s : ins.w;
    // anti-firefly: luminance clamped to the neighbours' largest, the RGB scaled
    float ld = dn_lum(cd), ls = dn_lum(cs);
    if (any && ld > lmax_d) { cd = cd * (lmax_d / ld); ld = dn_lum(cd); }
    if (any && ls > lmax_s) { cs = cs * (lmax_s / ls); ls = dn_lum(cs); }
    // reprojection: bilinear footprint of the previous slot around p + MotionVector.xy
    const f3 mv = make_f3(b.mv[3 * i], b.mv[3 * i + 1], b.mv[3 * i + 2]);
    const float fx = (float)x + mv.x, fy = (float)y + mv.y, ze = z + mv.z;
    float sw = 0.0f;
    f3 hd = make_f3(0.0f, 0.0f, 0.0f), hs = make_f3(0.0f, 0.0f, 0.0f);
    float nd = 0.0f, ns = 0.0f;
    float4 hm = dn_f4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!P.restart && fx > -1.0f && fy > -1.0f && fx < (float)b.w && fy < (float)b.h) {
        const float x0f = pt_floor(fx), y0f = pt_floor(fy);
        const float tx = fx - x0f, ty = fy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        for (int k = 0; k < 4; k++) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            if (qx < 0 || qy < 0 || qx >= (int)b.w || qy >= (int)b.h) continue;
            const size_t j = (size_t)qy * b.w + qx;
            const float4 g = b.prev_guide[j];
            if (!is_finite(g.x) || !(pt_abs(g.x - ze) <= kDnDepthRel * pt_abs(ze)) || !(dn_dot(make_f3(g.y, g.z, g.w), n) >= kDnNormalMin)) continue;
            const float wt = ((k & 1) ? tx : 1.0f - tx) * ((k >> 1) ? ty : 1.0f - ty);
            const float4 pd = b.prev_sig_d[j], ps = b.prev_sig_s[j], pm = b.prev_mom[j];
            sw = sw + wt;
            hd = hd + dn_rgb(pd) * wt;
            hs = hs + dn_rgb(ps) * wt;
            nd = nd + pd.w * wt;
            ns = ns + ps.w * wt;
            hm = dn_f4(hm.x + pm.x * wt, hm.y + pm.y * wt, hm.z + pm.z * wt, hm.w + pm.w * wt);
        }
    }
    if (sw >= kDnWeightMin) {
        const float r = 1.0f / sw;
        hd = hd * r; hs = hs * r; nd = nd * r; ns = ns * r;
        hm = dn_f4(hm.x * r, hm.y * r, hm.z * r, hm.w * r);
    } else {  // disoccluded
        hd = make_f3(0.0f, 0.0f, 0.0f); hs = hd; nd = 0.0f; ns = 0.0f;
        hm = dn_f4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    // accumulation: n = min(n_hist + 1, cap), c = lerp(c_hist, c_cur, 1 / n), the moments alike
    const float cap_s = pt_max(1.0f, pt_floor((float)P.max_s * saturate(nr.w / kDnRoughFull) + 0.5f));
    const float n_d = pt_min(nd + 1.0f, (float)P.max_d), n_s = pt_min(ns + 1.0f, cap_s);
    const float a_d = 1.0f / n_d, a_s = 1.0f / n_s;
    cd = hd + (cd - hd) * a_d;
    cs = hs + (cs - hs) * a_s;
    b.sig_d[i] = dn_f4(cd.x, cd.y, cd.z, n_d);
    b.sig_s[i] = dn_f4(cs.x, cs.y, cs.z, n_s);
    b.mom[i] = dn_f4(hm.x + (ld - hm.x) * a_d, hm.y + (ld * ld - hm.y) * a_d, hm.z + (ls - hm.z) * a_s, hm.w + (ls * ls - hm.w) * a_s);
    b.guide[i] = dn_f4(z, n.x, n.y, n.z);
    b.hitd[2 * i] = hd_d;
    b.hitd[2 * i + 1] = hd_s;
}

// Pass (b): the variance of each lobe -- temporal (max(m2 - m1^2, 0)) from a history of 4 frames on, else over the 7x7 hit
// neighbours with the edge weights w_z w_n (specular: also w_r) -- into the first a-trous buffer next to the accumulated RGB
PT_HD void dn_variance_px(const DnBuffers& b, int x, int y)
{
    const size_t i = (size_t)y * b.w + x;
    const float z = b.viewz[i];
    if (!is_finite(z)) return;
    const float4 sd = b.sig_d[i], ss = b.sig_s[i], m = b.mom[i];
    float vd = pt_max(m.y - m.x * m.x, 0.0f), vs = pt_max(m.w - m.z * m.z, 0.0f);
    if (sd.w < kDnSpatialBelow || ss.w < kDnSpatialBelow) {
        const float4 nr = b.nr[i];
        const f3 n = dn_rgb(nr);
        float gx, gy;
        dn_grad(b, x, y, z, gx, gy);
        float swd = 0.0f, m1d = 0.0f, m2d = 0.0f, sws = 0.0f, m1s = 0.0f, m2s = 0.0f;
        for (int dy = -3; dy <= 3; dy++)
            for (int dx = -3; dx <= 3; dx++) {
                if (!dn_hit_at(b, x + dx, y + dy)) continue;
                const size_t j = (size_t)(y + dy) * b.w + (x + dx);
                const float4 q = b.nr[j], mq = b.mom[j];
                const float w = dn_wz(z, b.viewz[j], gx, gy, dx, dy) * dn_wn(n, dn_rgb(q));
                const float ws = w * dn_wr(nr.w, q.w);
                swd = swd + w; m1d = m1d + w * mq.x; m2d = m2d + w * mq.y;
                sws = sws + ws; m1s = m1s + ws * mq.z; m2s = m2s + ws * mq.w;
            }
        if (sd.w < kDnSpatialBelow) {
            const float a = swd > 0.0f ? m1d / swd : 0.0f, c = swd > 0.0f ? m2d / swd : 0.0f;
            vd = pt_max(c - a * a, 0.0f);
        }
        if (ss.w < kDnSpatialBelow) {
            const float a = sws > 0.0f ? m1s / sws : 0.0f, c = sws > 0.0f ? m2s / sws : 0.0f;
            vs = pt_max(c - a * a, 0.0f);
        }
    }
    b.xd[0][i] = dn_f4(sd.x, sd.y, sd.z, vd);
    b.xs[0][i] = dn_f4(ss.x, ss.y, ss.z, vs);
}

// Pass (c), one a-trous step of `step` pixels from xd/xs[src] into xd/xs[1 - src], or, on the last step, into OutDiffuse /
// OutSpecular in the mode's encoding with the reconstructed hit distance in .w.  c = c_p + sum w (c_q - c_p) / sum w,
// var = sum w^2 var_q / (sum w)^2; w = h w_z w_n w_l (specular: h w_z w_n w_l w_r, off the centre times s_p = saturate(r_p / 0.5):
// a mirror's reflection is image detail, not noise, so it is filtered in proportion to the roughness).
template <uint32_t kMode, bool kLast>
PT_HD void dn_atrous_px(const DnBuffers& b, int src, int step, int x, int y)
{
    const size_t i = (size_t)y * b.w + x;
    const float z = b.viewz[i];
    if (!is_finite(z)) return;
    const float4* xd = b.xd[src];
    const float4* xs = b.xs[src];
    const float4 nr = b.nr[i], pd = xd[i], ps = xs[i];
    const f3 n = dn_rgb(nr), cd = dn_rgb(pd), cs = dn_rgb(ps);
    float gx, gy;
    dn_grad(b, x, y, z, gx, gy);
    // 3x3 Gaussian of the variance over the hit neighbours
    float gk = 0.0f, gd = 0.0f, gs = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if (!dn_hit_at(b, x + dx, y + dy)) continue;
            const size_t j = (size_t)(y + dy) * b.w + (x + dx);
            const float k = dn_gauss(dy < 0 ? -dy : dy) * dn_gauss(dx < 0 ? -dx : dx);
            gk = gk + k; gd = gd + k * xd[j].w; gs = gs + k * xs[j].w;
        }
    const float inv_d = 1.0f / (kDnSigmaL * pt_sqrt(gd / gk) + kDnEpsL), inv_s = 1.0f / (kDnSigmaL * pt_sqrt(gs / gk) + kDnEpsL);
    const float lpd = dn_lum(cd), lps = dn_lum(cs), sp = saturate(nr.w / kDnRoughFull);
    float swd = 0.0f, sws = 0.0f, vd = 0.0f, vs = 0.0f;
    f3 ad = make_f3(0.0f, 0.0f, 0.0f), as = ad;
    for (int ty = -2; ty <= 2; ty++)
        for (int tx = -2; tx <= 2; tx++) {
            const int ox = tx * step, oy = ty * step;
            if (!dn_hit_at(b, x + ox, y + oy)) continue;
            const size_t j = (size_t)(y + oy) * b.w + (x + ox);
            const float4 q = b.nr[j], qd = xd[j], qs = xs[j];
            const float h = dn_bspline(ty < 0 ? -ty : ty) * dn_bspline(tx < 0 ? -tx : tx);
            const float wzn = (h * dn_wz(z, b.viewz[j], gx, gy, ox, oy)) * dn_wn(n, dn_rgb(q));
            const f3 ed = dn_rgb(qd), es = dn_rgb(qs);
            const float wd = wzn * dn_wl(lpd, dn_lum(ed), inv_d);
            const float ws = ((wzn * dn_wl(lps, dn_lum(es), inv_s)) * dn_wr(nr.w, q.w)) * (tx == 0 && ty == 0 ? 1.0f : sp);
            swd = swd + wd; ad = ad + (ed - cd) * wd; vd = vd + (wd * wd) * qd.w;
            sws = sws + ws; as = as + (es - cs) * ws; vs = vs + (ws * ws) * qs.w;
        }
    const f3 od = swd > 0.0f ? cd + ad * (1.0f / swd) : cd;
    const f3 os = sws > 0.0f ? cs + as * (1.0f / sws) : cs;
    if (kLast) {
        b.out_d[i] = dn_encode<kMode>(od, b.hitd[2 * i]);
        b.out_s[i] = dn_encode<kMode>(os, b.hitd[2 * i + 1]);
    } else {
        b.xd[1 - src][i] = dn_f4(od.x, od.y, od.z, swd > 0.0f ? vd / (swd * swd) : pd.w);
        b.xs[1 - src][i] = dn_f4(os.x, os.y, os.z, sws > 0.0f ? vs / (sws * sws) : ps.w);
    }
}

#if defined(__HIPCC__)
// pt_denoise.hip: pass (a), pass (b) and `iterations` a-trous steps of mode kNrdReblur / kNrdRelax, in order on `stream`
hipError_t launch_nrd_denoise(const DnBuffers& b, uint32_t mode, const DnParams& P, uint32_t iterations, hipStream_t stream);
#endif

}  // namespace pt
