// pt_reblur.h -- the ReBLUR stand-in (row N30): a recurrent-blur denoiser of the family NRD's ReBLUR comes from, reading and writing
// the resources the reference tags for NRD (App::ProcessNRD, Source/App.cpp:1549-1642) in ReBLUR's encoding (YCoCg + normalised hit
// distance): temporal accumulation into a slow and a fast history, a history fix and a clamp of the slow history to the fast one, and
// two blur passes over a rotated 8-point disc whose radius shrinks with the history length and grows with the normalised hit distance;
// the blurred result is the next call's history (DESIGN.md spec S32).  The arithmetic is this project's own: the NRD SDK is not
// vendored and no parity with it is claimed.
// Per-pixel functions for the kernels of pt_reblur.hip; they also compile as host C++ (tests/hostshim/reblur_host.cpp), so the GPU
// output is pinned bit for bit to the host-compiled header.  fp32 throughout, no contraction (-ffp-contract=off), no pt_fma.  The
// filter works on the YCoCg-encoded signal (every step is linear in it); Y serves as the luminance.
#pragma once

#include "pt_denoise.h"

namespace pt {

constexpr uint32_t kRbDefaultFrames = 30, kRbDefaultFastFrames = 6, kRbDefaultFixFrames = 3;  // nrd::ReblurSettings as recollected
constexpr float kRbDefaultMinRadius = 1.0f, kRbDefaultMaxRadius = 30.0f, kRbMaxRadius = 64.0f;
constexpr float kRbMotion = 2.0f;      // specular cap: the share of MaxAccumulatedFrames above S15's cap is 1 / (1 + 2 |MV.xy|)
constexpr int kRbFixStride = 2;        // history fix: the 5x5 taps are 2 pixels apart
constexpr float kRbClampSigma = 2.0f;  // fast clamp: mean +- 2 sigma of the fast history's 3x3 hit taps
constexpr float kRbSigmaH = 1.0f, kRbEpsH = 0.1f;  // w_h = exp(-|a_p - a_q| / (sigma_h a_p + eps_h)), a = normalised hit distance

// the 8 points of the blur's disc (a Vogel spiral: radius sqrt((k + 1/2) / 8), angle k * 2.39996 rad)
PT_HD void rb_disc(int k, float& px, float& py)
{
    switch (k) {
    case 0: px = 0.25000000f; py = 0.00000000f; break;
    case 1: px = -0.31929010f; py = 0.29249588f; break;
    case 2: px = 0.04887247f; py = -0.55687654f; break;
    case 3: px = 0.40244448f; py = 0.52491754f; break;
    case 4: px = -0.73853511f; py = -0.13063647f; break;
    case 5: px = 0.69960493f; py = -0.44503140f; break;
    case 6: px = -0.23400415f; py = 0.87048382f; break;
    default: px = -0.44627130f; py = -0.85926825f; break;
    }
}

// (cos, sin) of 2 pi k / 16, k = 0..15: the four tabulated pairs of the first quadrant, turned by k / 4 quarter turns
PT_HD void rb_rotation(uint32_t k, float& c, float& s)
{
    const uint32_t j = k & 3u, q = (k >> 2) & 3u;
    const float c0 = j == 0 ? 1.0f : (j == 1 ? 0.92387950f : (j == 2 ? 0.70710677f : 0.38268343f));
    const float s0 = j == 0 ? 0.0f : (j == 1 ? 0.38268343f : (j == 2 ? 0.70710677f : 0.92387950f));
    c = q == 0 ? c0 : (q == 1 ? -s0 : (q == 2 ? -c0 : s0));
    s = q == 0 ? s0 : (q == 1 ? c0 : (q == 2 ? -s0 : -c0));
}

// The buffers of one call: the caller's (the reference's nrd::ResourceType tags) and the context's history and work buffers, all
// w * h pixels, row-major.  prev_* = the history slot the previous call wrote (read), the others = this call's slot (written).
struct RbBuffers {
    uint32_t w, h;
    const float* viewz;          // IN_VIEWZ
    const float* mv;             // IN_MV: float3, previous - current, in pixels (.z: linear depth)
    const float4* nr;            // IN_NORMAL_ROUGHNESS
    const float4* in_d;          // IN_DIFF_RADIANCE_HITDIST (YCoCg, normalised hit distance)
    const float4* in_s;          // IN_SPEC_RADIANCE_HITDIST
    float4* out_d;               // OUT_DIFF_RADIANCE_HITDIST
    float4* out_s;               // OUT_SPEC_RADIANCE_HITDIST
    const float4* prev_slow[2];  // history, diffuse / specular: the blurred slow signal (YCoCg), .w = its reconstructed hit distance
    const float4* prev_fast[2];  // history: the fast signal (YCoCg), .w = the history length n
    const float4* prev_guide;    // history: (ViewZ, normal)
    float4* slow[2];
    float4* fast[2];
    float4* guide;
    float4* x[2];                // work: (signal, reconstructed hit distance) after pass (a) and after pass (c)
};

struct RbParams {
    uint32_t max_n, max_fast, fix_frames;  // MaxAccumulatedFrames, MaxFastAccumulatedFrames, HistoryFixFrames (0 already replaced)
    uint32_t restart;                      // nonzero: no history is read
    uint32_t frame;                        // FrameIndex: turns the tap pattern
    float rmin, rmax;                      // MinBlurRadius, MaxBlurRadius in pixels (0 already replaced)
};

// pt_denoise.h's guide helpers (dn_hit_at, dn_grad) read w, h and viewz of a DnBuffers
PT_HD DnBuffers rb_guides(const RbBuffers& b)
{
    DnBuffers g{};
    g.w = b.w;
    g.h = b.h;
    g.viewz = b.viewz;
    return g;
}

// the specular history cap: S15's roughness-scaled cap c15, raised to MaxAccumulatedFrames at rest and falling back to c15 as the
// surface's screen motion m = |MV.xy| (pixels) grows: max(1, floor(c15 + (N - c15) / (1 + 2 m) + 0.5)); a motion that is not finite: c15
PT_HD float rb_spec_cap(uint32_t max_n, float roughness, float mx, float my)
{
    const float c15 = pt_max(1.0f, pt_floor((float)max_n * saturate(roughness / kDnRoughFull) + 0.5f));
    const float m = pt_sqrt(mx * mx + my * my);
    const float t = is_finite(m) ? 1.0f / (1.0f + kRbMotion * m) : 0.0f;
    return pt_max(1.0f, pt_floor(c15 + ((float)max_n - c15) * t + 0.5f));
}

// the blur radius of a lobe in pixels: clamp(Rmax sqrt(a / n), Rmin, Rmax) with n >= 1 the history length and a the normalised hit
// distance; specular multiplies it by saturate(r / 0.5)
PT_HD float rb_radius(const RbParams& P, float n, float a)
{
    const float r = P.rmax * pt_sqrt(a * (1.0f / n));
    return pt_min(pt_max(r, P.rmin), P.rmax);
}

PT_HD int rb_round(float v) { return (int)pt_floor(v + 0.5f); }

// Pass (a) at pixel (x, y): hit-distance reconstruction, anti-firefly, reprojection and accumulation of the slow and the fast
// history of both lobes.  Writes x[] = (slow signal, hit distance), this call's fast[] = (fast signal, n) and guide; a miss: zeros in
// x[], slow[] and fast[] (history length 0), its depth in the guide.
PT_HD void rb_temporal_px(const RbBuffers& b, const RbParams& P, int x, int y)
{
    const DnBuffers g = rb_guides(b);
    const size_t i = (size_t)y * b.w + x;
    const float z = b.viewz[i];
    if (!is_finite(z)) {
        const float4 zero = dn_f4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int l = 0; l < 2; l++) { b.x[l][i] = zero; b.slow[l][i] = zero; b.fast[l][i] = zero; }
        b.guide[i] = dn_f4(z, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 nr = b.nr[i];
    const f3 n = dn_rgb(nr);
    const float4 ind = b.in_d[i], ins = b.in_s[i];
    f3 cd = dn_rgb(ind), cs = dn_rgb(ins);
    // the 3x3 hit neighbours (row by row): the largest Y, and the non-zero hit distances of those within the depth test
    bool any = false;
    float lmax_d = 0.0f, lmax_s = 0.0f, hsum_d = 0.0f, hsum_s = 0.0f, hn_d = 0.0f, hn_s = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if ((dx == 0 && dy == 0) || !dn_hit_at(g, x + dx, y + dy)) continue;
            const size_t j = (size_t)(y + dy) * b.w + (x + dx);
            const float4 qd = b.in_d[j], qs = b.in_s[j];
            lmax_d = any ? pt_max(lmax_d, qd.x) : qd.x;
            lmax_s = any ? pt_max(lmax_s, qs.x) : qs.x;
            any = true;
            if (pt_abs(b.viewz[j] - z) <= kDnDepthRel * pt_abs(z)) {
                if (qd.w != 0.0f) { hsum_d = hsum_d + qd.w; hn_d = hn_d + 1.0f; }
                if (qs.w != 0.0f) { hsum_s = hsum_s + qs.w; hn_s = hn_s + 1.0f; }
            }
        }
    const float hd_d = (ind.w == 0.0f && hn_d > 0.0f) ? hsum_d / hn_d : ind.w;
    const float hd_s = (ins.w == 0.0f && hn_s > 0.0f) ? hsum_s / hn_s : ins.w;
    // anti-firefly: Y clamped to the neighbours' largest, the signal scaled
    if (any && cd.x > lmax_d) cd = cd * (lmax_d / cd.x);
    if (any && cs.x > lmax_s) cs = cs * (lmax_s / cs.x);
    // reprojection: bilinear footprint of the previous slot around p + MotionVector.xy
    const f3 mv = make_f3(b.mv[3 * i], b.mv[3 * i + 1], b.mv[3 * i + 2]);
    const float fx = (float)x + mv.x, fy = (float)y + mv.y, ze = z + mv.z;
    const f3 zero3 = make_f3(0.0f, 0.0f, 0.0f);
    float sw = 0.0f, nd = 0.0f, ns = 0.0f;
    f3 hd = zero3, hs = zero3, gd = zero3, gs = zero3;  // slow and fast history of each lobe
    if (!P.restart && fx > -1.0f && fy > -1.0f && fx < (float)b.w && fy < (float)b.h) {
        const float x0f = pt_floor(fx), y0f = pt_floor(fy);
        const float tx = fx - x0f, ty = fy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        for (int k = 0; k < 4; k++) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            if (qx < 0 || qy < 0 || qx >= (int)b.w || qy >= (int)b.h) continue;
            const size_t j = (size_t)qy * b.w + qx;
            const float4 pg = b.prev_guide[j];
            if (!is_finite(pg.x) || !(pt_abs(pg.x - ze) <= kDnDepthRel * pt_abs(ze)) || !(dn_dot(make_f3(pg.y, pg.z, pg.w), n) >= kDnNormalMin)) continue;
            const float wt = ((k & 1) ? tx : 1.0f - tx) * ((k >> 1) ? ty : 1.0f - ty);
            const float4 fd = b.prev_fast[0][j], fs = b.prev_fast[1][j];
            sw = sw + wt;
            hd = hd + dn_rgb(b.prev_slow[0][j]) * wt;
            hs = hs + dn_rgb(b.prev_slow[1][j]) * wt;
            gd = gd + dn_rgb(fd) * wt;
            gs = gs + dn_rgb(fs) * wt;
            nd = nd + fd.w * wt;
            ns = ns + fs.w * wt;
        }
    }
    if (sw >= kDnWeightMin) {
        const float r = 1.0f / sw;
        hd = hd * r; hs = hs * r; gd = gd * r; gs = gs * r; nd = nd * r; ns = ns * r;
    } else {  // disoccluded
        hd = zero3; hs = zero3; gd = zero3; gs = zero3; nd = 0.0f; ns = 0.0f;
    }
    // accumulation: n = min(n_hist + 1, cap), c = lerp(c_hist, c_cur, 1 / n); the fast history with min(n, MaxFastAccumulatedFrames)
    const float n_d = pt_min(nd + 1.0f, (float)P.max_n), n_s = pt_min(ns + 1.0f, rb_spec_cap(P.max_n, nr.w, mv.x, mv.y));
    const float a_d = 1.0f / n_d, a_s = 1.0f / n_s;
    const float f_d = 1.0f / pt_min(n_d, (float)P.max_fast), f_s = 1.0f / pt_min(n_s, (float)P.max_fast);
    const f3 sd = hd + (cd - hd) * a_d, ss = hs + (cs - hs) * a_s;
    const f3 qd = gd + (cd - gd) * f_d, qs = gs + (cs - gs) * f_s;
    b.x[0][i] = dn_f4(sd.x, sd.y, sd.z, hd_d);
    b.x[1][i] = dn_f4(ss.x, ss.y, ss.z, hd_s);
    b.fast[0][i] = dn_f4(qd.x, qd.y, qd.z, n_d);
    b.fast[1][i] = dn_f4(qs.x, qs.y, qs.z, n_s);
    b.guide[i] = dn_f4(z, n.x, n.y, n.z);
}

// the fast clamp of one lobe: c clamped per channel to m +- 2 sigma, m and sigma the mean and the deviation of the fast history over
// the 3x3 hit taps (s1, s2 = the sums of (f_q - f_p) and of its square over the cnt taps: a constant fast history gives m = f_p, sigma = 0)
PT_HD float rb_clamp1(float c, float fp, float s1, float s2, float inv)
{
    const float md = s1 * inv;
    const float sig = kRbClampSigma * pt_sqrt(pt_max(s2 * inv - md * md, 0.0f));
    const float m = fp + md;
    return pt_min(pt_max(c, m - sig), m + sig);
}

PT_HD f3 rb_clamp(f3 c, f3 fp, f3 s1, f3 s2, float inv)
{
    return make_f3(rb_clamp1(c.x, fp.x, s1.x, s2.x, inv), rb_clamp1(c.y, fp.y, s1.y, s2.y, inv), rb_clamp1(c.z, fp.z, s1.z, s2.z, inv));
}

// Pass (b): the history fix of the lobes whose history is shorter than HistoryFixFrames -- the slow signal rebuilt from the 5x5 hit
// taps kRbFixStride pixels apart, w = w_z w_n n_q (specular: w_z w_n w_r n_q, the tap offsets scaled by saturate(r_p / 0.5): a mirror
// has no taps but itself) -- then the fast clamp; from x[] into this call's slow[] (the hit distance in .w passes through)
PT_HD void rb_fix_px(const RbBuffers& b, const RbParams& P, int x, int y)
{
    const DnBuffers g = rb_guides(b);
    const size_t i = (size_t)y * b.w + x;
    const float z = b.viewz[i];
    if (!is_finite(z)) return;
    const float4 pd = b.x[0][i], ps = b.x[1][i], fd = b.fast[0][i], fs = b.fast[1][i];
    const f3 cd = dn_rgb(pd), cs = dn_rgb(ps), fcd = dn_rgb(fd), fcs = dn_rgb(fs);
    f3 od = cd, os = cs;
    // (n + 0.5 < HistoryFixFrames: a whole history length that the bilinear footprint reproduces up to a rounding decides like itself)
    const bool fix_d = fd.w + 0.5f < (float)P.fix_frames, fix_s = fs.w + 0.5f < (float)P.fix_frames;
    if (fix_d || fix_s) {
        const float4 nr = b.nr[i];
        const f3 n = dn_rgb(nr);
        const float sp = saturate(nr.w / kDnRoughFull);
        float gx, gy;
        dn_grad(g, x, y, z, gx, gy);
        float swd = 0.0f, sws = 0.0f;
        f3 ad = make_f3(0.0f, 0.0f, 0.0f), as = ad;
        for (int ty = -2; ty <= 2; ty++)
            for (int tx = -2; tx <= 2; tx++) {
                const bool centre = tx == 0 && ty == 0;
                const int ox = tx * kRbFixStride, oy = ty * kRbFixStride;
                if (fix_d && dn_hit_at(g, x + ox, y + oy)) {
                    const size_t j = (size_t)(y + oy) * b.w + (x + ox);
                    const float wd = (dn_wz(z, b.viewz[j], gx, gy, ox, oy) * dn_wn(n, dn_rgb(b.nr[j]))) * b.fast[0][j].w;
                    swd = swd + wd; ad = ad + (dn_rgb(b.x[0][j]) - cd) * wd;
                }
                // specular: the offsets scaled by saturate(r_p / 0.5) and rounded; off the centre, one that rounds to the centre is no tap
                const int sx = rb_round((float)ox * sp), sy = rb_round((float)oy * sp);
                if (fix_s && (centre || sx != 0 || sy != 0) && dn_hit_at(g, x + sx, y + sy)) {
                    const size_t j = (size_t)(y + sy) * b.w + (x + sx);
                    const float4 q = b.nr[j];
                    const float ws = ((dn_wz(z, b.viewz[j], gx, gy, sx, sy) * dn_wn(n, dn_rgb(q))) * dn_wr(nr.w, q.w)) * b.fast[1][j].w;
                    sws = sws + ws; as = as + (dn_rgb(b.x[1][j]) - cs) * ws;
                }
            }
        if (fix_d && swd > 0.0f) od = cd + ad * (1.0f / swd);
        if (fix_s && sws > 0.0f) os = cs + as * (1.0f / sws);
    }
    // fast clamp over the 3x3 hit taps (row by row, the centre among them)
    float cnt = 0.0f;
    f3 s1d = make_f3(0.0f, 0.0f, 0.0f), s2d = s1d, s1s = s1d, s2s = s1d;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if (!dn_hit_at(g, x + dx, y + dy)) continue;
            const size_t j = (size_t)(y + dy) * b.w + (x + dx);
            const f3 ed = dn_rgb(b.fast[0][j]) - fcd, es = dn_rgb(b.fast[1][j]) - fcs;
            cnt = cnt + 1.0f;
            s1d = s1d + ed; s2d = s2d + ed * ed;
            s1s = s1s + es; s2s = s2s + es * es;
        }
    const float inv = 1.0f / cnt;
    od = rb_clamp(od, fcd, s1d, s2d, inv);
    os = rb_clamp(os, fcs, s1s, s2s, inv);
    b.slow[0][i] = dn_f4(od.x, od.y, od.z, pd.w);
    b.slow[1][i] = dn_f4(os.x, os.y, os.z, ps.w);
}

// one lobe's blur at a hit pixel: the centre (weight 1) and the 8 disc points turned by (rc, rs), scaled by `radius` and rounded to
// the nearest pixel; a point that rounds to the centre or does not land on a hit pixel inside the image is no tap.
// w = w_z w_n w_h (specular: w_z w_n w_r w_h); c' = c_p + (sum w (c_q - c_p)) (1 / sum w)
template <bool kSpecular>
PT_HD f3 rb_blur_lobe(const RbBuffers& b, const DnBuffers& g, const float4* src, int x, int y, float z, float4 nr, float gx, float gy, float4 p,
                      float radius, float rc, float rs)
{
    const f3 n = dn_rgb(nr), c = dn_rgb(p);
    const float inv_h = 1.0f / (kRbSigmaH * p.w + kRbEpsH);
    float sw = 1.0f;
    f3 acc = make_f3(0.0f, 0.0f, 0.0f);
    for (int k = 0; k < 8; k++) {
        float px, py;
        rb_disc(k, px, py);
        const int ox = rb_round((px * rc - py * rs) * radius), oy = rb_round((px * rs + py * rc) * radius);
        if ((ox == 0 && oy == 0) || !dn_hit_at(g, x + ox, y + oy)) continue;
        const size_t j = (size_t)(y + oy) * b.w + (x + ox);
        const float4 q = b.nr[j], e = src[j];
        float w = dn_wz(z, b.viewz[j], gx, gy, ox, oy) * dn_wn(n, dn_rgb(q));
        if (kSpecular) w = w * dn_wr(nr.w, q.w);
        w = w * dn_exp_neg(pt_abs(p.w - e.w) * inv_h);
        sw = sw + w;
        acc = acc + (dn_rgb(e) - c) * w;
    }
    return c + acc * (1.0f / sw);
}

// Pass (c) (kPost = false: this call's slow[] -> x[]) and pass (d) (kPost = true: x[] -> Out and this call's slow[], the next call's
// history).  The rotation is entry ((x & 3) + 4 (y & 3) + FrameIndex + (kPost ? 8 : 0)) & 15 of the table.
template <bool kPost>
PT_HD void rb_blur_px(const RbBuffers& b, const RbParams& P, int x, int y)
{
    const DnBuffers g = rb_guides(b);
    const size_t i = (size_t)y * b.w + x;
    const float z = b.viewz[i];
    if (!is_finite(z)) return;
    const float4* const src_d = kPost ? b.x[0] : b.slow[0];
    const float4* const src_s = kPost ? b.x[1] : b.slow[1];
    const float4 nr = b.nr[i], pd = src_d[i], ps = src_s[i];
    float gx, gy, rc, rs;
    dn_grad(g, x, y, z, gx, gy);
    rb_rotation(((uint32_t)x & 3u) + (((uint32_t)y & 3u) << 2) + P.frame + (kPost ? 8u : 0u), rc, rs);
    const float rad_d = rb_radius(P, b.fast[0][i].w, pd.w), rad_s = saturate(nr.w / kDnRoughFull) * rb_radius(P, b.fast[1][i].w, ps.w);
    const f3 od = rb_blur_lobe<false>(b, g, src_d, x, y, z, nr, gx, gy, pd, rad_d, rc, rs);
    const f3 os = rb_blur_lobe<true>(b, g, src_s, x, y, z, nr, gx, gy, ps, rad_s, rc, rs);
    const float4 rd = dn_f4(od.x, od.y, od.z, pd.w), rsp = dn_f4(os.x, os.y, os.z, ps.w);
    if (kPost) {
        b.out_d[i] = rd; b.out_s[i] = rsp;
        b.slow[0][i] = rd; b.slow[1][i] = rsp;
    } else {
        b.x[0][i] = rd; b.x[1][i] = rsp;
    }
}

#if defined(__HIPCC__)
// pt_reblur.hip: passes (a) to (d), four launches in order on `stream`
hipError_t launch_nrd_reblur(const RbBuffers& b, const RbParams& P, hipStream_t stream);
#endif

}  // namespace pt
