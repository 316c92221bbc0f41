// pt_chromab.h -- chromatic aberration (row N29): per-channel radial fringing about a focus point, the entry the reference's README
// lists between NVIDIA Image Scaling and Bloom in its Post-Processing settings.  The reference tree at hand has no source for it, so
// the arithmetic is this project's own (DESIGN.md spec S31); no parity with upstream is claimed.
// Per-pixel functions for the kernel of pt_chromab.hip; they also compile as host C++ (tests/hostshim/chromab_host.cpp), so the GPU
// output is pinned bit for bit to the host-compiled header.  fp32 throughout, no contraction (-ffp-contract=off), no fma anywhere.
//
// Channel c of output texel (x, y) is the bilinear sample (clamp addressing) of channel c of the sanitised input at
//   sx = x + ((x + 0.5) - fx) k_c,  sy = y + ((y + 0.5) - fy) k_c      (texel-centre coordinates; fx = FocusUV.x W, fy = FocusUV.y H)
// so k_c = 0, or a texel whose centre is the focus, gives sx = x exactly and, the taps being finite, the sanitised texel itself.
//
// The window of a 32 x 8 workgroup.  Write s(x) for cab_pos(x, f, k) as fp32 evaluates it, |k| <= 1/16, 0 <= f <= n <= 16384.
//  * Roundings.  (float)x and x + 0.5 are exact (15 bits and a half).  d = (x + 0.5) - f has |d| <= 16384, so its rounding is at most
//    2^-11 (half an ulp below 2^14); p = d k has |p| <= 1024 + 2^-15, rounding at most 2^-14; s = x + p has |s| < 32768, rounding at most
//    2^-10.  Against the real value x + (x + 0.5 - f) k that is |error| <= 2^-11 / 16 + 2^-14 + 2^-10 < 1.1e-3 texel.
//  * s is non-decreasing in x.  Rounding is monotone, so d is non-decreasing in x and p is monotone in d.  For k >= 0 both terms of
//    x + p are non-decreasing.  For k < 0 one step of x raises d by at most 1 + 2^-10, so lowers p by at most (1 + 2^-10) / 16 + 2^-13
//    < 0.063, while x rises by 1: the exact sum rises by more than 0.93 and its rounding keeps the order.
//  * So over the texels x0 .. x0 + m of a tile the first taps floor(s) lie between floor(s(x0)) and floor(s(x0 + m)), and
//    s(x0 + m) - s(x0) <= m (1 + 1/16) + 2 * 1.1e-3: 32.9397 for m = 31 and 7.4397 for m = 7, below 33 and 8.  floor(b) - floor(a) <
//    b - a + 1, so the first taps span at most 34 columns (9 rows) from floor(s(x0)) and, with the second tap one further, a tile
//    touches kCabWinW = 35 columns and kCabWinH = 10 rows: ceil(31 * 17/16) + 2 and ceil(7 * 17/16) + 2.
//  * Clamping.  A tap index i is clamped into the image before it is read: c(i) = min(max(i, 0), n - 1), which is monotone, so the
//    clamped taps of a tile lie in [c(o), c(o + 34)] with o = floor(s(x0)), and c(o + 34) <= c(o) + 34.  The window origin is therefore
//    c(o) = cab_origin(x0, ...) -- made with the same cab_pos the lanes use -- and entry l of the window holds texel min(c(o) + l, n - 1).
//    Every clamped tap then finds its own texel at index c(i) - c(o) in [0, 34], wherever the unclamped window lies.
#pragma once

#include "pt_upscale.h"

namespace pt {

constexpr uint32_t kCabMaxSize = 16384;
constexpr float kCabMaxOffset = 0.0625f;  // |k_c| <= 1/16: what keeps the window above small; a 120-texel fringe at 3840 x 2160
constexpr float kCabDefaultFocus = 0.5f;
// A recollection of the defaults of upstream's later revision, not read from the reference tree at hand (which has no source for it).
constexpr float kCabDefaultOffsets[3] = { 0.003f, 0.003f, -0.003f };

// Made once per call on the host and passed to the kernel by value.
struct CabConfig {
    float fx, fy;  // FocusUV.x W, FocusUV.y H, each one fp32 product
    float k[3];    // Offsets
};

PT_HD CabConfig cab_config(uint32_t w, uint32_t h, const float* focus_uv, const float* offsets)
{
    CabConfig k;
    k.fx = focus_uv[0] * (float)w;
    k.fy = focus_uv[1] * (float)h;
    for (int c = 0; c < 3; c++) k.k[c] = offsets[c];
    return k;
}

constexpr int kCabBlockW = 32, kCabBlockH = 8;
constexpr int kCabWinW = 35, kCabWinH = 10, kCabPlane = kCabWinW * kCabWinH;
static_assert(kCabWinW == (31 * 17 + 15) / 16 + 2 && kCabWinH == (7 * 17 + 15) / 16 + 2, "window = ceil((block - 1) * 17/16) + 2");
static_assert(kCabBlockW == 32 && kCabBlockH == 8, "the window constants are derived for a 32 x 8 workgroup");
static_assert(3 * kCabPlane * sizeof(float) == 4200, "three planes of 35 x 10 floats");

// The sanitised scalars of one channel the taps are read from: the texels [x0, x0 + ...) x [y0, y0 + ...) with `stride` floats per row.
// The kernel's is its workgroup's window in LDS (origin cab_origin), the host shim's the whole image (origin 0).
struct CabPlane {
    const float* v;
    int x0, y0, stride;
};
struct CabWindow {
    CabPlane c[3];
};

PT_HD int cab_clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the sample position of coordinate x along an axis with focus f (in texels) and offset k
PT_HD float cab_pos(int x, float f, float k)
{
    const float xf = (float)x;
    return xf + ((xf + 0.5f) - f) * k;
}

// the two taps of one axis, clamped into [0, n), and the weight of the second
struct CabTaps {
    int i0, i1;
    float t;
};

PT_HD CabTaps cab_taps(int x, float f, float k, int n)
{
    const float s = cab_pos(x, f, k), fl = pt_floor(s);
    const int i = (int)fl;
    CabTaps T;
    T.i0 = cab_clamp_index(i, n);
    T.i1 = cab_clamp_index(i + 1, n);
    T.t = s - fl;
    return T;
}

// the origin along one axis of the window of a tile that starts at x0: the first tap of its first texel
PT_HD int cab_origin(int x0, float f, float k, int n) { return cab_clamp_index((int)pt_floor(cab_pos(x0, f, k)), n); }

// channel ch of texel (x, y) of a w x h image
PT_HD float cab_channel(const CabConfig& k, const CabPlane& P, int ch, int x, int y, int w, int h)
{
    const CabTaps X = cab_taps(x, k.fx, k.k[ch], w), Y = cab_taps(y, k.fy, k.k[ch], h);
    const float* r0 = P.v + (Y.i0 - P.y0) * P.stride;  // (at most 2^28 floats: W, H <= 16384)
    const float* r1 = P.v + (Y.i1 - P.y0) * P.stride;
    const int j0 = X.i0 - P.x0, j1 = X.i1 - P.x0;
    const float a = r0[j0], b = r0[j1], c = r1[j0], d = r1[j1];
    const float ux = 1.0f - X.t, uy = 1.0f - Y.t;
    return (a * ux + b * X.t) * uy + (c * ux + d * X.t) * Y.t;
}

// texel (x, y): the three channels from their planes; alpha is the bits of the texel's own
PT_HD float4 cab_pixel(const CabConfig& k, const CabWindow& W, float alpha, int x, int y, int w, int h)
{
    return up_f4(cab_channel(k, W.c[0], 0, x, y, w, h), cab_channel(k, W.c[1], 1, x, y, w, h), cab_channel(k, W.c[2], 2, x, y, w, h), alpha);
}

#if defined(__HIPCC__)
// pt_chromab.hip: one launch on `stream`
hipError_t launch_chromab(const float4* color, float4* out, uint32_t w, uint32_t h, const CabConfig& k, hipStream_t stream);
#endif

}  // namespace pt
