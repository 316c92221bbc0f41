// pt_nis.h -- the sharpening stand-in (row N12): a directional unsharp mask in the form of NVIDIA Image Scaling's sharpen pass
// (NVSharpen), which App::ProcessNIS evaluates through Streamline between the upscaler and bloom (Source/App.cpp:1710-1721; the NIS
// plugin is not vendored).  The arithmetic is a recollection of the published NIS v1 shader, frozen by DESIGN.md spec S18.
// Per-pixel functions for the kernel of pt_nis.hip; they also compile as host C++ (tests/hostshim/nis_host.cpp), so the GPU output is
// pinned bit for bit to the host-compiled header.  fp32 throughout, no contraction (-ffp-contract=off), no fma anywhere.
#pragma once

#include "pt_upscale.h"

namespace pt {

constexpr uint32_t kNisMaxSize = 16384;
constexpr uint32_t kNisHdrNone = 0, kNisHdrLinear = 1, kNisHdrPQ = 2;  // sl::NISHDR; PQ is not built
constexpr float kNisDefaultSharpness = 0.5f;                          // PostProcessing.NIS.Sharpness (Source/MyAppData.h:297-303)
constexpr float kNisK = 0.282842712f;                                 // Linear mode: Y = sqrt(Y) * K
constexpr float kNisMaxColor = kUpMaxRadiance;                        // step 1 and step 6: 65504

// The values of spec S18's tables, made once per call on the host and passed to the kernel by value.
struct NisConfig {
    float detect_ratio, detect_thres;
    float min_contrast_ratio, ratio_norm;
    float sharp_start_y, scale_y;
    float strength_min, strength_scale;
    float limit_min, limit_scale, limit_max;
    float eps;
};

PT_HD NisConfig nis_config(float sharpness, uint32_t hdr_mode)
{
    const bool lin = hdr_mode == kNisHdrLinear;
    const float s = sharpness - 0.5f;
    const float max_scale = s >= 0.0f ? 1.25f : 1.75f;
    const float min_scale = s >= 0.0f ? 1.25f : 1.0f;
    const float limit_scale = s >= 0.0f ? 1.25f : 1.0f;
    NisConfig k;
    k.detect_ratio = 2.0f * 1127.0f / 1024.0f;
    k.detect_thres = (lin ? 32.0f : 64.0f) / 1024.0f;
    k.min_contrast_ratio = lin ? 1.5f : 2.0f;
    const float max_contrast_ratio = lin ? 5.0f : 10.0f;
    k.ratio_norm = 1.0f / (max_contrast_ratio - k.min_contrast_ratio);
    k.sharp_start_y = lin ? 0.35f : 0.45f;
    const float sharp_end_y = lin ? 0.55f : 0.9f;
    k.scale_y = 1.0f / (sharp_end_y - k.sharp_start_y);
    k.strength_min = pt_max(0.0f, 0.4f + s * min_scale * (lin ? 1.1f : 1.2f));
    const float strength_max = (lin ? 2.2f : 1.6f) + s * max_scale * 1.8f;
    k.strength_scale = strength_max - k.strength_min;
    k.limit_min = lin ? pt_max(0.06f, 0.10f + s * limit_scale * 0.28f) : pt_max(0.1f, 0.14f + s * limit_scale * 0.32f);
    k.limit_max = (lin ? 0.6f : 0.5f) + s * limit_scale * 0.6f;
    k.limit_scale = k.limit_max - k.limit_min;
    k.eps = lin ? 1e-4f * kNisK * kNisK : 1.0f / 255.0f;
    return k;
}

// The staged lumas the patch is read from: Y of the texels [x0, x0 + ...) x [y0, y0 + ...) with `stride` floats per row.  The kernel's
// is its workgroup's footprint in LDS, the host shim's the whole image.
struct NisTile {
    const float* y;
    int x0, y0, stride;
};

// The 36 x 12 footprint of a 32 x 8 workgroup of pt_nis.hip: two texels either side.  Its origin may lie outside the image; entry
// (lx, ly) holds the luma of the texel (x0 + lx, y0 + ly) clamped into the image, so a patch coordinate clamped into the image, which
// lies within two texels of its lane, always finds its own texel there.
constexpr int kNisBlockW = 32, kNisBlockH = 8, kNisBorder = 2;
constexpr int kNisTileW = kNisBlockW + 2 * kNisBorder, kNisTileH = kNisBlockH + 2 * kNisBorder;

PT_HD int nis_clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
PT_HD float nis_min3(float a, float b, float c) { return pt_min(pt_min(a, b), c); }

// step 1, once per texel: the luma of the sanitised colour
template <uint32_t kHdr>
PT_HD float nis_luma(float4 c)
{
    const float r = up_sanitize(c.x), g = up_sanitize(c.y), b = up_sanitize(c.z);
    const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    return kHdr == kNisHdrLinear ? pt_sqrt(y) * kNisK : y;
}

// step 5: the limited unsharp mask of one five-tap line, scaled down where the contrast either side of the centre is lopsided
PT_HD float nis_line_usm(const NisConfig& k, float y0, float y1, float y2, float y3, float y4, float strength, float limit)
{
    float u = ((-0.6001f * y1 + 1.2002f * y2) - 0.6001f * y3) * strength;
    u = pt_min(limit, pt_max(-limit, u));
    const float ac = up_max3(y0, y1, y2) - nis_min3(y0, y1, y2);
    const float bc = up_max3(y2, y3, y4) - nis_min3(y2, y3, y4);
    const float r = pt_max(ac, bc) / (pt_min(ac, bc) + k.eps);
    return u * (1.0f - saturate((r - k.min_contrast_ratio) * k.ratio_norm));
}

// steps 2-5 of texel (x, y) of a w x h image: the sum of the four directions' unsharp masks
PT_HD float nis_usm(const NisConfig& k, const NisTile& T, int x, int y, int w, int h)
{
    // step 2: the 5 x 5 patch, coordinates clamped into the image
    float p[5][5];
    int col[5];
    for (int j = 0; j < 5; j++) col[j] = nis_clamp_index(x + j - 2, w) - T.x0;
    for (int i = 0; i < 5; i++) {
        const float* row = T.y + (nis_clamp_index(y + i - 2, h) - T.y0) * T.stride;
        for (int j = 0; j < 5; j++) p[i][j] = row[col[j]];
    }
    // step 3: the edge map on the inner 3 x 3
    const float q00 = p[1][1], q01 = p[1][2], q02 = p[1][3];
    const float q10 = p[2][1], q12 = p[2][3];
    const float q20 = p[3][1], q21 = p[3][2], q22 = p[3][3];
    const float g0 = pt_abs(((q00 + q01) + q02) - ((q20 + q21) + q22));
    const float g45 = pt_abs(((q10 + q00) + q01) - ((q21 + q22) + q12));
    const float g90 = pt_abs(((q00 + q10) + q20) - ((q02 + q12) + q22));
    const float g135 = pt_abs(((q10 + q20) + q21) - ((q01 + q02) + q12));
    const float A = pt_max(g0, g90), a = pt_min(g0, g90), B = pt_max(g45, g135), b = pt_min(g45, g135);
    float w0 = 0.0f, w90 = 0.0f, w45 = 0.0f, w135 = 0.0f;
    if (A + B != 0.0f) {
        const float e = pt_min(A / (A + B), 1.0f);
        const bool cA = A > a * k.detect_ratio && A > k.detect_thres && A > b;
        const bool cB = B > b * k.detect_ratio && B > k.detect_thres && B > a;
        const float fA = (cA && cB) ? e : 1.0f, fB = (cA && cB) ? 1.0f - e : 1.0f;
        w0 = (cA && A == g0) ? fA : 0.0f;
        w90 = (cA && A != g0) ? fA : 0.0f;
        w45 = (cB && B == g45) ? fB : 0.0f;
        w135 = (cB && B != g45) ? fB : 0.0f;
    }
    // step 4: strength and limit at the centre
    const float yc = p[2][2];
    const float t = 1.0f - saturate((yc - k.sharp_start_y) * k.scale_y);
    const float strength = t * k.strength_scale + k.strength_min;
    const float limit = (t * k.limit_scale + k.limit_min) * yc;
    // step 5: 0 deg = the column through the centre, 90 deg = its row, 45 and 135 deg = the diagonals
    const float u0 = nis_line_usm(k, p[0][2], p[1][2], p[2][2], p[3][2], p[4][2], strength, limit);
    const float u90 = nis_line_usm(k, p[2][0], p[2][1], p[2][2], p[2][3], p[2][4], strength, limit);
    const float u45 = nis_line_usm(k, p[4][0], p[3][1], p[2][2], p[1][3], p[0][4], strength, limit);
    const float u135 = nis_line_usm(k, p[0][0], p[1][1], p[2][2], p[3][3], p[4][4], strength, limit);
    return ((w0 * u0 + w90 * u90) + w45 * u45) + w135 * u135;
}

// step 6: the texel's colour c with its luma yc and the sum of step 5 -> the output texel; alpha passes through
template <uint32_t kHdr>
PT_HD float4 nis_output(const NisConfig& k, float4 c, float yc, float usm)
{
    const float r = up_sanitize(c.x), g = up_sanitize(c.y), b = up_sanitize(c.z);
    if (kHdr == kNisHdrLinear) {
        const float yn = pt_max(yc + usm, 0.0f);
        const float corr = (yn * yn + k.eps) / (yc * yc + k.eps);
        return up_f4(pt_min(r * corr, kNisMaxColor), pt_min(g * corr, kNisMaxColor), pt_min(b * corr, kNisMaxColor), c.w);
    }
    return up_f4(pt_max(r + usm, 0.0f), pt_max(g + usm, 0.0f), pt_max(b + usm, 0.0f), c.w);
}

// texel (x, y): steps 2-6 on the staged lumas T and the texel's own colour
template <uint32_t kHdr>
PT_HD float4 nis_pixel(const NisConfig& k, const NisTile& T, float4 c, int x, int y, int w, int h)
{
    const float usm = nis_usm(k, T, x, y, w, h);
    const float yc = T.y[(y - T.y0) * T.stride + (x - T.x0)];
    return nis_output<kHdr>(k, c, yc, usm);
}

#if defined(__HIPCC__)
// pt_nis.hip: one launch on `stream`
hipError_t launch_nis(const float4* color, float4* out, uint32_t w, uint32_t h, const NisConfig& k, uint32_t hdr_mode, hipStream_t stream);
#endif

}  // namespace pt
