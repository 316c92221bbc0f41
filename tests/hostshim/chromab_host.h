// chromab_host.h -- TEST SHIM: the two host paths over csrc/pt_chromab.h that chromab_host.cpp exports and tests/cpp/chromab_sanitize.cpp
// runs under the sanitizers.  The caller owns every buffer.  Not part of the product.
#pragma once

#include <cstdint>
#include <initializer_list>
#include <vector>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_chromab.h"

// What a workgroup of pt_chromab.hip stages for its windows, here for the whole image: planes = 3 * w * h floats.
inline void chromab_frame(int w, int h, const pt::CabConfig& k, const float4* color, float4* out, float* planes)
{
    const size_t n = (size_t)w * h;
    const float* scalars = reinterpret_cast<const float*>(color);
    pt::CabWindow W;
    for (int ch = 0; ch < 3; ch++) {
        float* p = planes + ch * n;
        for (size_t i = 0; i < n; i++) p[i] = pt::up_sanitize(scalars[i * 4 + ch]);
        W.c[ch].v = p; W.c[ch].x0 = 0; W.c[ch].y0 = 0; W.c[ch].stride = w;
    }
    for (int py = 0; py < h; py++)  // what each lane does
        for (int px = 0; px < w; px++) {
            const size_t o = (size_t)py * w + px;
            out[o] = pt::cab_pixel(k, W, scalars[o * 4 + 3], px, py, w, h);
        }
}

inline void chromab_frame(int w, int h, const pt::CabConfig& k, const float4* color, float4* out)
{
    std::vector<float> planes(3 * (size_t)w * h);
    chromab_frame(w, h, k, color, out, planes.data());
}

// The call the way pt_chromab.hip runs it: per 32 x 8 block, three kCabWinW x kCabWinH windows (window = 3 * kCabPlane floats) staged
// from cab_origin with the kernel's own index arithmetic, then the block's texels through cab_pixel.  Before a texel is evaluated its
// clamped taps are checked against the window of their channel: -> the number of tap indices outside; such a texel is written as 0.
inline uint64_t chromab_frame_tiled(int w, int h, const pt::CabConfig& k, const float4* color, float4* out, float* window)
{
    using namespace pt;
    const float* scalars = reinterpret_cast<const float*>(color);
    uint64_t outside = 0;
    for (int Y0 = 0; Y0 < h; Y0 += kCabBlockH)
        for (int X0 = 0; X0 < w; X0 += kCabBlockW) {
            int ox[3], oy[3];
            CabWindow W;
            for (int ch = 0; ch < 3; ch++) {
                ox[ch] = cab_origin(X0, k.fx, k.k[ch], w);
                oy[ch] = cab_origin(Y0, k.fy, k.k[ch], h);
                W.c[ch].v = window + ch * kCabPlane; W.c[ch].x0 = ox[ch]; W.c[ch].y0 = oy[ch]; W.c[ch].stride = kCabWinW;
            }
            for (int i = 0; i < 3 * kCabPlane; i++) {
                const int ch = i / kCabPlane, r = i - ch * kCabPlane;
                const int ly = r / kCabWinW, lx = r - ly * kCabWinW;
                const int gx = cab_clamp_index(ox[ch] + lx, w), gy = cab_clamp_index(oy[ch] + ly, h);
                window[i] = up_sanitize(scalars[((size_t)gy * w + gx) * 4 + ch]);
            }
            for (int py = Y0; py < Y0 + kCabBlockH && py < h; py++)
                for (int px = X0; px < X0 + kCabBlockW && px < w; px++) {
                    uint64_t bad = 0;
                    for (int ch = 0; ch < 3; ch++) {
                        const CabTaps X = cab_taps(px, k.fx, k.k[ch], w), Y = cab_taps(py, k.fy, k.k[ch], h);
                        for (const int i : { X.i0, X.i1 }) bad += (i - ox[ch] < 0 || i - ox[ch] >= kCabWinW) ? 1u : 0u;
                        for (const int i : { Y.i0, Y.i1 }) bad += (i - oy[ch] < 0 || i - oy[ch] >= kCabWinH) ? 1u : 0u;
                    }
                    const size_t o = (size_t)py * w + px;
                    outside += bad;
                    out[o] = bad ? up_f4(0.0f, 0.0f, 0.0f, 0.0f) : cab_pixel(k, W, scalars[o * 4 + 3], px, py, w, h);
                }
        }
    return outside;
}

inline uint64_t chromab_frame_tiled(int w, int h, const pt::CabConfig& k, const float4* color, float4* out)
{
    std::vector<float> window(3 * pt::kCabPlane);
    return chromab_frame_tiled(w, h, k, color, out, window.data());
}
