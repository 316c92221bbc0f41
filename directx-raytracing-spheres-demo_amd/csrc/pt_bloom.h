// pt_bloom.h -- bloom (row N5): PostProcessing::Bloom and ::Merge (Source/Bloom.ixx, Shaders/Bloom.hlsl, Source/Merge.ixx,
// Shaders/Merge.hlsl), as device functions that also compile on the host (tests/hostshim/bloom_host.cpp).  These functions
// are the whole spec (DESIGN.md spec S11); the kernels of pt_bloom.hip and the CPU shim only call them.
//
// The chain: two half-size textures of 5 mips ping-pong, one mip written per dispatch (Bloom.ixx:71-125):
//   1 input -> A.0 (Karis)   2 A.0 -> B.1 (Karis)   3 B.1 -> A.2   4 A.2 -> B.3   5 B.3 -> A.4        (downsample)
//   6 A.4 -> B.3             7 B.3 -> A.2           8 A.2 -> B.1   9 B.1 -> A.0                       (upsample, overwrites)
//   merge: out = input * (1 - Strength) + A.0 * Strength
// Every mip level lives in exactly one of the two textures, so here they are one chain of 5 levels in one allocation
// (BloomChain): an upsample overwrites the level that the downsample wrote, which has already been read.
//
// Sampling is SampleLevel(linear, clamp) at an integer level = sample_bilinear_clamp on that level's own TexView.  A tap is
// `uv + g_size * k`, written as a multiply then an add; g_size * k is exact for every k used, so that is one rounding.
// Radiance and the chain are fp32 (the reference's are R16G16B16A16_FLOAT).  Only RGB is filtered; a chain texel's w is 0.
#pragma once

#include "pt_texture.h"
#include "pt_post.h"

namespace pt {

constexpr uint32_t kBloomMips = 5;                  // Bloom::BlurMipLevels
constexpr uint32_t kBloomMinSize = 32;              // W, H >= 32: every level of the half-size chain is >= 1 texel
constexpr float kBloomUpsampleRadius = 5e-3f;       // UpsamplingFilterRadius, in UV units on both axes

struct u2 { uint32_t x, y; };

// The chain of a W x H input: level k is max(1, (W/2) >> k) x max(1, (H/2) >> k) texels at texel offset off[k].
struct BloomChain {
    uint32_t w[kBloomMips], h[kBloomMips];
    uint64_t off[kBloomMips];
    uint64_t texels;  // all levels
};

PT_HD BloomChain bloom_chain(uint32_t width, uint32_t height)
{
    BloomChain c;
    uint64_t o = 0;
    for (uint32_t k = 0; k < kBloomMips; k++) {
        const uint32_t w = (width / 2u) >> k, h = (height / 2u) >> k;
        c.w[k] = w ? w : 1u;
        c.h[k] = h ? h : 1u;
        c.off[k] = o;
        o += (uint64_t)c.w[k] * c.h[k];
    }
    c.texels = o;
    return c;
}

// Color::ToSrgb of the un-vendored MathLib (recollection, build-frozen like S6-S8): the IEC 61966-2-1 curve per channel
PT_HD float to_srgb_exact(float x) { return x < 0.0031308f ? 12.92f * x : 1.055f * pow_pos(x, 1.0f / 2.4f) - 0.055f; }

// KarisAverage: 1 / (1 + Luminance(ToSrgb(rgb)) * 0.25), Luminance = the project's luminance (pt_math.h)
PT_HD float karis_weight(f3 c)
{
    return 1.0f / (1.0f + luminance(make_f3(to_srgb_exact(c.x), to_srgb_exact(c.y), to_srgb_exact(c.z))) * 0.25f);
}

// Math::CalculateUV: (p + 0.5) / dims, IEEE divide
PT_HD f2 bloom_uv(u2 dims, u2 p)
{
    f2 uv;
    uv.x = ((float)p.x + 0.5f) / (float)dims.x;
    uv.y = ((float)p.y + 0.5f) / (float)dims.y;
    return uv;
}

PT_HD f3 bloom_tap(const TexView& in, f2 uv, f2 g, float kx, float ky)
{
    f2 t;
    t.x = uv.x + g.x * kx;
    t.y = uv.y + g.y * ky;
    float s[4];
    sample_bilinear_clamp(in, t, s);
    return make_f3(s[0], s[1], s[2]);
}

// Downsample: 13 taps at {-2..2} output texels around p (g_size = 1 / out_dims).  Karis (steps 1 and 2: InputMipLevel == 0)
// weights five groups -- four corner quads * 0.125/4, the inner quad * 0.5/4 -- each by karis_weight, and returns
// max(sum, 1e-4) (pt_max: NaN -> 1e-4, as HLSL max).
PT_HD f3 bloom_downsample_px(const TexView& in, u2 out_dims, u2 p, bool karis)
{
    const f2 uv = bloom_uv(out_dims, p);
    f2 g;
    g.x = 1.0f / (float)out_dims.x;
    g.y = 1.0f / (float)out_dims.y;
    const f3 a = bloom_tap(in, uv, g, -2.f, 2.f), b = bloom_tap(in, uv, g, 0.f, 2.f), c = bloom_tap(in, uv, g, 2.f, 2.f);
    const f3 d = bloom_tap(in, uv, g, -2.f, 0.f), e = bloom_tap(in, uv, g, 0.f, 0.f), f = bloom_tap(in, uv, g, 2.f, 0.f);
    const f3 gg = bloom_tap(in, uv, g, -2.f, -2.f), h = bloom_tap(in, uv, g, 0.f, -2.f), i = bloom_tap(in, uv, g, 2.f, -2.f);
    const f3 j = bloom_tap(in, uv, g, -1.f, 1.f), k = bloom_tap(in, uv, g, 1.f, 1.f);
    const f3 l = bloom_tap(in, uv, g, -1.f, -1.f), m = bloom_tap(in, uv, g, 1.f, -1.f);
    if (!karis)
        return e * 0.125f + (a + c + gg + i) * 0.03125f + (b + d + f + h) * 0.0625f + (j + k + l + m) * 0.125f;
    const float v0 = 0.125f / 4.0f, v1 = 0.5f / 4.0f;
    f3 g0 = (a + b + d + e) * v0, g1 = (b + c + e + f) * v0, g2 = (d + e + gg + h) * v0, g3 = (e + f + h + i) * v0;
    f3 g4 = (j + k + l + m) * v1;
    g0 = g0 * karis_weight(g0);
    g1 = g1 * karis_weight(g1);
    g2 = g2 * karis_weight(g2);
    g3 = g3 * karis_weight(g3);
    g4 = g4 * karis_weight(g4);
    const f3 s = g0 + g1 + g2 + g3 + g4;
    return make_f3(pt_max(s.x, 1e-4f), pt_max(s.y, 1e-4f), pt_max(s.z, 1e-4f));
}

// Upsample: 3x3 tent at +-UpsamplingFilterRadius UV around p: (4e + 2(b+d+f+h) + a+c+g+i) / 16
PT_HD f3 bloom_upsample_px(const TexView& in, u2 out_dims, u2 p)
{
    const f2 uv = bloom_uv(out_dims, p);
    f2 g;
    g.x = kBloomUpsampleRadius;
    g.y = kBloomUpsampleRadius;
    const f3 a = bloom_tap(in, uv, g, -1.f, 1.f), b = bloom_tap(in, uv, g, 0.f, 1.f), c = bloom_tap(in, uv, g, 1.f, 1.f);
    const f3 d = bloom_tap(in, uv, g, -1.f, 0.f), e = bloom_tap(in, uv, g, 0.f, 0.f), f = bloom_tap(in, uv, g, 1.f, 0.f);
    const f3 gg = bloom_tap(in, uv, g, -1.f, -1.f), h = bloom_tap(in, uv, g, 0.f, -1.f), i = bloom_tap(in, uv, g, 1.f, -1.f);
    const f3 r = e * 4.0f + (b + d + f + h) * 2.0f + a + c + gg + i;
    return make_f3(r.x / 16.0f, r.y / 16.0f, r.z / 16.0f);
}

// Merge: input * w1 + SampleLevel(A.0, uv, 0) * w2 with w1 = 1 - Strength, w2 = Strength (products, then the sum).  The
// input is read at the output texel itself (what a hardware filter at an exact texel centre returns); A.0 is a bilinear
// upsample from the half-size level.  Alpha is the input's.
PT_HD float4 bloom_merge_px(float4 in, const TexView& blur0, u2 out_dims, u2 p, float w1, float w2)
{
    float s[4];
    sample_bilinear_clamp(blur0, bloom_uv(out_dims, p), s);
    float4 o;
    o.x = in.x * w1 + s[0] * w2;
    o.y = in.y * w1 + s[1] * w2;
    o.z = in.z * w1 + s[2] * w2;
    o.w = in.w;
    return o;
}

}  // namespace pt
