// pt_pixfmt.h -- the texel formats the reference's G-buffer textures have (Source/App.cpp:431-447) and the packed form of the 13 surface
// buffers of row N6 (row N27, DESIGN.md spec S30): 79 bytes per pixel where PtGBuffer's float32 layouts take 128.  The conversions are
// this project's own and frozen in S30 -- nothing in the reference tree pins D3D's rules, so no parity with a D3D device is claimed.
// Everything compiles on the device (pt_gbuffer_packed.hip, pt_gbframe.hip) and as host C++ (the bit-parity tests):
//   half_encode / half_decode       R16_FLOAT: round to nearest even, |x| >= 65520 -> inf, NaN -> sign | 0x7E00, subnormals kept, -0 kept;
//                                   in integer arithmetic, so host and device agree by construction
//   unorm8_encode / unorm8_decode   R8_UNORM: NaN and x <= 0 -> 0, x >= 1 -> 255, else uint(x * 255 + 0.5) (a product, then a sum)
//   snorm16_encode / snorm16_decode R16_SNORM: NaN -> 0, clamp to [-1, 1], s = x * 32767, int(s + (s >= 0 ? 0.5 : -0.5)); max(q / 32767, -1)
//   gbp_pack_* / gbp_unpack_*       a channel of GBufferPixel to its texel and back
#pragma once

#include "pt_gbuffer.h"

namespace pt {

// ---------------------------------------------------------------- scalar formats
PT_HD uint32_t half_encode(float x)
{
    const uint32_t u = as_uint(x);
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return sign | 0x7E00u;   // NaN
    if (a >= 0x477FF000u) return sign | 0x7C00u;  // |x| >= 65520: the halfway point above 65504 rounds to the even neighbour, infinity
    if (a >= 0x38800000u) {                       // |x| >= 2^-14: a normal half; the carry of the rounding runs into the exponent
        const uint32_t m = a - 0x38000000u;
        return sign | ((m + 0xFFFu + ((m >> 13) & 1u)) >> 13);
    }
    // a subnormal half: |x| * 2^24 rounded to an integer, ties to even
    const uint32_t e = a >> 23;
    if (e < 102u) return sign;                    // |x| < 2^-25: below half of the smallest subnormal
    const uint32_t mant = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;  // 14 .. 24
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (q & 1u))) q++;
    return sign | q;
}

PT_HD float half_decode(uint32_t h)
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return as_float(sign | 0x7F800000u | (m << 13));
    if (e == 0u) return as_float(as_uint((float)m * 5.9604644775390625e-08f) | sign);  // m * 2^-24, exact
    return as_float(sign | ((e + 112u) << 23) | (m << 13));
}

PT_HD uint32_t unorm8_encode(float x)
{
    if (!(x > 0.0f)) return 0u;
    if (x >= 1.0f) return 255u;
    const float p = x * 255.0f;
    return (uint32_t)(p + 0.5f);
}

PT_HD float unorm8_decode(uint32_t q) { return (float)q / 255.0f; }

PT_HD uint32_t snorm16_encode(float x)  // -> the 16 bits of the two's-complement value
{
    if (x != x) return 0u;
    x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
    const float s = x * 32767.0f;
    const int32_t q = (int32_t)(s + (s >= 0.0f ? 0.5f : -0.5f));
    return (uint32_t)q & 0xFFFFu;
}

PT_HD float snorm16_decode(uint32_t q)
{
    const int32_t v = (int32_t)(q << 16) >> 16;
    return pt_max((float)v / 32767.0f, -1.0f);
}

// ---------------------------------------------------------------- texels
// R16G16B16A16: x in the low 16 bits of the first dword (little-endian memory order x, y, z, w)
PT_HD uint64_t pix_half4(float x, float y, float z, float w)
{
    return (uint64_t)(half_encode(x) | (half_encode(y) << 16)) | ((uint64_t)(half_encode(z) | (half_encode(w) << 16)) << 32);
}
PT_HD uint64_t pix_snorm16x4(float x, float y, float z, float w)
{
    return (uint64_t)(snorm16_encode(x) | (snorm16_encode(y) << 16)) | ((uint64_t)(snorm16_encode(z) | (snorm16_encode(w) << 16)) << 32);
}
PT_HD uint32_t pix_snorm16x2(float x, float y) { return snorm16_encode(x) | (snorm16_encode(y) << 16); }
PT_HD uint32_t pix_unorm8x4(float x, float y, float z, float w)
{
    return unorm8_encode(x) | (unorm8_encode(y) << 8) | (unorm8_encode(z) << 16) | (unorm8_encode(w) << 24);
}

// The packed buffers, in PtGBufferPacked's (= PtGBuffer's) order; bytes per texel 16, 4, 4, 4, 4, 8, 4, 8, 8, 8, 2, 1, 8 = 79
struct GBufferPackedOut {
    float4* Position;              // R32G32B32A32_FLOAT
    uint32_t* FlatNormal;          // R16G16_SNORM
    uint32_t* GeometricNormal;     // R16G16_SNORM
    float* LinearDepth;            // R32_FLOAT
    float* NormalizedDepth;        // R32_FLOAT
    uint64_t* MotionVector;        // R16G16B16A16_FLOAT, w = 0
    uint32_t* BaseColorMetalness;  // R8G8B8A8_UNORM
    uint64_t* DiffuseAlbedo;       // R16G16B16A16_FLOAT, w = 0
    uint64_t* SpecularAlbedo;      // R16G16B16A16_FLOAT, w = 0
    uint64_t* NormalRoughness;     // R16G16B16A16_SNORM
    uint16_t* IOR;                 // R16_FLOAT
    uint8_t* Transmission;         // R8_UNORM
    uint64_t* Radiance;            // R16G16B16A16_FLOAT, w = 1
};
constexpr uint32_t kGbPackedTexelBytes[13] = { 16, 4, 4, 4, 4, 8, 4, 8, 8, 8, 2, 1, 8 };

PT_HD uint32_t gbp_pack_normal(f2 e) { return pix_snorm16x2(e.x, e.y); }
PT_HD uint64_t gbp_pack_motion(f3 v) { return pix_half4(v.x, v.y, v.z, 0.0f); }
PT_HD uint32_t gbp_pack_base_color_metalness(float4 v) { return pix_unorm8x4(v.x, v.y, v.z, v.w); }
PT_HD uint64_t gbp_pack_albedo(f3 v) { return pix_half4(v.x, v.y, v.z, 0.0f); }
PT_HD uint64_t gbp_pack_normal_roughness(float4 v) { return pix_snorm16x4(v.x, v.y, v.z, v.w); }
PT_HD uint16_t gbp_pack_ior(float v) { return (uint16_t)half_encode(v); }
PT_HD uint8_t gbp_pack_transmission(float v) { return (uint8_t)unorm8_encode(v); }
PT_HD uint64_t gbp_pack_radiance(f3 v) { return pix_half4(v.x, v.y, v.z, 1.0f); }

PT_HD f2 gbp_unpack_normal(uint32_t q) { f2 e; e.x = snorm16_decode(q & 0xFFFFu); e.y = snorm16_decode(q >> 16); return e; }
PT_HD float4 gbp_unpack_base_color_metalness(uint32_t q)
{
    return gb_float4(unorm8_decode(q & 255u), unorm8_decode((q >> 8) & 255u), unorm8_decode((q >> 16) & 255u), unorm8_decode(q >> 24));
}
PT_HD float4 gbp_unpack_normal_roughness(uint64_t q)
{
    const uint32_t lo = (uint32_t)q, hi = (uint32_t)(q >> 32);
    return gb_float4(snorm16_decode(lo & 0xFFFFu), snorm16_decode(lo >> 16), snorm16_decode(hi & 0xFFFFu), snorm16_decode(hi >> 16));
}
PT_HD float gbp_unpack_ior(uint16_t q) { return half_decode(q); }
PT_HD float gbp_unpack_transmission(uint8_t q) { return unorm8_decode(q); }
PT_HD f3 gbp_unpack_radiance(uint64_t q)
{
    const uint32_t lo = (uint32_t)q, hi = (uint32_t)(q >> 32);
    return make_f3(half_decode(lo & 0xFFFFu), half_decode(lo >> 16), half_decode(hi & 0xFFFFu));
}

#if defined(__HIPCC__)
struct SceneView;
struct PixelMap;
// pt_render_gbuffer_packed (pt_gbuffer_packed.hip): launch_gbuffer's pass, stored through the packers.  One launch on `stream`.
hipError_t launch_gbuffer_packed(const SceneView& sv, const PixelMap& pm, const GBufferFrame& fr, const GBufferScene& sc, const GBufferPackedOut& out, uint32_t want,
                                 uint32_t grid, hipStream_t stream);
#endif

}  // namespace pt
