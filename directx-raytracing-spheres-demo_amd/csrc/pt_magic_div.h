// pt_magic_div.h -- exact unsigned division by a launch-invariant divisor: one multiply-high and one shift, the pair made on the host.
// No HIP types: the host side (pt_api.hip), the kernels (pt_pixel_map.h) and the host-compiled tests share this file.
//
// For a divisor d >= 1 that is no power of two let s = ceil(log2 d) - 1 (so 2^s < d < 2^(s+1)), k = 32 + s, mul = ceil(2^k / d).
//   mul < 2^32, because 2^k / d < 2^32 (2^s < d) and d does not divide 2^k.
//   With e = mul * d - 2^k (0 < e < d):  n * mul / 2^k = n / d + n * e / (d * 2^k), and floor() of it is floor(n / d) as long as the
//   excess stays below the 1 / d that separates n / d from the next integer: n * e < 2^k.
//   2^k = 2^32 * 2^s >= 2^31 * d > n * e for every n < 2^31, so the pair is exact for all n below 2^31 whatever d is.
//   floor(n * mul / 2^k) = umulhi(n, mul) >> s.
// A power of two (d = 1 included) would need mul = 2^32; it is kept as mul = 0 and means the plain shift n >> shift.
#pragma once

#include <stdint.h>
#include <cstdio>
#include <cstdlib>

#if defined(__HIPCC__)
#define PT_MD __host__ __device__ __forceinline__
#else
#define PT_MD inline
#endif

namespace pt {

struct MagicDiv {
    uint32_t mul;    // 0: the divisor is 1 << shift
    uint32_t shift;
};

// n / d for the pair made from d; exact for every n below the bound the pair was made for
PT_MD uint32_t magic_div(uint32_t n, MagicDiv m)
{
    const uint32_t hi = (uint32_t)(((uint64_t)n * m.mul) >> 32);  // (v_mul_hi_u32, or s_mul_hi_u32 for a wave-uniform n)
    return (m.mul == 0u ? n : hi) >> m.shift;
}

constexpr uint32_t kMagicDivBound = 1u << 31;  // the largest exclusive bound a pair can be made for

// The pair for d (>= 1; 0 is taken as 1: a map that never divides by it), exact for every n < n_max (<= 2^31).  The inequality above is
// checked for the pair that is returned, whatever the argument that leads to it: a pair that failed it would map pixels wrongly, so the
// process stops here.
inline MagicDiv make_magic_div(uint32_t d, uint32_t n_max = kMagicDivBound)
{
    if (d == 0u) d = 1u;
    MagicDiv m{ 0u, 0u };
    if ((d & (d - 1u)) == 0u) {
        while ((1u << m.shift) != d) m.shift++;
        return m;
    }
    uint32_t s = 0;
    while ((2ull << s) < d) s++;  // 2^s < d < 2^(s + 1)
    const uint64_t two_k = 1ull << (32u + s);
    const uint64_t mul = (two_k + d - 1u) / d;
    const uint64_t e = mul * d - two_k;
    const bool ok = n_max >= 1u && n_max <= kMagicDivBound && mul < (1ull << 32) && e < d && (uint64_t)(n_max - 1u) * e < two_k;
    if (!ok) {
        std::fprintf(stderr, "make_magic_div: no exact pair for d = %u below %u\n", d, n_max);
        std::abort();
    }
    m.mul = (uint32_t)mul;
    m.shift = s;
    return m;
}

}  // namespace pt
