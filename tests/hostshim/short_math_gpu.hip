// short_math_gpu.hip -- TEST SHIM: pt_math.h's short exact forms (pt_sqrt_ranged, pt_rcp_ranged, pt_half_rcp_ranged) against the compiler's
// expansions (pt_sqrt, pt_rcp, pt_half_rcp), compiled by hipcc for gfx950 with the HIPFLAGS of csrc/Makefile.
//   sm_sweep(counts, first): one launch over all 2^32 bit patterns.  Per function k = 0 (sqrt), 1 (rcp), 2 (half_rcp): counts[k] = operands
//   INSIDE the contract (or +-0, +-inf, NaN) whose results differ, counts[3 + k] = operands outside it whose results differ (reported, not an
//   error), first[k] / first[3 + k] = the smallest such bit pattern.  Two NaNs count as equal.
//   sm_edges(n, in, out): out[6 i ..] = {sqrt_ranged, sqrt, rcp_ranged, rcp, half_rcp_ranged, half_rcp}(in[i]) as bit patterns.
// Both take HOST pointers and return the hipError_t as an int (0 = success).  A thread writes only its own element or the twelve counters.
// Not part of the product; never loaded by it.
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_math.h"

namespace {

__device__ __forceinline__ bool same(float a, float b) { return pt::as_uint(a) == pt::as_uint(b) || (a != a && b != b); }
__device__ __forceinline__ bool special(uint32_t mag) { return mag == 0u || mag >= 0x7F800000u; }  // +-0, +-inf, NaN

// the contracts of pt_math.h, on the magnitude's bit pattern (2^e is (e + 127) << 23)
constexpr uint32_t kTwoM96 = (127u - 96u) << 23, kTwoM126 = 1u << 23, kTwo126 = 253u << 23, kTwo125 = 252u << 23;
__device__ __forceinline__ bool in_sqrt(uint32_t mag) { return special(mag) || mag >= kTwoM96; }
__device__ __forceinline__ bool in_rcp(uint32_t mag) { return special(mag) || (mag >= kTwoM126 && mag <= kTwo126); }
__device__ __forceinline__ bool in_half(uint32_t mag) { return special(mag) || (mag >= kTwoM126 && mag <= kTwo125); }

__global__ void sweep_kernel(unsigned long long* __restrict__ counts, uint32_t* __restrict__ first)
{
    unsigned long long n[6] = { 0, 0, 0, 0, 0, 0 };
    uint32_t f[6] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const uint32_t u = (uint32_t)i, mag = u & 0x7FFFFFFFu;
        const float x = pt::as_float(u);
        const bool bad[3] = { !same(pt::pt_sqrt_ranged(x), pt::pt_sqrt(x)), !same(pt::pt_rcp_ranged(x), pt::pt_rcp(x)),
                              !same(pt::pt_half_rcp_ranged(x), pt::pt_half_rcp(x)) };
        const bool in[3] = { in_sqrt(mag), in_rcp(mag), in_half(mag) };
        for (int k = 0; k < 3; k++)
            if (bad[k]) { const int j = in[k] ? k : 3 + k; n[j]++; f[j] = u < f[j] ? u : f[j]; }
    }
    for (int j = 0; j < 6; j++)
        if (n[j]) { atomicAdd(&counts[j], n[j]); atomicMin(&first[j], f[j]); }
}

__global__ void edges_kernel(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = pt::as_float(in[i]);
    uint32_t* o = out + (size_t)i * 6u;
    o[0] = pt::as_uint(pt::pt_sqrt_ranged(x)); o[1] = pt::as_uint(pt::pt_sqrt(x));
    o[2] = pt::as_uint(pt::pt_rcp_ranged(x)); o[3] = pt::as_uint(pt::pt_rcp(x));
    o[4] = pt::as_uint(pt::pt_half_rcp_ranged(x)); o[5] = pt::as_uint(pt::pt_half_rcp(x));
}

}  // namespace

extern "C" {

int sm_sweep(unsigned long long* counts, uint32_t* first)
{
    if (counts == nullptr || first == nullptr) return (int)hipErrorInvalidValue;
    unsigned long long* d_counts = nullptr;
    uint32_t* d_first = nullptr;
    hipError_t e = hipMalloc(&d_counts, 6 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&d_first, 6 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_counts, 0, 6 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_first, 0xFF, 6 * sizeof(uint32_t));
    if (e == hipSuccess) {
        sweep_kernel<<<256 * 32, 256>>>(d_counts, d_first);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(counts, d_counts, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first, d_first, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_counts); (void)hipFree(d_first);
    return (int)e;
}

int sm_edges(uint32_t n, const uint32_t* in, uint32_t* out)
{
    if (n == 0) return 0;
    if (in == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    const size_t in_bytes = (size_t)n * sizeof(uint32_t), out_bytes = in_bytes * 6u;
    hipError_t e = hipMalloc(&d_in, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        edges_kernel<<<(n + 255u) / 256u, 256>>>(n, d_in, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_out);
    return (int)e;
}

}
