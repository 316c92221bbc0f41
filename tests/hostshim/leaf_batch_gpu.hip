// leaf_batch_gpu.hip -- TEST SHIM: the wrappers of leaf_batch.h compiled by hipcc for gfx950 with the HIPFLAGS of csrc/Makefile, one
// thread per element.  lbg_NAME(n, in, out, aux, aux_words) takes HOST pointers and has the signature of leaf_batch_host.cpp's
// lbh_NAME: it copies in, launches, synchronises, copies out and returns the hipError_t as an int (0 = success).  Nothing in a kernel
// aborts or asserts; a thread reads only its own element's words and the shared table.  Not part of the product; never loaded by it.
#include "leaf_batch.h"

namespace {

using LbFn = void (*)(const float*, float*, const float*);

template <LbFn F, int IN, int OUT>
__global__ void lb_kernel(uint32_t n, const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ aux)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[IN], r[OUT];
    for (int k = 0; k < IN; k++) a[k] = in[(size_t)i * IN + k];
    for (int k = 0; k < OUT; k++) r[k] = 0.0f;
    F(a, r, aux);
    for (int k = 0; k < OUT; k++) out[(size_t)i * OUT + k] = r[k];
}

// the texel table of the samplers (leaf_batch.h aux_texture): every header must describe texels inside the table
bool aux_ok(const float* aux, uint32_t aux_words)
{
    if (aux == nullptr || aux_words == 0) return true;  // (only the samplers read it; the tests always pass one to them)
    if (aux_words < 4 * lb::kAuxTextures) return false;
    for (uint32_t k = 0; k < lb::kAuxTextures; k++) {
        const uint64_t w = pt::as_uint(aux[4 * k]), h = pt::as_uint(aux[4 * k + 1]), first = pt::as_uint(aux[4 * k + 2]);
        if (w == 0 || h == 0 || w > 32767 || h > 32767 || 4 * first < 4 * lb::kAuxTextures || 4 * (first + w * h) > aux_words) return false;
    }
    return true;
}

template <LbFn F, int IN, int OUT, bool kNeedsAux>
int lb_run(uint32_t n, const float* in, float* out, const float* aux, uint32_t aux_words)
{
    if (n == 0) return 0;
    if (in == nullptr || out == nullptr || !aux_ok(aux, aux_words) || (kNeedsAux && (aux == nullptr || aux_words == 0))) return (int)hipErrorInvalidValue;
    float *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
    const size_t in_bytes = (size_t)n * IN * sizeof(float), out_bytes = (size_t)n * OUT * sizeof(float), aux_bytes = (size_t)aux_words * sizeof(float);
    hipError_t e = hipMalloc(&d_in, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
    if (e == hipSuccess && aux_bytes) e = hipMalloc(&d_aux, aux_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && aux_bytes) e = hipMemcpy(d_aux, aux, aux_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const uint32_t block = 256, grid = (n + block - 1) / block;
        lb_kernel<F, IN, OUT><<<grid, block>>>(n, d_in, d_out, d_aux);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_aux);
    return (int)e;
}

constexpr bool str_eq(const char* a, const char* b) { return *a == *b && (*a == 0 || str_eq(a + 1, b + 1)); }
constexpr bool needs_aux(const char* name) { return str_eq(name, "sample_bilinear") || str_eq(name, "sample_bilinear_clamp"); }

}  // namespace

extern "C" {

#define LB_GPU_ENTRY(name, IN, OUT)                                                                               \
    int lbg_##name(uint32_t n, const float* in, float* out, const float* aux, uint32_t aux_words)                 \
    {                                                                                                             \
        return lb_run<lb::lb_##name, IN, OUT, needs_aux(#name)>(n, in, out, aux, aux_words);                      \
    }
LB_FUNCTIONS(LB_GPU_ENTRY)

}
