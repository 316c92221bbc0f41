// gbframe_leaf_gpu.hip -- TEST SHIM: the encoders and decoders of csrc/pt_pixfmt.h (row N27, spec S30) compiled by hipcc for gfx950 with
// the HIPFLAGS of csrc/Makefile, one thread per 32-bit word.  gbf_gpu_leaf(op, n, in, out) takes HOST pointers and has the signature of
// gbframe_host.cpp's gbf_host_leaf: it copies in, launches, synchronises, copies out and returns the hipError_t as an int (0 = success).
// Nothing in the kernel aborts or asserts; a thread reads and writes only its own word.  Not part of the product; never loaded by it.
#include "gbframe_host.h"

namespace {

__global__ void leaf_kernel(uint32_t op, uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = gbfhost::leaf(op, in[i]);
}

}  // namespace

extern "C" int gbf_gpu_leaf(uint32_t op, uint32_t n, const uint32_t* in, uint32_t* out)
{
    if (n == 0) return 0;
    if (op >= gbfhost::kLeafCount || in == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    hipError_t e = hipMalloc(&d_in, bytes);
    if (e == hipSuccess) e = hipMalloc(&d_out, bytes);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const uint32_t block = 256, grid = (n + block - 1) / block;
        leaf_kernel<<<grid, block>>>(op, n, d_in, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_out);
    return (int)e;
}
