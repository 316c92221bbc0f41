// pixmap_gpu.hip -- TEST SHIM: csrc/pt_pixel_map.h's slot -> pixel mapping in its device build, compiled by hipcc for gfx950 with the HIPFLAGS
// of csrc/Makefile.
//   pix_gpu_map(desc, n, slots, out, form): out[4 i ..] = {px, py, out_index, valid} of slots[i] for the map that desc describes
//   (pixmap_host.h).  form 0: block_origin on a wave-uniform block index (the wave visits the distinct blocks of its 64 slots one after another,
//   so the origin's arithmetic runs on the scalar unit as in the primary pass) + block_pixel; form 1: the per-lane slot_to_pixel.
// Takes HOST pointers and returns the hipError_t as an int (0 = success).  A thread writes only its own four words.
// Not part of the product; never loaded by it.
#include <hip/hip_runtime.h>

#include "pixmap_host.h"

namespace {

__global__ void map_kernel(pt::PixelMap pm, uint32_t n, const uint32_t* __restrict__ slots, uint32_t* __restrict__ out, int form)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slots[i];
    pt::PixelRef r;
    if (form == 0) {
        const uint32_t block = s >> 6;
        for (bool done = false; !done;) {
            const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane(block);
            if (b == block) {
                r = pt::block_pixel(pt::block_origin(pm, b), s & 63u);
                done = true;
            }
        }
    } else {
        r = pt::slot_to_pixel(pm, s);
    }
    uint32_t* o = out + (size_t)i * 4u;
    o[0] = r.px; o[1] = r.py; o[2] = r.out_index; o[3] = r.valid ? 1u : 0u;
}

}  // namespace

extern "C" int pix_gpu_map(const uint32_t* desc, uint32_t n, const uint32_t* slots, uint32_t* out, int form)
{
    if (n == 0) return 0;
    if (desc == nullptr || slots == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    const pt::PixelMap pm = pixhost::make_map(desc);
    uint32_t *d_slots = nullptr, *d_out = nullptr;
    const size_t in_bytes = (size_t)n * sizeof(uint32_t), out_bytes = in_bytes * 4u;
    hipError_t e = hipMalloc(&d_slots, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_slots, slots, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        map_kernel<<<(n + 255u) / 256u, 256>>>(pm, n, d_slots, d_out, form);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_slots); (void)hipFree(d_out);
    return (int)e;
}
