// chromab_host.cpp -- TEST SHIM: compiles the product's chromatic-aberration header (csrc/pt_chromab.h) as plain host C++ (the flags of
// nis_host.cpp) so the tests can check it against the numpy restatement without a GPU, and the GPU kernel against it bit for bit.  Not
// part of the product; never loaded by it.
#include "chromab_host.h"

extern "C" {

// cab_config's five values: fx, fy, k[0..2]
void chromab_host_config(uint32_t w, uint32_t h, const float* focus_uv, const float* offsets, float* out)
{
    const pt::CabConfig k = pt::cab_config(w, h, focus_uv, offsets);
    out[0] = k.fx; out[1] = k.fy;
    for (int c = 0; c < 3; c++) out[2 + c] = k.k[c];
}

// one call of pt_chromatic_aberration on a w x h image: color and out are float4 per texel
void chromab_host_frame(uint32_t w, uint32_t h, const float* focus_uv, const float* offsets, const void* color, void* out)
{
    chromab_frame((int)w, (int)h, pt::cab_config(w, h, focus_uv, offsets), static_cast<const float4*>(color), static_cast<float4*>(out));
}

// the same call the way pt_chromab.hip runs it: per 32 x 8 block three 35 x 10 windows staged from cab_origin, then the block's texels.
// Returns the number of taps whose index fell outside its window (such a tap reads 0 instead); 0 is what pt_chromab.h proves.
uint64_t chromab_host_frame_tiled(uint32_t w, uint32_t h, const float* focus_uv, const float* offsets, const void* color, void* out)
{
    return chromab_frame_tiled((int)w, (int)h, pt::cab_config(w, h, focus_uv, offsets), static_cast<const float4*>(color), static_cast<float4*>(out));
}

}  // extern "C"
