// denoise_host.cpp -- TEST SHIM: compiles the product's NRD stand-in header (csrc/pt_denoise.h) as plain host C++ (the flags of
// nrd_host.cpp) so the tests can check it pass by pass against the numpy restatement without a GPU, and the GPU kernels against it
// bit for bit.  Not part of the product; never loaded by it.
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_denoise.h"

using namespace pt;

namespace {

template <uint32_t kMode>
void run(uint32_t pass, const DnBuffers& b, const DnParams& P, int src, int step)
{
    for (int y = 0; y < (int)b.h; y++)  // what each lane of pt_denoise.hip does, one launch per pass
        for (int x = 0; x < (int)b.w; x++) {
            if (pass == 0) dn_temporal_px<kMode>(b, P, x, y);
            else if (pass == 1) dn_variance_px(b, x, y);
            else if (pass == 2) dn_atrous_px<kMode, false>(b, src, step, x, y);
            else dn_atrous_px<kMode, true>(b, src, step, x, y);
        }
}

}  // namespace

extern "C" {

// one pass of pt_nrd_denoise: pass 0 temporal, 1 variance, 2 a-trous step, 3 last a-trous step; mode 2 ReBLUR / 3 ReLAX.
// prm = {w, h, max_d, max_s, restart, src, step}; ptrs = viewz, mv, nr, in_d, in_s, out_d, out_s, prev_sig_d, prev_sig_s, prev_mom,
// prev_guide, sig_d, sig_s, mom, guide, hitd, xd0, xs0, xd1, xs1 (what a pass does not touch may be null)
void dn_host_pass(uint32_t pass, uint32_t mode, const uint32_t* prm, void* const* ptrs)
{
    DnBuffers b{};
    b.w = prm[0];
    b.h = prm[1];
    b.viewz = static_cast<const float*>(ptrs[0]);
    b.mv = static_cast<const float*>(ptrs[1]);
    b.nr = static_cast<const float4*>(ptrs[2]);
    b.in_d = static_cast<const float4*>(ptrs[3]);
    b.in_s = static_cast<const float4*>(ptrs[4]);
    b.out_d = static_cast<float4*>(ptrs[5]);
    b.out_s = static_cast<float4*>(ptrs[6]);
    b.prev_sig_d = static_cast<const float4*>(ptrs[7]);
    b.prev_sig_s = static_cast<const float4*>(ptrs[8]);
    b.prev_mom = static_cast<const float4*>(ptrs[9]);
    b.prev_guide = static_cast<const float4*>(ptrs[10]);
    b.sig_d = static_cast<float4*>(ptrs[11]);
    b.sig_s = static_cast<float4*>(ptrs[12]);
    b.mom = static_cast<float4*>(ptrs[13]);
    b.guide = static_cast<float4*>(ptrs[14]);
    b.hitd = static_cast<float*>(ptrs[15]);
    b.xd[0] = static_cast<float4*>(ptrs[16]);
    b.xs[0] = static_cast<float4*>(ptrs[17]);
    b.xd[1] = static_cast<float4*>(ptrs[18]);
    b.xs[1] = static_cast<float4*>(ptrs[19]);
    DnParams P{prm[2], prm[3], prm[4]};
    if (mode == kNrdReblur) run<kNrdReblur>(pass, b, P, (int)prm[5], (int)prm[6]);
    else run<kNrdRelax>(pass, b, P, (int)prm[5], (int)prm[6]);
}

}  // extern "C"
