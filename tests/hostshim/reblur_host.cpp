// reblur_host.cpp -- TEST SHIM: compiles the product's ReBLUR stand-in header (csrc/pt_reblur.h) as plain host C++ (the flags of
// denoise_host.cpp) so the tests can check it pass by pass against the numpy restatement without a GPU, and the GPU kernels against it
// bit for bit.  Not part of the product; never loaded by it.
#include "reblur_host.h"

extern "C" {

// one pass of pt_nrd_reblur: pass 0 temporal, 1 history fix and fast clamp, 2 blur, 3 post-blur.
// prm = {w, h, max_n, max_fast, fix_frames, restart, frame}; radii = {rmin, rmax}; ptrs in the order of rb_host_buffers
void rb_host_pass(uint32_t pass, const uint32_t* prm, const float* radii, void* const* ptrs)
{
    rb_host_run(pass, rb_host_buffers(prm[0], prm[1], ptrs), rb_host_params(prm, radii));
}

// the blur radius and the specular history cap of spec S32, for the tests of their shape
float rb_host_radius(float rmin, float rmax, float n, float a)
{
    pt::RbParams P{};
    P.rmin = rmin;
    P.rmax = rmax;
    return pt::rb_radius(P, n, a);
}

float rb_host_spec_cap(uint32_t max_n, float roughness, float mx, float my) { return pt::rb_spec_cap(max_n, roughness, mx, my); }

}  // extern "C"
