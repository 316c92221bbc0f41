// leaf_batch_host.cpp -- TEST SHIM: the wrappers of leaf_batch.h compiled as plain host C++ (the flags of devmath_host.cpp), one loop
// per wrapper.  lbh_NAME(n, in, out, aux, aux_words) has the signature of leaf_batch_gpu.hip's lbg_NAME and returns 0.
// PT_BEAM_RSQ_TEST: pt_beam.h's host beam_rsq moves its result by pt_beam_rsq_test_ulps floats (0 = the exact host value), which puts
// the error class of the device's reciprocal-square-root instruction into the CPU suite.  The shift is a global of this library, which
// is also the parity reference: with 0 (the initial value, restored by the one test that sets it in a `finally`) the arithmetic is the
// product's host branch -- test_beam_wrappers_match_beam_shim checks that bit for bit -- but the setting is per process, so tests that
// share a process with that test see it only between its set and its restore (sequential pytest; not isolated under a parallel runner
// that threads tests within one process).  Not part of the product; never loaded by it.
#define PT_BEAM_RSQ_TEST 1
#include "leaf_batch.h"

namespace pt {
int pt_beam_rsq_test_ulps = 0;
}

extern "C" {

void lbh_set_beam_rsq_ulps(int ulps) { pt::pt_beam_rsq_test_ulps = ulps; }

#define LB_HOST_ENTRY(name, IN, OUT)                                                                              \
    int lbh_##name(uint32_t n, const float* in, float* out, const float* aux, uint32_t aux_words)                 \
    {                                                                                                             \
        (void)aux_words;                                                                                          \
        for (uint32_t i = 0; i < n; i++) lb::lb_##name(in + (size_t)i * IN, out + (size_t)i * OUT, aux);          \
        return 0;                                                                                                 \
    }
LB_FUNCTIONS(LB_HOST_ENTRY)

}
