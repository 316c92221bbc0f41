// pt_launch.h -- host side of the kernel launches that take dynamic LDS: one launcher (the opt-in for more than the default LDS
// limit, the launch, the error) and the choice of the template arguments a launch wrapper derives from run-time values.
#pragma once

#include "pt_device.h"

namespace pt {

// static LDS of the kernels (counters, the segment prefix table of the looping pass) on top of their dynamic LDS: the
// 64 KB default limit counts both, so the opt-in for more is taken this much earlier
constexpr uint32_t kStaticLdsMargin = (kMaxSegs + 64u + kCutSlots) * 4u;

// Launches `kernel` with `lds` bytes of dynamic LDS; the kernel's arguments follow the stream.
template <typename... Params, typename... Args>
hipError_t launch_kernel(void (*kernel)(Params...), uint32_t grid, uint32_t threads, uint32_t lds, hipStream_t stream, const Args&... args)
{
    if (lds + kStaticLdsMargin > 65536u) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, stream, args...);
    return hipGetLastError();
}

// f.operator()<kLds, StackT>() for the tree the scene has: kLds -- the kernels walk a copy staged in LDS; StackT -- the type of a
// stack entry (16 bits hold a child reference of a tree with fewer than 32767 nodes: stack_encode, pt_trace.h)
template <typename F>
hipError_t with_tree_walk(const SceneView& sv, F&& f)
{
    const bool small = sv.n_nodes < 32767u;
    if (sv.lds_scene) return small ? f.template operator()<true, uint16_t>() : f.template operator()<true, uint32_t>();
    return small ? f.template operator()<false, uint16_t>() : f.template operator()<false, uint32_t>();
}

// f.operator()<flag>(): a run-time switch as a template argument
template <typename F>
hipError_t with_flag(bool flag, F&& f)
{
    return flag ? f.template operator()<true>() : f.template operator()<false>();
}

}  // namespace pt
