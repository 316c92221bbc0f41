// pt_args.h -- the buffer-argument rule of the C-ABI passes that take caller buffers (pt_nrd_composition, pt_nrd_denoise, pt_upscale,
// pt_nis_sharpen, pt_frame_gen, pt_restir_di): every required pointer present, every pointer aligned to its channel width, and no
// buffer the pass writes sharing a byte with any other buffer of the call.  Host-only and free of HIP, so that tests/hostshim/args_host.cpp
// compiles it with g++ and tests/test_buffer_args.py checks it without a GPU.
#pragma once

#include <cstdint>
#include <string>

namespace pt {

struct BufferUse {
    const void* p;
    uint64_t bytes;
    uint32_t align;
    bool written;
    bool required;
    const char* name;
};

// "" if the table is acceptable, else the message of the first violation: presence and alignment in table order first, then every
// written buffer against every other one, both in table order.  A null optional buffer takes no part; touching ranges do not overlap;
// two inputs may share memory.
inline std::string check_buffers(const char* who, const BufferUse* use, uint32_t n)
{
    const std::string head = std::string(who) + ": ";
    for (uint32_t i = 0; i < n; i++) {
        const BufferUse& u = use[i];
        if (!u.p) {
            if (u.required) return head + u.name + " is required";
            continue;
        }
        if (reinterpret_cast<uintptr_t>(u.p) % u.align) return head + u.name + " is not " + std::to_string(u.align) + "-byte aligned";
    }
    for (uint32_t i = 0; i < n; i++) {
        const BufferUse& a = use[i];
        if (!a.p || !a.written) continue;
        for (uint32_t j = 0; j < n; j++) {
            const BufferUse& b = use[j];
            if (i == j || !b.p) continue;
            const uintptr_t pa = reinterpret_cast<uintptr_t>(a.p), pb = reinterpret_cast<uintptr_t>(b.p);
            if (pa < pb + b.bytes && pb < pa + a.bytes) return head + a.name + " overlaps " + b.name;
        }
    }
    return std::string();
}

}  // namespace pt
