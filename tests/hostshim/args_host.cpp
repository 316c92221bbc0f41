// args_host.cpp -- TEST SHIM: compiles the product's buffer-argument rule (csrc/pt_args.h) as plain host C++ so that
// tests/test_buffer_args.py can check it against a brute-force restatement without a GPU.  Addresses are only numbers here: no memory
// is touched.  Not part of the product; never loaded by it.
#include <cstring>
#include <vector>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_args.h"

extern "C" {

// check_buffers over a table given as flat arrays of n entries; the message (empty = acceptable) is copied to msg, cut to cap - 1
// characters.  Returns the message's full length.
uint32_t args_host_check(const char* who, uint32_t n, const uint64_t* addr, const uint64_t* bytes, const uint32_t* align, const uint8_t* written,
                         const uint8_t* required, const char* const* names, char* msg, uint32_t cap)
{
    std::vector<pt::BufferUse> use(n);
    for (uint32_t i = 0; i < n; i++)
        use[i] = { reinterpret_cast<const void*>(static_cast<uintptr_t>(addr[i])), bytes[i], align[i], written[i] != 0, required[i] != 0, names[i] };
    const std::string m = pt::check_buffers(who, use.data(), n);
    if (cap) {
        std::strncpy(msg, m.c_str(), cap - 1);
        msg[cap - 1] = '\0';
    }
    return (uint32_t)m.size();
}

}  // extern "C"
