// args_host.cpp -- TEST SHIM: compiles the product's buffer-argument rule (csrc/pt_args.h) and its buffer ledger and ordering rule of
// frames and side passes (csrc/pt_lane_order.h) as plain host C++ so that tests/test_buffer_args.py and tests/test_lane_order.py can check
// them against restatements without a GPU.  Addresses are only numbers here: no memory is touched.  Not part of the product; never loaded by it.
#include <cstring>
#include <vector>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_args.h"
#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_lane_order.h"

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

// The ledger functions over flat arrays: led = n_lanes ledgers of 21 addresses each (out, dn[3], di[2], gb[13], ri[2]), updated in place;
// a call's pointers as addresses (0 = null).  Each returns `shared`.
namespace {

constexpr uint32_t kLedgerWords = 21;

const void* ptr(uint64_t a) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a)); }

// copies one ledger from (load) or to its 21 words, group by group
void copy_ledger(pt::LaneLedger& l, uint64_t* w, bool load)
{
    const void** const groups[5] = { &l.out, l.dn, l.di, l.gb, l.ri };
    const uint32_t counts[5] = { 1, 3, 2, 13, 2 };
    for (uint32_t g = 0; g < 5; g++)
        for (uint32_t k = 0; k < counts[g]; k++, w++) {
            if (load) groups[g][k] = ptr(*w);
            else *w = reinterpret_cast<uintptr_t>(groups[g][k]);
        }
}

template <typename F>
uint32_t with_ledgers(uint64_t* led, uint32_t n_lanes, uint32_t own, F&& call)
{
    std::vector<pt::LaneLedger> l(n_lanes);
    std::vector<pt::LaneLedger*> of(n_lanes);
    for (uint32_t i = 0; i < n_lanes; i++) { copy_ledger(l[i], led + i * kLedgerWords, true); of[i] = &l[i]; }
    const bool shared = call(pt::Ledgers{ of.data(), n_lanes, own });
    for (uint32_t i = 0; i < n_lanes; i++) copy_ledger(l[i], led + i * kLedgerWords, false);
    return shared ? 1u : 0u;
}

}  // namespace

extern "C" {

uint32_t lane_host_holds(uint64_t* led, uint32_t n_lanes, uint32_t own, uint64_t p, uint32_t groups)
{
    return with_ledgers(led, n_lanes, own, [&](pt::Ledgers v) { return pt::other_lane_holds(v, ptr(p), groups); });
}

// dn: Diffuse, Specular, SpecularHitDistance; di: the DI's two buffers, used when has_di
uint32_t lane_host_frame(uint64_t* led, uint32_t n_lanes, uint32_t own, uint64_t out, const uint64_t* dn, uint32_t has_di, const uint64_t* di)
{
    return with_ledgers(led, n_lanes, own, [&](pt::Ledgers v) { return pt::ledger_frame(v, ptr(out), ptr(dn[0]), ptr(dn[1]), ptr(dn[2]), has_di != 0, ptr(di[0]), ptr(di[1])); });
}

uint32_t lane_host_gbuffer(uint64_t* led, uint32_t n_lanes, uint32_t own, uint32_t first_call, const uint64_t* gb)
{
    const void* g[13];
    for (int k = 0; k < 13; k++) g[k] = ptr(gb[k]);
    return with_ledgers(led, n_lanes, own, [&](pt::Ledgers v) { return pt::ledger_gbuffer(v, first_call != 0, g); });
}

uint32_t lane_host_reservoir(uint64_t* led, uint32_t n_lanes, uint32_t own, uint32_t first_call, const uint64_t* io)
{
    return with_ledgers(led, n_lanes, own, [&](pt::Ledgers v) { return pt::ledger_reservoir(v, first_call != 0, [&](int k) { return ptr(io[k]); }); });
}

// dn: SpecularHitDistance, Diffuse, Specular
uint32_t lane_host_cache(uint64_t* led, uint32_t n_lanes, uint32_t own, uint32_t first_call, uint32_t query, uint64_t out, uint32_t outputs, const uint64_t* dn,
                         uint32_t has_di, const uint64_t* di)
{
    return with_ledgers(led, n_lanes, own, [&](pt::Ledgers v) {
        return pt::ledger_cache(v, first_call != 0, query != 0, ptr(out), outputs != 0, ptr(dn[0]), ptr(dn[1]), ptr(dn[2]), has_di != 0, ptr(di[0]), ptr(di[1]));
    });
}

uint64_t lane_host_window_marker_slot(uint64_t calls, uint64_t n_lanes) { return pt::window_marker_slot(calls, n_lanes); }

}  // extern "C"
