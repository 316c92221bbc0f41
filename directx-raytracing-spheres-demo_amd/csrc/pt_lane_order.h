// pt_lane_order.h -- which caller buffers the lanes' latest calls hold, and when a call on a lane must wait for everything the caller has
// queued instead of the window marker.  Host-only and free of HIP, like pt_args.h: tests/hostshim/args_host.cpp compiles it with g++ and
// tests/test_lane_order.py pins it against a restatement of the table below without a GPU.
//
// A frame, and every side pass of the frame the NEXT render call renders, runs on a lane with a stream of its own.  The caller rotates over
// n_lanes sets of buffers, so a call may start once the marker recorded on the caller's stream at the start of the render call n_lanes - 1
// calls ago has passed (window_marker_slot) -- unless something forces it, or one of the pointers it asks about (null ones are not asked) is
// held by ANOTHER lane's ledger in one of the groups it looks at: then the call is `shared` and waits for everything the caller has queued
// so far (that costs the overlap of the frames, never correctness).  Every call records on its own lane's ledger, always overwriting:
//   frame (render_common)         asks out and its dn Diffuse, Specular, SpecularHitDistance; looks at out, dn, di; forced by a supplied DI;
//                                 records out, dn = Diffuse, Specular, SpecularHitDistance, di = the supplied DI's buffers or nulls
//   G-buffer (pt_render_gbuffer)  asks its 13 channels; looks at out, gb, dn, di; forced by first_call; records gb = the 13 pointers, nulls included
//   reservoir (pt_restir_di*)     asks its 8 inputs and 2 outputs; looks at all five groups; forced by first_call and by an input that is not in
//                                 its OWN lane's gb (it was made elsewhere: on the caller's stream; tested first); records ri = Diffuse, Specular
//   cache (pt_render_sharc*)      asks, with QUERY only, out, SpecularHitDistance, Diffuse, Specular; looks at all five groups; forced by first_call
//                                 and by a supplied DI; records only with a DI or denoiser outputs: dn = SpecularHitDistance, Diffuse, Specular
//                                 (nulls without QUERY), di = the DI's buffers or nulls
//   G-buffer frame                asks out and its 8 input channels; looks at all five groups; forced by first_call, by a supplied DI and by an
//   (pt_render_from_gbuffer)      input that is not in its OWN lane's gb (made elsewhere: on the caller's stream; written by pt_render_gbuffer*
//                                 on the same lane just before, it is ordered by the lane's stream); records di = the DI's buffers or nulls
//                                 with a DI, and, where an input was made elsewhere, gb = the inputs at their channels (nulls between them): a
//                                 G-buffer, reservoir or cache call of another lane that would write one of them inside the window then waits
// first_call: no render call has recorded a marker yet (PtContext::calls == 0).  A supplied DI is an input that may have been written on the
// caller's stream right before the call, after the window marker.  Three asymmetries are kept as they are (removing one would add waits):
// frames and the G-buffer pass do not look at `ri` (a caller that hands them a DI output of another lane inside the window relies on the
// rotation rule); the cache pass does not record the `out` it writes; and it stores `dn` in another order than the frames do (no answer
// depends on that: a group is searched whole).
#pragma once

#include <algorithm>
#include <cstdint>

namespace pt {

// the buffers of a lane's latest frame (out, dn; di = the DI buffers it READ: a later frame on another lane that writes one must not
// overwrite it before this frame's gather has read it), G-buffer call (gb) and reservoir pass (ri)
struct LaneLedger { const void *out = nullptr, *dn[3] = {}, *di[2] = {}, *gb[13] = {}, *ri[2] = {}; };
enum : uint32_t { kLedgerOut = 1u, kLedgerDn = 2u, kLedgerDi = 4u, kLedgerGb = 8u, kLedgerRi = 16u, kLedgerAll = 31u };
struct Ledgers { LaneLedger* const* of; uint32_t n_lanes, own; };  // every lane's ledger, and the lane the call runs on

// does a lane other than v.own hold p in one of `groups`?  Null is no buffer: it never matches, not even an empty slot.
static inline bool other_lane_holds(Ledgers v, const void* p, uint32_t groups)
{
    for (uint32_t i = 0; p && i < v.n_lanes; i++) {
        if (i == v.own) continue;
        const LaneLedger& o = *v.of[i];
        bool hit = (groups & kLedgerOut) && p == o.out;
        for (const void* q : o.dn) hit = hit || ((groups & kLedgerDn) && p == q);
        for (const void* q : o.di) hit = hit || ((groups & kLedgerDi) && p == q);
        for (const void* q : o.gb) hit = hit || ((groups & kLedgerGb) && p == q);
        for (const void* q : o.ri) hit = hit || ((groups & kLedgerRi) && p == q);
        if (hit) return true;
    }
    return false;
}

// The four families of the table: each returns `shared` and records on v.own's ledger.  has_di: a DI is supplied (di_d, di_s: its buffers).
static inline bool ledger_frame(Ledgers v, const void* out, const void* diffuse, const void* specular, const void* hit_dist, bool has_di, const void* di_d, const void* di_s)
{
    bool shared = has_di;
    for (const void* p : { out, diffuse, specular, hit_dist }) shared = shared || other_lane_holds(v, p, kLedgerOut | kLedgerDn | kLedgerDi);
    LaneLedger& me = *v.of[v.own];
    me.out = out; me.dn[0] = diffuse; me.dn[1] = specular; me.dn[2] = hit_dist;
    me.di[0] = has_di ? di_d : nullptr; me.di[1] = has_di ? di_s : nullptr;
    return shared;
}

static inline bool ledger_gbuffer(Ledgers v, bool first_call, const void* const gb[13])
{
    bool shared = first_call;
    for (int k = 0; k < 13; k++) shared = shared || other_lane_holds(v, gb[k], kLedgerOut | kLedgerGb | kLedgerDn | kLedgerDi);
    std::copy(gb, gb + 13, v.of[v.own]->gb);
    return shared;
}

template <typename Get>  // get(k): the 8 inputs, then Diffuse and Specular
static inline bool ledger_reservoir(Ledgers v, bool first_call, Get&& get)
{
    LaneLedger& me = *v.of[v.own];
    bool shared = first_call;
    for (int k = 0; k < 8; k++) shared = shared || std::find(me.gb, me.gb + 13, get(k)) == me.gb + 13;
    for (int k = 0; k < 10; k++) shared = shared || other_lane_holds(v, get(k), kLedgerAll);
    me.ri[0] = get(8); me.ri[1] = get(9);
    return shared;
}

// hit_dist, diffuse, specular: null where the call has no such output; outputs: denoiser outputs were asked for
static inline bool ledger_cache(Ledgers v, bool first_call, bool query, const void* out, bool outputs, const void* hit_dist, const void* diffuse, const void* specular, bool has_di, const void* di_d, const void* di_s)
{
    bool shared = first_call || has_di;
    for (const void* p : { out, hit_dist, diffuse, specular }) shared = shared || (query && other_lane_holds(v, p, kLedgerAll));
    if (has_di || outputs) {
        LaneLedger& me = *v.of[v.own];
        me.dn[0] = query ? hit_dist : nullptr; me.dn[1] = query ? diffuse : nullptr; me.dn[2] = query ? specular : nullptr;
        me.di[0] = has_di ? di_d : nullptr; me.di[1] = has_di ? di_s : nullptr;
    }
    return shared;
}

// in13: the 8 input channels at their places among PtGBuffer's 13, nulls elsewhere
static inline bool ledger_gbframe(Ledgers v, bool first_call, const void* out, const void* const in13[13], bool has_di, const void* di_d, const void* di_s)
{
    LaneLedger& me = *v.of[v.own];
    bool elsewhere = false, shared = false;
    for (int k = 0; k < 13; k++) elsewhere = elsewhere || (in13[k] && std::find(me.gb, me.gb + 13, in13[k]) == me.gb + 13);
    for (int k = 0; k < 13; k++) shared = shared || other_lane_holds(v, in13[k], kLedgerAll);
    shared = ledger_cache(v, first_call, true, out, false, nullptr, nullptr, nullptr, has_di, di_d, di_s) || shared || elsewhere;
    if (elsewhere) std::copy(in13, in13 + 13, me.gb);
    return shared;
}

// the slot of PtContext::ev_in with the marker of the render call n_lanes - 1 calls before call number `calls`; slot 0 before that call exists
static inline uint64_t window_marker_slot(uint64_t calls, uint64_t n_lanes) { return calls >= n_lanes - 1 ? (calls - (n_lanes - 1)) % n_lanes : 0; }

}  // namespace pt
