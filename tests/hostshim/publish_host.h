// publish_host.h -- pt_publish_order.h (row N24, host-only) behind flat functions: the calls tests/test_publish.py makes through the shared
// library (publish_host.cpp) and the stand-alone sanitizer program makes directly (publish_sanitize.cpp).
#pragma once

#include <cstdint>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_publish_order.h"

namespace pubshim {

inline pt::PublishOrder* make(uint32_t n_lanes)
{
    pt::PublishOrder* o = new pt::PublishOrder();
    o->n_lanes = n_lanes;
    return o;
}

// out: gen, slot, lanes to wait for
inline void publish(pt::PublishOrder* o, int with_rotations, uint64_t out[3])
{
    const pt::PublishPlan p = pt::publish_begin(*o, with_rotations != 0);
    out[0] = p.gen; out[1] = p.slot; out[2] = p.wait_lanes;
}

// out: gen, slot, prev_slot (-1: previous = current)
inline void take(pt::PublishOrder* o, uint32_t lane, int want_current, int want_prev, int64_t out[3])
{
    const pt::TakePlan t = pt::publish_take(*o, lane, want_current != 0, want_prev != 0);
    out[0] = (int64_t)t.gen; out[1] = t.slot; out[2] = t.prev_slot;
}

// out: gen, first_gen, sph_live, rot_live, slot_gen[kPubMaxSlots], readers[kPubMaxSlots]
inline void state(const pt::PublishOrder* o, uint64_t out[4 + 2 * pt::kPubMaxSlots])
{
    out[0] = o->gen; out[1] = o->first_gen; out[2] = o->sph_live; out[3] = o->rot_live;
    for (uint32_t s = 0; s < pt::kPubMaxSlots; s++) { out[4 + s] = o->slot_gen[s]; out[4 + pt::kPubMaxSlots + s] = o->readers[s]; }
}

}  // namespace pubshim
