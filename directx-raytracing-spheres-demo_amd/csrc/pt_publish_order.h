// pt_publish_order.h -- where a published pose lives and who may touch it (pt_physics_publish, DESIGN.md spec S28).  Host-only and free of
// HIP, like pt_lane_order.h: tests/hostshim/publish_host.cpp compiles it with g++ and tests/test_publish.py pins it against a restatement of
// the rules below without a GPU.
//
// The simulation runs on the context's stream; every lane reads on a stream of its own, possibly much later.  Publish number g (1, 2, ...:
// never reset) copies the simulation's pose into slot g % R of a ring of R = n_lanes + 2 slots and records the slot's marker on the
// context's stream.  A lane that is behind TAKES the newest generation: it waits for that slot's marker on its stream, copies the slot --
// and, where a previous pose is asked for, the slot of generation g - 1 -- into its own buffers and records its reader marker (one per
// lane, re-recorded by every take: a later record covers the earlier ones).  A publish that is about to overwrite a slot makes the
// context's stream wait for the reader markers of the lanes that read the slot since it was written: `readers`, a bit per lane.  Nothing
// here waits on the host.
//
// The previous pose of generation g is generation g - 1, if it was published since the last restart (pt_physics_create, pt_set_scene) and
// its slot still holds it; else the previous pose is the current one (no object motion).  Since a take always reads the NEWEST generation
// and R >= 3, g - 1 is intact whenever it exists; the test is made all the same.
// pt_update_spheres / pt_update_rotations and a publish may be mixed: the newest call wins, per quantity (sph_live, rot_live).
#pragma once

#include <cstdint>

namespace pt {

constexpr uint32_t kPubMaxLanes = 8, kPubMaxSlots = kPubMaxLanes + 2;

struct PublishOrder {
    uint32_t n_lanes = 1;
    uint64_t gen = 0;                       // publishes so far
    uint64_t first_gen = 1;                 // the oldest generation that may be a previous pose (restart: gen + 1)
    uint64_t slot_gen[kPubMaxSlots] = {};   // the generation every slot holds; 0 = none
    uint32_t readers[kPubMaxSlots] = {};    // lanes whose reader marker covers a read of the slot that may still be running
    bool sph_live = false, rot_live = false;  // the newest spheres / rotations of the scene are the newest generation's
};

static inline uint32_t publish_ring_size(uint32_t n_lanes) { return n_lanes + 2u; }
static inline uint32_t publish_slot(const PublishOrder& o, uint64_t g) { return (uint32_t)(g % publish_ring_size(o.n_lanes)); }

// generation g - 1 exists and its slot still holds it
static inline bool publish_prev_intact(const PublishOrder& o, uint64_t g)
{
    return g >= 2 && g - 1 >= o.first_gen && o.slot_gen[publish_slot(o, g - 1)] == g - 1;
}

// A publish: the new generation, its slot, and the lanes whose reader markers the context's stream must wait for before the slot is
// written (they are no longer outstanding afterwards: the stream wait stands for them).
struct PublishPlan { uint64_t gen; uint32_t slot, wait_lanes; };
static inline PublishPlan publish_begin(PublishOrder& o, bool with_rotations)
{
    const uint64_t g = ++o.gen;
    const uint32_t s = publish_slot(o, g);
    const PublishPlan p{ g, s, o.readers[s] };
    o.readers[s] = 0;
    o.slot_gen[s] = g;
    o.sph_live = true;
    if (with_rotations) o.rot_live = true;
    return p;
}

// A take by `lane`: the newest generation and its slot; prev_slot = the slot of generation g - 1 if a previous pose is wanted and intact,
// else -1 (previous = current).  gen == 0: nothing has been published.
struct TakePlan { uint64_t gen; uint32_t slot; int32_t prev_slot; };
static inline TakePlan publish_take(PublishOrder& o, uint32_t lane, bool want_current, bool want_prev)
{
    TakePlan t{ o.gen, publish_slot(o, o.gen), -1 };
    if (o.gen == 0) return t;
    if (want_current) o.readers[t.slot] |= 1u << lane;
    if (want_prev && publish_prev_intact(o, o.gen)) {
        t.prev_slot = (int32_t)publish_slot(o, o.gen - 1);
        o.readers[t.prev_slot] |= 1u << lane;
    }
    return t;
}

// the lane's reader marker has been seen complete: none of its reads is outstanding
static inline void publish_reader_done(PublishOrder& o, uint32_t lane)
{
    for (uint32_t& r : o.readers) r &= ~(1u << lane);
}

static inline void publish_host_spheres(PublishOrder& o) { o.sph_live = false; }    // pt_update_spheres
static inline void publish_host_rotations(PublishOrder& o) { o.rot_live = false; }  // pt_update_rotations
static inline void publish_restart(PublishOrder& o) { o.first_gen = o.gen + 1; }    // pt_physics_create: the next publish has no predecessor
static inline void publish_forget(PublishOrder& o) { publish_restart(o); o.sph_live = o.rot_live = false; }  // pt_set_scene

}  // namespace pt
