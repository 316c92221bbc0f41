// pt_publish.h -- the device side of pt_physics_publish (row N24, DESIGN.md spec S28): the copy of the simulation's pose into a ring slot
// and a lane's take of a slot into its own scene.  Which slot, and who waits for whom: pt_publish_order.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pt_api.h"

namespace pt {

// A slot holds n spheres, then n rotations.  What a take copies: a null source or destination leaves that part out.
struct PublishTake {
    const float4* cur = nullptr;   // the slot of the generation taken
    const float4* prev = nullptr;  // the slot of the generation before it (the previous pose)
    float4* sph = nullptr;         // <- cur's spheres (n)
    float4* rot = nullptr;         // <- cur's rotations (n)
    float4* prev_pose = nullptr;   // <- prev's spheres, then (prev_rot) its rotations (2n)
    uint32_t n = 0;
    uint32_t prev_rot = 0;
};

// sph, rot (n each) -> slot (2n), one launch
hipError_t launch_physics_publish(const float4* sph, const float4* rot, uint32_t n, float4* slot, hipStream_t stream);

// the copies of a take, one launch (any n > 0); the caller refits afterwards (lbvh_gpu_refit)
hipError_t launch_lane_take(const PublishTake& t, hipStream_t stream);

// Small scenes (lbvh_gpu_refit_fused_possible(n), t.cur and t.sph set): the copies of a take AND the refit of the lane's tree in ONE
// launch -- lbvh_gpu_refit_fused with the slot as its source.  The same arithmetic, the same records.
hipError_t launch_lane_take_small(const PublishTake& t, PtBvhNode* d_nodes, float4* d_sorted, const uint32_t* d_sorted_id, uint32_t* d_hdr, hipStream_t stream);

}  // namespace pt
