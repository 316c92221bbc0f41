// pt_api_physics.hip -- the C-ABI of row N23 (pt_physics_*, DESIGN.md spec S27): the state the context owns (PtContext::physics), its tree
// (an LbvhGpu of its own over its own spheres) and the launches of a step on the context's stream.  It reads and writes nothing of the
// scene, the lanes or the frames -- but for pt_physics_publish (row N24, spec S28), which hands the pose to the frames through the context's ring.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_device.h"
#include "pt_trace.h"
#include "pt_physics.h"
#include "pt_publish.h"

struct PtPhysicsState {
    PhDevice d{};
    uint32_t* d_large = nullptr;
    // the tree over d.sph
    LbvhGpu* builder = nullptr;
    PtBvhNode* d_nodes = nullptr;
    float4* d_sorted = nullptr;
    uint32_t* d_sorted_id = nullptr;
    uint32_t* d_refit_flags = nullptr;
    uint32_t* d_refit_hdr = nullptr;
    uint32_t depth = 0;
    bool lds = false;
    PtPhysicsSettings s{};
    PtPhysicsAttractor attractors[PT_PHYSICS_MAX_ATTRACTORS]{};
    uint32_t n_attractors = 0;
    uint64_t steps = 0;
};

namespace {

constexpr uint32_t kPhMaxLdsBytes = 160u * 1024u;   // gfx950 LDS per workgroup
constexpr uint32_t kPhLdsSceneBudget = 64u * 1024u; // the tree is staged in LDS while two 512-thread blocks still fit per CU (pt_build_accel's rule)
constexpr uint32_t kPhMaxBodies = 1u << 30;

void free_state(PtPhysicsState* p)
{
    if (!p) return;
    free_dev(p->d.sph); free_dev(p->d.rot); free_dev(p->d.vel); free_dev(p->d.ang); free_dev(p->d.v0); free_dev(p->d.vel_start); free_dev(p->d.ang_start);
    free_dev(p->d.body); free_dev(p->d.count); free_dev(p->d.acc); free_dev(p->d.report); free_dev(p->d_large);
    free_dev(p->d_nodes); free_dev(p->d_sorted); free_dev(p->d_sorted_id); free_dev(p->d_refit_flags); free_dev(p->d_refit_hdr);
    if (p->builder) lbvh_gpu_destroy(p->builder);
    delete p;
}

bool finite_all(const float* v, size_t n)
{
    for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

// builds the tree over the state's spheres (synchronises the stream) and decides where the walks read it
PtStatus build_tree(PtContext* c, PtPhysicsState* p)
{
    const uint32_t n = p->d.n;
    if (n < 2u) return PT_OK;
    LbvhGpuInfo info{};
    PT_HIP(c, lbvh_gpu_build(p->builder, reinterpret_cast<const float4*>(p->d.sph), n, p->d_nodes, p->d_sorted, p->d_sorted_id, c->stream, &info));
    p->depth = info.depth;
    const uint32_t stack = std::max(1u, p->depth);
    p->lds = traverse_lds_bytes_for(n - 1u, n, 0, true) <= kPhLdsSceneBudget && traverse_lds_bytes_for(n - 1u, n, stack, true) <= kPhMaxLdsBytes / 2;
    if (traverse_lds_bytes_for(n - 1u, n, stack, p->lds) > kPhMaxLdsBytes - 9u * 1024u)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_physics: the tree's depth needs more traversal-stack LDS than a workgroup can have");
    return PT_OK;
}

SceneView tree_view(const PtPhysicsState* p)
{
    SceneView sv{};
    sv.nodes = reinterpret_cast<const float4*>(p->d_nodes);
    sv.sph_sorted = p->d_sorted;
    sv.sorted_id = p->d_sorted_id;
    sv.sph = reinterpret_cast<const float4*>(p->d.sph);
    sv.n = p->d.n;
    sv.n_nodes = p->d.n - 1u;
    sv.stack_depth = std::max(1u, p->depth);
    sv.lds_scene = p->lds ? 1u : 0u;
    return sv;
}

}  // namespace

extern "C" {

void pt_physics_destroy(PtContext* c)
{
    if (!c || !c->physics) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_state(c->physics);
    c->physics = nullptr;
}

PtStatus pt_physics_create(PtContext* c, const PtSphere* spheres, const PtPhysicsBody* bodies, const float* lin_vel, const float* ang_vel, const float* rotations,
                           uint32_t n, const PtPhysicsSettings* settings)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (n > 0 && (!spheres || !bodies)) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_create: null pointer");
    if (n > kPhMaxBodies) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_create: more than 2^30 bodies");
    PtPhysicsSettings s{};
    if (settings) s = *settings;
    if (s.Iterations == 0) s.Iterations = 4;
    if (!settings) { s.Restitution = 0.6f; s.Friction = 0.5f; s.Baumgarte = 0.2f; s.Slop = 0.005f; s.BounceThreshold = 2.0f; }
    if (s.Iterations > 64u || s._pad != 0u || !(s.Restitution >= 0.0f && s.Restitution <= 1.0f) || !(s.Friction >= 0.0f && std::isfinite(s.Friction))
        || !(s.Baumgarte >= 0.0f && s.Baumgarte <= 1.0f) || !(s.Slop >= 0.0f && std::isfinite(s.Slop)) || !(s.BounceThreshold >= 0.0f && std::isfinite(s.BounceThreshold)))
        return fail(c, PT_ERR_INVALID_ARG, "pt_physics_create: settings out of range");
    for (uint32_t i = 0; i < n; i++) {
        if (!finite_all(&spheres[i].cx, 4) || !(spheres[i].r > 0.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_create: sphere " + std::to_string(i) + " is not finite or has no radius");
        if (!(bodies[i].InvMass >= 0.0f && std::isfinite(bodies[i].InvMass)) || (bodies[i].Flags & ~kPhFlagMask) || !std::isfinite(bodies[i].SpringY0) || !std::isfinite(bodies[i].SpringOmega2))
            return fail(c, PT_ERR_INVALID_ARG, "pt_physics_create: body " + std::to_string(i) + " is out of range");
    }
    if ((lin_vel && !finite_all(lin_vel, (size_t)n * 3)) || (ang_vel && !finite_all(ang_vel, (size_t)n * 3)) || (rotations && !finite_all(rotations, (size_t)n * 4)))
        return fail(c, PT_ERR_INVALID_ARG, "pt_physics_create: a velocity or rotation is not finite");
    PT_HIP(c, hipSetDevice(c->device));
    pt_physics_destroy(c);
    // a new simulation: its first published pose has no predecessor (pt_render_gbuffer_published: no object motion)
    publish_restart(c->pub.order);
    for (auto& L : c->lanes) L.pub_prev_gen = 0;

    PtPhysicsState* p = new PtPhysicsState;
    p->s = s;
    p->d.n = n;
    c->physics = p;  // (owned from here on: a failure below leaves an empty state behind, which pt_physics_destroy frees)
    PT_HIP(c, hipMalloc(&p->d.report, 4 * sizeof(uint32_t)));
    PT_HIP(c, hipMemset(p->d.report, 0, 4 * sizeof(uint32_t)));
    if (n == 0) return PT_OK;
    auto fail_empty = [&](PtStatus st) { free_state(p); c->physics = nullptr; return st; };
    std::vector<PhVec4> sph(n), vel(n), ang(n), rot(n);
    std::vector<PtPhysicsBody> body(bodies, bodies + n);
    std::vector<uint32_t> large;
    for (uint32_t i = 0; i < n; i++) {
        sph[i] = { spheres[i].cx, spheres[i].cy, spheres[i].cz, spheres[i].r };
        vel[i] = lin_vel ? PhVec4{ lin_vel[3 * i], lin_vel[3 * i + 1], lin_vel[3 * i + 2], 0.0f } : PhVec4{ 0, 0, 0, 0 };
        ang[i] = ang_vel ? PhVec4{ ang_vel[3 * i], ang_vel[3 * i + 1], ang_vel[3 * i + 2], 0.0f } : PhVec4{ 0, 0, 0, 0 };
        rot[i] = rotations ? PhVec4{ rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3] } : PhVec4{ 0, 0, 0, 1 };
        if ((body[i].Flags & PT_PHYSICS_LARGE) && large.size() < PT_PHYSICS_MAX_LARGE) { large.push_back(i); body[i].Flags |= kPhNoWalk; }
    }
    const size_t v4 = (size_t)n * sizeof(PhVec4);
    auto alloc = [&]() -> hipError_t {
        hipError_t e;
        for (PhVec4** q : { &p->d.sph, &p->d.rot, &p->d.vel, &p->d.ang, &p->d.v0, &p->d.vel_start, &p->d.ang_start })
            if ((e = hipMalloc(q, v4)) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d.body, (size_t)n * sizeof(PtPhysicsBody))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d.count, (size_t)n * sizeof(uint32_t))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d.acc, (size_t)n * kPhAccPerBody * sizeof(long long))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d_large, PT_PHYSICS_MAX_LARGE * sizeof(uint32_t))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d_nodes, (size_t)std::max(1u, n - 1u) * sizeof(PtBvhNode))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d_sorted, (size_t)n * sizeof(float4))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d_sorted_id, (size_t)n * sizeof(uint32_t))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d_refit_flags, (size_t)n * sizeof(uint32_t))) != hipSuccess) return e;
        if ((e = hipMalloc(&p->d_refit_hdr, 16 * sizeof(uint32_t))) != hipSuccess) return e;
        if ((e = hipMemcpy(p->d.sph, sph.data(), v4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(p->d.vel, vel.data(), v4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(p->d.ang, ang.data(), v4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(p->d.rot, rot.data(), v4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(p->d.body, body.data(), (size_t)n * sizeof(PtPhysicsBody), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if (!large.empty() && (e = hipMemcpy(p->d_large, large.data(), large.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemset(p->d.acc, 0, (size_t)n * kPhAccPerBody * sizeof(long long))) != hipSuccess) return e;
        if ((e = hipMemset(p->d.count, 0, (size_t)n * sizeof(uint32_t))) != hipSuccess) return e;
        return hipSuccess;
    };
    if (const hipError_t e = alloc(); e != hipSuccess)
        return fail_empty(fail(c, e == hipErrorOutOfMemory ? PT_ERR_OOM : PT_ERR_HIP, std::string("pt_physics_create: ") + hipGetErrorString(e)));
    p->d.large = p->d_large;
    p->d.n_large = (uint32_t)large.size();
    if (n > 1u) {
        p->builder = lbvh_gpu_create();
        if (!p->builder) return fail_empty(fail(c, PT_ERR_OOM, "pt_physics_create: the tree builder could not be created"));
        if (const PtStatus st = build_tree(c, p); st != PT_OK) return fail_empty(st);
    }
    return PT_OK;
}

PtStatus pt_physics_set_attractors(PtContext* c, const PtPhysicsAttractor* attractors, uint32_t n_attractors)
{
    if (!c) return PT_ERR_INVALID_ARG;
    PtPhysicsState* p = c->physics;
    if (!p) return fail(c, PT_ERR_STATE, "pt_physics_set_attractors: pt_physics_create has not been called");
    if (n_attractors > PT_PHYSICS_MAX_ATTRACTORS || (n_attractors && !attractors)) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_set_attractors: at most 4 attractors, not null");
    for (uint32_t k = 0; k < n_attractors; k++) {
        const PtPhysicsAttractor& a = attractors[k];
        if (a.Body >= p->d.n || a.Kind > PT_PHYSICS_CONSTANT || !std::isfinite(a.Strength) || (a.Target != PT_PHYSICS_ALL_BODIES && a.Target >= p->d.n))
            return fail(c, PT_ERR_INVALID_ARG, "pt_physics_set_attractors: attractor " + std::to_string(k) + " is out of range");
    }
    std::copy(attractors, attractors + n_attractors, p->attractors);
    p->n_attractors = n_attractors;
    return PT_OK;
}

PtStatus pt_physics_step(PtContext* c, float dt, uint32_t substeps, PtPhysicsReport* report)
{
    if (!c) return PT_ERR_INVALID_ARG;
    PtPhysicsState* p = c->physics;
    if (!p) return fail(c, PT_ERR_STATE, "pt_physics_step: pt_physics_create has not been called");
    if (!(dt > 0.0f) || !std::isfinite(dt) || substeps == 0u || substeps > 1024u) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_step: dt must be finite and > 0, substeps in [1, 1024]");
    PhParams prm{};
    prm.h = dt / (float)substeps;
    if (!(prm.h > 0.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_step: dt / substeps underflows");
    prm.restitution = p->s.Restitution; prm.friction = p->s.Friction; prm.baumgarte = p->s.Baumgarte; prm.slop = p->s.Slop; prm.bounce_threshold = p->s.BounceThreshold;
    prm.n_attractors = p->n_attractors;
    std::copy(p->attractors, p->attractors + p->n_attractors, prm.attractors);
    PT_HIP(c, hipSetDevice(c->device));
    const uint32_t n = p->d.n;
    PT_HIP(c, hipMemsetAsync(p->d.report, 0, 4 * sizeof(uint32_t), c->stream));
    for (uint32_t k = 0; k < substeps && n > 0; k++) {
        if (n > 1u) {
            if (p->s.RebuildInterval && p->steps && p->steps % p->s.RebuildInterval == 0) {
                if (const PtStatus st = build_tree(c, p); st != PT_OK) return st;
            } else {
                PT_HIP(c, lbvh_gpu_refit(p->builder, reinterpret_cast<const float4*>(p->d.sph), n, p->d_nodes, p->d_sorted, p->d_sorted_id, p->d_refit_flags, p->d_refit_hdr,
                                         p->depth, c->stream));
            }
        }
        PT_HIP(c, launch_physics_forces(p->d, prm, c->stream));
        if (n > 1u) {
            const SceneView sv = tree_view(p);
            PT_HIP(c, launch_physics_pairs(sv, p->d, prm, true, c->stream));
            for (uint32_t it = 0; it < p->s.Iterations; it++) {
                PT_HIP(c, launch_physics_pairs(sv, p->d, prm, false, c->stream));
                PT_HIP(c, launch_physics_apply(p->d, c->stream));
            }
        }
        PT_HIP(c, launch_physics_integrate(p->d, prm, c->stream));
        p->steps++;
    }
    if (n == 0) p->steps += substeps;
    if (report) {
        uint32_t r[4] = {};
        PT_HIP(c, hipMemcpyAsync(r, p->d.report, sizeof r, hipMemcpyDeviceToHost, c->stream));
        PT_HIP(c, hipStreamSynchronize(c->stream));
        report->Contacts = r[0]; report->Clamped = r[1]; report->Frozen = r[2];
        report->Steps = (uint32_t)p->steps;
    }
    return PT_OK;
}

PtStatus pt_physics_download(PtContext* c, PtSphere* spheres, float* rotations, float* lin_vel, float* ang_vel)
{
    if (!c) return PT_ERR_INVALID_ARG;
    PtPhysicsState* p = c->physics;
    if (!p) return fail(c, PT_ERR_STATE, "pt_physics_download: pt_physics_create has not been called");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipStreamSynchronize(c->stream));
    const uint32_t n = p->d.n;
    if (n == 0) return PT_OK;
    std::vector<PhVec4> tmp(n);
    const size_t v4 = (size_t)n * sizeof(PhVec4);
    if (spheres) PT_HIP(c, hipMemcpy(spheres, p->d.sph, v4, hipMemcpyDeviceToHost));
    if (rotations) PT_HIP(c, hipMemcpy(rotations, p->d.rot, v4, hipMemcpyDeviceToHost));
    if (lin_vel) {
        PT_HIP(c, hipMemcpy(tmp.data(), p->d.vel, v4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) { lin_vel[3 * i] = tmp[i].x; lin_vel[3 * i + 1] = tmp[i].y; lin_vel[3 * i + 2] = tmp[i].z; }
    }
    if (ang_vel) {
        PT_HIP(c, hipMemcpy(tmp.data(), p->d.ang, v4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) { ang_vel[3 * i] = tmp[i].x; ang_vel[3 * i + 1] = tmp[i].y; ang_vel[3 * i + 2] = tmp[i].z; }
    }
    return PT_OK;
}

// Row N24 (DESIGN.md spec S28): the simulation's current pose becomes the pose of every frame from the next render call on -- what
// pt_physics_download + pt_update_spheres (+ pt_update_rotations with textures) would do, without the host: one copy kernel into the
// next slot of the context's ring, behind the steps queued so far; the lanes take it from there when they next render (lane_catch_up).
PtStatus pt_physics_publish(PtContext* c)
{
    if (!c) return PT_ERR_INVALID_ARG;
    PtPhysicsState* p = c->physics;
    if (!p) return fail(c, PT_ERR_STATE, "pt_physics_publish: pt_physics_create has not been called");
    if (!c->scene_set || !c->accel_valid) return fail(c, PT_ERR_STATE, "pt_physics_publish: pt_set_scene + pt_build_accel first");
    const uint32_t n = p->d.n;
    if (c->empty_scene && n == 0) return PT_OK;  // nothing to move
    if (c->empty_scene || n != c->n) return fail(c, PT_ERR_INVALID_ARG, "pt_physics_publish: the body count differs from the scene's sphere count");
    if (!c->gpu_builder) return fail(c, PT_ERR_UNSUPPORTED, "pt_physics_publish needs the device LBVH builder (no PT_FLAG_HOST_LBVH)");
    PT_HIP(c, hipSetDevice(c->device));
    auto& P = c->pub;
    const uint32_t ring = publish_ring_size(c->n_lanes);
    if (P.cap_n != n) {
        // one-off: the ring for this body count, with nothing in flight (a ring of another count holds nothing a frame could still want:
        // the count changes with pt_set_scene only, which forgets what was published)
        for (uint32_t i = 0; i < c->n_lanes; i++) PT_HIP(c, hipStreamSynchronize(c->lanes[i].stream));
        PT_HIP(c, hipStreamSynchronize(c->stream));
        free_dev(P.ring);
        P.cap_n = 0;
        PT_HIP(c, hipMalloc(&P.ring, (size_t)ring * 2u * n * sizeof(float4)));
        for (uint32_t s = 0; s < ring; s++)
            if (!P.ev_slot[s]) PT_HIP(c, hipEventCreateWithFlags(&P.ev_slot[s], hipEventDisableTiming));
        P.cap_n = n;
        publish_restart(P.order);
        for (uint32_t s = 0; s < kPubMaxSlots; s++) { P.order.slot_gen[s] = 0; P.order.readers[s] = 0; }
    }
    const PublishPlan plan = publish_begin(P.order, c->has_textures);
    // the slot's outstanding readers: the caller's stream waits for their markers (a stream wait; none is needed where the marker has passed)
    for (uint32_t i = 0; i < c->n_lanes; i++) {
        Lane& L = c->lanes[i];
        if (!(plan.wait_lanes >> i & 1u) || L.stream == c->stream || !L.ev_pub_read) continue;
        if (hipEventQuery(L.ev_pub_read) == hipSuccess) { publish_reader_done(P.order, i); continue; }
        (void)hipGetLastError();  // hipErrorNotReady is not an error here
        PT_HIP(c, hipStreamWaitEvent(c->stream, L.ev_pub_read, 0));
    }
    PT_HIP(c, launch_physics_publish(reinterpret_cast<const float4*>(p->d.sph), reinterpret_cast<const float4*>(p->d.rot), n, P.ring + (size_t)plan.slot * 2u * n, c->stream));
    if (c->n_lanes > 1) PT_HIP(c, hipEventRecord(P.ev_slot[plan.slot], c->stream));
    // as pt_update_spheres / pt_update_rotations: beam lists are dropped, every lane is behind
    c->scene_gen++;
    ++c->sph_gen;
    if (c->has_textures) ++c->rot_gen;
    return PT_OK;
}

}  // extern "C"
