// pt_context.h -- the context behind the C-ABI's opaque PtContext and the helpers every entry point uses (fail, PT_HIP, free_dev).
// Internal to the three translation units that implement include/pt_api.h: pt_api.hip (the context, the scene, the tree, the beam cache
// and the frames), pt_api_side.hip (the side passes of a frame: G-buffer, reservoir pass, radiance cache; they share the helpers declared
// at the end of this file) and pt_api_post.hip (the passes that touch nothing but the context's stream and their own state).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: the library itself is loaded at run time (pt_comm_init)

#include <string>
#include <utility>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_args.h"
#include "pt_kernels.h"
#include "pt_lane_order.h"
#include "pt_lbvh.h"
#include "pt_lbvh_gpu.h"
#include "pt_publish_order.h"

using namespace pt;  // (an internal header: the units it serves are written in pt's names throughout)

struct EventPair {
    hipEvent_t a, b;
    int kind;  // 0 primary, 1 traverse / fused bounce, 2 shade, 3 looping pass
};

// PT_* tuning knobs (DESIGN.md "Tuning knobs"): environment variables for A/B runs, read ONCE when the context is created --
// the render path never touches the environment.  -1 = not set (the measured default applies).
struct Knobs {
    int split = -1, traverse_blocks_per_cu = -1, fused_threads = -1, no_adaptive_grid = -1, shade_blocks_per_cu = -1, tail_threshold = -1,
        tail_blocks_per_cu = -1, loop_threads = -1, inline2_min_slots = -1, tail_after = -1, seg = -1, loop_use_tail = -1, fuse_loop = -1,
        ray_replacement = -1, dyn_blocks_per_cu = -1, debug_counts = -1, sah = -1, sah_max_spheres = -1, beams = -1, wide = -1, descent = -1, roctx = -1, lane_priority = -1, fused_refit = -1, beam_reach = -1, beam_max_slack_pct = -1, beam_max_margin = -1, beam_share_wgs = -1, refl_beams = -1, coop_walk = -1, tile_order = -1, sky_fast = -1, tile_table = -1, tile_interleave = -1;
};

struct PtPhysicsState;

// Per-frame-in-flight state (see PtContext::lanes).
struct Lane {
    hipStream_t stream = nullptr;  // == PtContext::stream when there is a single lane
    hipEvent_t ev_done = nullptr;
    size_t cap_slots = 0;
    RayQueue q[2]{};
    Scratch scratch{};
    bool scratch_spp = false;
    uint32_t* d_counts = nullptr;  // two parities: [0, cap_counts) and [cap_counts, 2 cap_counts)
    size_t cap_counts = 0;
    uint32_t parity = 0;           // parity of the frame being (or last) submitted on this lane
    uint32_t* h_counts = nullptr;  // pinned
    // queue sizes of a recent frame (pinned, written by an async copy, read without waiting): they only size the
    // launch grids -- every kernel is a grid-stride loop, so a stale or missing estimate costs time, never correctness
    uint32_t* h_prev_counts = nullptr;   // host-mapped: the GPU writes it when it folds a frame's counters (no copy call)
    uint32_t* d_prev_counts = nullptr;   // device address of h_prev_counts
    uint64_t prev_signature = 0;
    uint32_t* d_seg_counts = nullptr;        // kMaxSegs segment sizes of the primary pass -> looping pass hand-over
    static constexpr uint32_t kTotals = 10;
    unsigned long long* d_totals = nullptr;  // [0] running secondary-ray total, [1] last folded frame, [2],[3] tail counters,
                                             // [4] running count of in-register secondary rays of primary passes, [5] unused,
                                             // [6] node visits, [7] sphere tests of the global-memory traversal kernels,
                                             // [8] waves of primary passes that traced in-register bounce-1 rays, [9] ... of them from a
                                             // reflection-beam list (pt_get_refl_stats)
    // private copy of the moving part of the scene (pt_update_spheres / pt_refit_accel): spheres, Morton-ordered spheres
    // and node boxes; null = this lane renders the context's master scene
    float4* d_sph = nullptr;
    float4* d_sph_sorted = nullptr;
    float4* d_nodes = nullptr;
    uint32_t* d_refit_flags = nullptr;
    uint32_t* d_refit_hdr = nullptr;
    PtSphere* h_stage = nullptr;      // pinned upload staging, host-mapped ...
    const float4* d_stage = nullptr;  // ... and its device address (the single-launch refit of small scenes reads the staging buffer itself)
    hipEvent_t ev_upload = nullptr;   // the last upload from h_stage has been consumed
    hipEvent_t ev_poll[4] = {};       // queue-size read-backs of the last passes (spp > 1 lagged polling)
    uint32_t scene_n = 0;             // sphere count the private copy was allocated for
    bool scene_private = false;
    uint64_t sph_gen = 0;         // the pt_update_spheres generation this lane's private scene holds (PtContext::sph_gen)
    float slab_tiny = 1e-30f;     // SceneView::slab_tiny of the private scene: chosen by pt_update_spheres from the staged coordinates, travels with sph_gen
    bool needs_refit = false;     // spheres were staged on this lane and its boxes / Morton-ordered copy have not been redone yet
    bool upload_pending = false;  // h_stage holds spheres that have not been copied to d_sph yet (pt_update_spheres of a small scene: pt_refit_accel's kernel reads them)
    LaneLedger ledger;  // the caller buffers of the lane's latest frame, G-buffer call and reservoir pass (pt_lane_order.h: repeated buffers inside the window)
    // object rotations (textured scenes): the lane's own copy, refreshed from PtContext::h_rot when its generation is behind
    float4* d_rot = nullptr;
    float4* h_rot_stage = nullptr;    // pinned
    hipEvent_t ev_rot = nullptr;      // the last upload from h_rot_stage has been consumed
    uint64_t rot_gen = 0;
    uint32_t rot_n = 0;
    // pt_render_gbuffer: the caller's previous poses (spheres, then rotations) as the lane's calls read them, their pinned staging
    // buffer, and the marker that orders a G-buffer call after what the caller queued on `stream`
    float4* d_prev_pose = nullptr;
    float4* h_prev_stage = nullptr;
    hipEvent_t ev_prev = nullptr;     // the last upload from h_prev_stage has been consumed
    uint32_t prev_cap = 0;            // spheres the two buffers hold room for
    hipEvent_t ev_gb_in = nullptr;
    // pt_physics_publish (row N24): the lane's reader marker (pt_publish_order.h), and the generation whose previous pose d_prev_pose holds
    // (0 = none) with whether that generation had one (else previous = current)
    hipEvent_t ev_pub_read = nullptr;
    uint64_t pub_prev_gen = 0;
    bool pub_prev_valid = false;
};
constexpr uint32_t kMaxLanes = 8;

// A pass's history on the context's stream: one allocation holding two alternating slots, made on first use and again when `dims`
// change; a change of `tag` (or of dims) restarts the history.
struct History {
    void* mem = nullptr;
    uint32_t dims[4] = {};  // the sizes `mem` was allocated for
    uint32_t slot = 0;      // the slot the last call wrote
    uint64_t tag = 0;       // the pass's restart tag as of the last call
    bool valid = false;
};

struct PtContext {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t flags = 0;
    uint32_t tile_size = 32;
    uint32_t num_cus = 256;
    Knobs knobs;
    std::string err;

    // scene
    uint32_t n = 0;
    float4* d_sph = nullptr;
    float4* d_mats = nullptr;
    PtSceneData sd{};
    std::vector<PtSphere> h_sph;
    bool scene_set = false;

    // textures (row N1): table of linear float4 images + per-sphere map indices and rotations
    std::vector<float4*> d_tex_images;
    std::vector<std::pair<uint32_t, uint32_t>> tex_dims;  // width, height of every table entry
    TexView* d_tex = nullptr;
    uint32_t* d_tex_maps = nullptr;  // n * 8
    float4* d_rot = nullptr;         // n: the rotations as of pt_set_textures (single-lane contexts update it in stream order)
    std::vector<float4> h_rot;       // latest rotations (pt_update_rotations); lanes pick them up when they next render
    uint64_t rot_gen = 0;            // generation of h_rot (never reset) ...
    uint64_t rot_master_gen = 0;     // ... and the generation d_rot holds: while they are equal every lane reads d_rot
    bool has_textures = false;

    // emissive spheres (row N4)
    uint32_t* d_lights = nullptr;
    uint32_t* d_light_of = nullptr;  // per sphere: its index in d_lights or 0xFFFFFFFF (pt_restir_di_ex's BRDF candidates, spec S23)
    uint32_t n_lights = 0;

    // alpha-tested hits (spec S10): the spheres whose AlphaMode is not Opaque, their class per sphere on the device (null while
    // every sphere is kAlphaVisible) and the leaf ids carrying it (Morton order; null = the traversal reads d_sorted_id)
    struct AlphaMat { uint32_t id; float base[4]; float cutoff; uint32_t base_map; };
    std::vector<AlphaMat> alpha_mats;
    uint32_t* d_alpha_class = nullptr;
    uint32_t* d_leaf_ids = nullptr;
    bool alpha_tested = false;

    // accel
    float4* d_nodes = nullptr;
    float4* d_wide = nullptr;        // 4-wide view of the tree (global-memory scenes only; null otherwise)
    float4* d_sph_sorted = nullptr;
    uint32_t* d_sorted_id = nullptr;
    uint32_t n_nodes = 0, depth = 0;
    bool lds_scene = false;
    bool accel_valid = false;
    LbvhResult lbvh;  // host copy (download / info); filled by either builder
    LbvhGpu* gpu_builder = nullptr;

    // frame state
    PtCamera cam{};
    PtGraphicsSettings gs{};
    bool cam_set = false, gs_set = false;
    uint32_t rank = 0, world = 1;                       // pt_set_partition (kept for pt_tiles_count(rank))
    uint32_t part_first = 0, part_run = 1, part_stride = 1;  // the residue range this context renders (pt_set_partition_ex)

    // work buffers: one set per frame in flight.  Frame f runs on lane f % n_lanes, on that lane's own stream, so the
    // latency-bound looping pass of one frame overlaps the throughput-bound first passes of the next.
    Lane lanes[kMaxLanes];
    LaneLedger* ledgers[kMaxLanes];  // &lanes[i].ledger (pt_create): the form pt_lane_order.h takes them in
    uint32_t n_lanes = 1;
    uint32_t next_lane = 0;
    uint32_t last_lane = 0;
    hipEvent_t ev_in[kMaxLanes] = {};  // markers on `stream` at the start of the last n_lanes render calls
    uint64_t calls = 0;
    uint64_t sph_gen = 0;      // counts pt_update_spheres calls since pt_set_scene; latest_lane: the lane whose staging buffer holds the newest spheres
    int latest_lane = -1;
    bool empty_scene = false;  // pt_set_scene(n = 0): one internal sphere that no ray can hit stands in (see pt_set_scene)
    float4* d_out = nullptr;
    size_t cap_out = 0;
    // pt_render_gbuffer before the render call that will take lane `gb_lane` as frame number `gb_frame`: whether every lane was idle
    // when it was made (render_common's one-frame-at-a-time test must not mistake that frame's own G-buffer work for a frame in flight)
    uint64_t frames = 0;  // render calls that took a lane
    uint64_t gb_frame = ~0ull;
    uint32_t gb_lane = 0;
    bool gb_lanes_idle = false;
    float4* d_bloom = nullptr;  // pt_bloom's blur chain (used on `stream` only), grown on demand
    uint64_t cap_bloom = 0;     // texels
    // The passes that keep a two-slot history on `stream` (pt_api_post.hip: history_begin / history_commit):
    //   dn  pt_nrd_denoise: history and work buffers, kDnBytesPerPixel per pixel; dims = RenderSize, tag = the denoiser mode
    //   up  pt_upscale (row N11): per output pixel and slot a float4 and a float; dims = OutputSize, tag = InputSize
    //   fg  pt_frame_gen (row N13): the motion field (8 B per render pixel), then per slot the previous Color (4 B per output pixel) and
    //       Depth (4 B per render pixel); dims = RenderSize, OutputSize, tag = the Format
    //   rr  pt_ray_reconstruction (row N15): per slot and output pixel two float4 and a float, then the prepare pass's three float4
    //       records per render pixel; dims = OutputSize, RenderSize, no tag
    //   rb  pt_nrd_reblur (row N30): history and work buffers, kRbBytesPerPixel per pixel; dims = RenderSize, no tag (last: the members
    //       before it keep their places)
    History dn, up, fg, rr;
    // pt_restir_di's history (row N10): two alternating slots of kRiBytesPerPixel / 2 bytes per pixel (surface record + reservoir),
    // allocated on first use and again when RenderSize changes; `ri_slot` = the slot the last call wrote, `ri_scene` = the
    // pt_set_scene count it was made under (emitter indices change with the scene), `ev_ri` = the last call's launches have finished
    // (consecutive calls run on different lanes and hand the history to each other)
    float4* d_ri = nullptr;
    uint32_t ri_w = 0, ri_h = 0, ri_slot = 0;
    uint64_t ri_scene = 0, set_scene_calls = 0;
    bool ri_valid = false;
    hipEvent_t ev_ri = nullptr;
    // pt_restir_di_sampled's presampled structures (row N16): the power pyramid and the RIS buffer (Power segment, then ReGIR segment),
    // rebuilt by every call with a presampling mode, grown on demand, protected by ev_ri like the history; lr_n_*: what the last such
    // call built (pt_light_ris_download)
    float* d_lr_pyramid = nullptr;
    void* d_lr_ris = nullptr;
    uint32_t lr_cap_pyramid = 0, lr_cap_ris = 0, lr_n_pyramid = 0, lr_n_ris = 0;
    // pt_render_sharc's cache (row N14): `sh_capacity` keys and two voxel arrays in one allocation (sh_accum = this frame's accumulators,
    // sh_resolved = the previous frame's resolved voxels: they swap at every resolve), two device counters (rays, failed inserts),
    // `sh_scene` = the pt_set_scene count the cache was filled under, `ev_sh` = the last call's launches have finished
    void* d_sh = nullptr;
    uint64_t* sh_keys = nullptr;
    uint4* sh_accum = nullptr;
    uint4* sh_resolved = nullptr;
    unsigned long long* d_sh_counters = nullptr;
    uint32_t sh_capacity = 0;
    uint64_t sh_scene = 0;
    bool sh_valid = false;
    hipEvent_t ev_sh = nullptr;
    // pt_render_lens (row N26): one ray counter per lane (calls on one lane are ordered by its stream), made by the first call;
    // pt_render_from_gbuffer (row N27) counts its rays there too
    unsigned long long* d_lens_counters = nullptr;
    uint64_t tot_pixels = 0, tot_paths = 0, tot_fixed_bytes = 0, tot_sec_coeff = 96;  // host-known parts of the totals
    uint32_t tot_beam_frames = 0;  // frames since the last reset whose primary pass used the primary-beam lists

    // Primary beams (DESIGN.md "Primary beams"): per-8x8-block candidate sphere lists for the primary pass.  They depend on the
    // camera's lens, the frame geometry and the scene, on the camera's POSITION up to the slack (Beam::slack) and on its ORIENTATION
    // up to the pixel margin (make_beam) they were built with -- not on the frame index or the jitter (the beams are a pixel wider
    // than the blocks).  A view that RESTS gets exact lists on its second frame (one launch on a side stream); a camera that
    // travels and turns gets lists centred and oriented some frames ahead of it, with a slack of a few frames' travel and a margin
    // of a few frames' turn, built in shares inside the frames' own primary passes
    // while the frames use the previous ones -- a frame never waits for a build of the moving kind: it takes the newest lists that
    // are readable and hold for its pose, or traverses per ray.
    struct BeamLists {
        uint32_t* d_lists = nullptr;   // n_blocks records of 16 dwords
        size_t cap_blocks = 0;
        uint32_t* d_regions = nullptr; // reflection beams: n_blocks region records of kReflRecord dwords (pt_region.h) ...
        size_t cap_regions = 0;
        bool regions = false;          // ... that d_regions holds for these lists (resting views' builds only)
        std::vector<uint32_t> key;     // orientation, frame geometry, scene generation of the lists in d_lists; empty = none
        float pos[3] = { 0, 0, 0 };    // the camera position they were built around ...
        float slack = 0.0f;            // ... and how far from it they hold
        float basis[9] = {};           // the orientation (Right, Up, Forward) they were built for ...
        float margin_px = 0.0f;        // ... and by how many pixels a ray's crossing of the image may differ from that orientation's
        hipEvent_t ev_ready = nullptr;   // the build has finished
        bool building = false;         // launched, ev_ready not yet seen complete
        bool used = false;             // read by a frame since the build (a rebuild must wait for the lanes)
        uint64_t first_call = 0;       // the first render call whose frame may read them (BeamCache::calls)
        uint64_t last_use_call = 0;    // the last render call whose frame was handed them
        uint64_t built_call = 0;       // the render call that started (resting view) or completed (moving camera) their build
    };
    struct BeamCache {
        BeamLists buf[2];
        int cur = 0;                     // the lists frames use; the other buffer is the one a build goes to
        uint64_t calls = 0;              // render calls that consulted the cache
        std::vector<uint32_t> last_key;  // key / position of the previous render call
        float last_pos[3] = { 0, 0, 0 };
        hipStream_t stream = nullptr;      // side stream (the builds of resting views)
        hipEvent_t ev_last_use = nullptr;  // scratch event of a rebuild (orders it after the lanes' frames in flight)
        // a moving camera's next lists, built a share per frame inside the frames' primary passes (FrameParams::beam_job)
        struct { bool active = false; BeamLists* dst = nullptr; std::vector<uint32_t> key; float centre[3] = { 0, 0, 0 }; float slack = 0.0f; float basis[9] = {}; float margin_px = 0.0f; uint32_t next_block = 0, n_blocks = 0; } inc;
        float last_vel[3] = { 0, 0, 0 };   // the camera's travel between the two calls before this one (its change bounds how far to trust the extrapolation)
        double last_turn[3] = { 0, 0, 0 }; // ... and its turn (rotation vector)
        float last_basis[9] = {};          // orientation of the previous render call
        bool have_vel = false;
    } beam;
    uint64_t scene_gen = 0;  // bumped by everything that changes what a ray can hit
    float slab_tiny = 1e-30f;  // SceneView::slab_tiny of the tree pt_build_accel made (a lane's private scene has its own: Lane::slab_tiny)
    float min_radius = 0.0f;  // smallest sphere of the scene set by pt_set_scene (bounds the slack of a moving camera's beam lists)

    // multi-GPU exchange (pt_comm_init / pt_gather): the RCCL communicator of this rank
    ncclComm_t comm = nullptr;
    uint32_t comm_rank = 0, comm_world = 1;

    // pt_physics_* (row N23): the rigid-sphere state and its tree (pt_api_physics.hip), used on `stream` only; null until pt_physics_create
    struct PtPhysicsState* physics = nullptr;
    // pt_physics_publish (row N24, spec S28): the ring of published poses -- publish_ring_size(n_lanes) slots of 2 * cap_n float4 (spheres,
    // then rotations) -- with a marker per slot on `stream`, and the bookkeeping of pt_publish_order.h.  want_prev: the take that the
    // call being made starts copies the previous pose too (pt_render_gbuffer_published).
    struct Published {
        PublishOrder order;
        float4* ring = nullptr;
        uint32_t cap_n = 0;
        hipEvent_t ev_slot[kPubMaxSlots] = {};
        bool want_prev = false;
    } pub;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool profiling = false;
    std::vector<EventPair> ev_pool;
    size_t ev_used = 0;
    History rb;
};

inline PtStatus fail(PtContext* ctx, PtStatus st, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    return st;
}

#define PT_HIP(ctx, expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            return fail(ctx, e_ == hipErrorOutOfMemory ? PT_ERR_OOM : PT_ERR_HIP,                      \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                            \
        }                                                                                              \
    } while (0)

// the buffer-argument rule (pt_args.h): a violation is the call's error
inline PtStatus buffers_ok(PtContext* ctx, const char* who, const BufferUse* use, uint32_t n)
{
    const std::string msg = check_buffers(who, use, n);
    return msg.empty() ? PT_OK : fail(ctx, PT_ERR_INVALID_ARG, msg);
}

template <typename T>
inline void free_dev(T*& p)
{
    if (p) { (void)hipFree(p); p = nullptr; }
}

// ---- the lane side of a frame and of its side passes: defined in pt_api.hip (each with its comment), used by pt_api_side.hip too; hidden: not part of the library's interface
#pragma GCC visibility push(hidden)
PtStatus validate_frame(PtContext* c), check_environment(PtContext* c), check_tree_lds(PtContext* c);
PtStatus rect_pixel_map(PtContext* c, const PtRect* rect, const char* who, PtRect& r, PixelMap& pm);
PixelMap make_pixel_map(uint32_t img_w, uint32_t img_h, const PtRect& r);
PtStatus denoise_out(PtContext* c, const PtDenoiserOutputs* outputs, const char* who, DenoiseOut& dn);
SceneView make_scene_view(const PtContext* c, const Lane* L = nullptr);
uint32_t side_pass_grid(const PtContext* c, uint32_t n_slots);
PtStatus side_pass_begin(PtContext* c, Lane& L, bool shared);
PtStatus lane_prev_pose_reserve(PtContext* c, Lane& L, uint32_t n);
PtStatus publish_lane_to_caller(PtContext* c, Lane& L, const char* who, PtStatus st);
EventPair* next_events(PtContext* c, int kind);
PtStatus staged_out_begin(PtContext* c, void* out, bool staged, size_t out_px, float4*& dev_out), staged_out_finish(PtContext* c, void* out, bool staged, size_t out_px);
#pragma GCC visibility pop

// launch() with its interval booked under `kind` while profiling is on (pt_get_profile: EventPair::kind); the second event is recorded after a failed launch too
template <typename F>
inline hipError_t profiled_launch(PtContext* c, hipStream_t stream, int kind, F&& launch)
{
    EventPair* ev = c->profiling ? next_events(c, kind) : nullptr;
    if (ev) (void)hipEventRecord(ev->a, stream);
    const hipError_t e = launch();
    if (ev) (void)hipEventRecord(ev->b, stream);
    return e;
}
